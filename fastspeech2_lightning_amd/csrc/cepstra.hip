// Cepstral coefficients of frame sequences: every valid row of x [B][T][C] against one table [K][C] that is the same for
// all rows (the caller's: hip.dct_table builds the orthonormal DCT-II rows 1..K, c0 dropped).  What MCD-DTW takes its
// frame distance on; here it feeds frame_dist + dtw (dtw.hip) with C = K.
//
//   cepstra : out[b][t][k] = sum_m x[b][t][m] * table[k][m]     for t < lens[b], k < K
//
// sum(lens) rows of C <= 204 floats meet K <= 64 table rows.  A row's C values are contiguous, so a lane that owned a row
// and read it from memory would touch 64 different lines per load.  A workgroup therefore stages 64 rows in LDS with an
// odd row stride (lane l reads bank l * stride + m: conflict-free in both 32-lane halves), a lane owns a row, and the four
// wavefronts split the K coefficients between them: a wavefront keeps its NK accumulators in registers over the whole
// sum, and table[k][m] is the same address for every lane (k comes from the wavefront's index: uniform loads, no LDS --
// a 64 x 204 table is 51 KiB and would not fit beside the row tile).  The results leave through the same LDS tile, which
// is free by then, so that the 64 x K block -- contiguous in out -- is stored in order.
#include "common.h"

// no a * b + c becomes an fma below: the summation order of a coefficient is part of its definition (include/fs2hip.h)
#pragma clang fp contract(off)

namespace {

constexpr int CP_ROWS = 64;  // rows per workgroup = lanes
constexpr int CP_WAVES = 4;

__device__ __forceinline__ int cp_clamp_len(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

// NK: coefficients per wavefront (CP_WAVES * NK >= K).  Wavefront w owns k = w * NK + q; an index past K - 1 is clamped to it
// (computed again, never stored), so the inner loop has no branch.
template <int NK>
__global__ __launch_bounds__(CP_ROWS * CP_WAVES) void cepstra_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                                     const float* __restrict__ table,
                                                                     float* __restrict__ out, int T, int C, int K,
                                                                     int tiles) {
  extern __shared__ float sm[];  // xs[64][C | 1], then (after the sums) os[64][K | 1] in the same place
  const int u = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * CP_ROWS;
  const int n = cp_clamp_len(lens[u], T);
  if (t0 >= n) return;  // (uniform) a tile wholly beyond the utterance's rows
  const int rows = min(CP_ROWS, n - t0);
  const int S = C | 1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const float* xb = x + ((long long)u * T + t0) * C;  // the tile's rows are one contiguous piece of x
  for (int i = threadIdx.x; i < rows * C; i += CP_ROWS * CP_WAVES) sm[(i / C) * S + i % C] = xb[i];
  __syncthreads();
  float acc[NK];
  const float* tk[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) {
    acc[q] = 0.f;
    tk[q] = table + (long long)min(wave * NK + q, K - 1) * C;
  }
  if (lane < rows) {
    const float* xr = sm + lane * S;
    for (int m = 0; m < C; ++m) {
      const float xv = xr[m];
#pragma unroll
      for (int q = 0; q < NK; ++q) acc[q] = acc[q] + xv * tk[q][m];
    }
  }
  __syncthreads();  // every wavefront is done with the rows: the tile becomes the output block
  const int So = K | 1;
  if (lane < rows) {
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      const int k = wave * NK + q;
      if (k < K) sm[lane * So + k] = acc[q];
    }
  }
  __syncthreads();
  float* ob = out + ((long long)u * T + t0) * K;
  for (int i = threadIdx.x; i < rows * K; i += CP_ROWS * CP_WAVES) ob[i] = sm[(i / K) * So + i % K];
}

}  // namespace

extern "C" int fs2hip_cepstra(const float* x, const int* lens, const float* table, float* out, int B, int T, int C, int K,
                              void* stream) {
  if (!x || !lens || !table || !out || B <= 0 || T <= 0 || C <= 0 || K <= 0) return FS2HIP_EINVAL;
  if (C > FS2_FRAME_DIST_MAX_C || K > FS2_CEPSTRA_MAX_K || K > C - 1) return FS2HIP_EINVAL;
  const int tiles = (T + CP_ROWS - 1) / CP_ROWS;
  if ((long long)B * tiles > 0x7fffffffLL) return FS2HIP_EINVAL;
  // K <= C - 1, so the output block [64][K | 1] is never larger than the row tile [64][C | 1]
  const size_t smem = (size_t)CP_ROWS * (C | 1) * sizeof(float);
  const dim3 grid((unsigned)(B * tiles)), block(CP_ROWS * CP_WAVES);
  const hipStream_t s = (hipStream_t)stream;
  const int per_wave = (K + CP_WAVES - 1) / CP_WAVES;
  if (per_wave <= 4) cepstra_kernel<4><<<grid, block, smem, s>>>(x, lens, table, out, T, C, K, tiles);
  else if (per_wave <= 8) cepstra_kernel<8><<<grid, block, smem, s>>>(x, lens, table, out, T, C, K, tiles);
  else cepstra_kernel<16><<<grid, block, smem, s>>>(x, lens, table, out, T, C, K, tiles);
  FS2_LAUNCH_CHECK();
  return 0;
}
