// Dynamic time warping between two sequences of frames of different lengths: what `fs2l synthesize --compare-to` scores
// free synthesis with (the MCD-DTW scheme of TTS evaluation, here on the model's own mel features).
//
//   frame_dist : cost[b][i][j] = sqrt(sum_c (a[b][i][c] - b[b][j][c])^2) on every utterance's own n_b x r_b box
//   dtw        : D[0][0] = c[0][0], D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) with the number of cells on
//                the chosen path carried along; the minimum is taken in that order with strict <, so a tie keeps the
//                diagonal, then the row above.  Adds and compares only: bit-exact from the cost matrix.
//   dtw_dirs   : dtw that also writes the predecessor taken at every cell (0 diagonal, 1 up, 2 left)
//   dtw_path   : the backtrack through those codes: per row of the box the first and last column on the path and the sum
//                of the row's path cells, from the last column towards the first
//
// MAS (aligner.hip) reads the previous row only, so a wavefront can take a whole row per step.  Here a cell also needs
// its LEFT neighbour of the same row: the cells of one anti-diagonal are what is independent.  One wavefront walks a
// strip of 64 columns with the rows skewed -- at step s lane t owns cell (s - t, j0 + t) -- so `up` is the lane's own
// previous result, `left` the neighbour's previous result (one DPP shift) and `diag` the `left` of the step before.
#include "common.h"

// no a * b + c becomes an fma below: the summation order of a cost is part of its definition (include/fs2hip.h)
#pragma clang fp contract(off)

namespace {

constexpr int DT_ROWS = 16;   // frame_dist: rows of `a` per workgroup (4 per wavefront)
constexpr int DT_STRIP = 64;  // columns per strip = lanes
constexpr int DT_CH = 8;      // dtw: rows of the cost matrix fetched ahead of the recursion

__device__ __forceinline__ int dt_clamp_len(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

// Tiled as attn_dist_kernel: 16 rows of a in LDS, 64 rows of b at a time (row stride C + 1: lane l reads bank l + c), a lane
// per column, four rows per wavefront.  Every element is the same C-term sum in ascending c, whatever the tile.
__global__ __launch_bounds__(256) void frame_dist_kernel(const float* __restrict__ a, const int* __restrict__ a_lens,
                                                          const float* __restrict__ b, const int* __restrict__ b_lens,
                                                          float* __restrict__ cost, int T1, int T2, int C) {
  extern __shared__ float sm[];  // as[16][C] | bs[64][C+1]
  float* as = sm;
  float* bs = sm + DT_ROWS * C;
  const int u = blockIdx.y, i0 = blockIdx.x * DT_ROWS;
  const int n = dt_clamp_len(a_lens[u], T1), r = dt_clamp_len(b_lens[u], T2);
  if (i0 >= n || r == 0) return;  // (uniform) a tile wholly outside the utterance's box
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < DT_ROWS * C; i += 256) {
    const int row = i / C, c = i % C;
    as[i] = (i0 + row < n) ? a[((long long)u * T1 + i0 + row) * C + c] : 0.f;
  }
  for (int j0 = 0; j0 < r; j0 += DT_STRIP) {
    __syncthreads();
    for (int i = threadIdx.x; i < DT_STRIP * C; i += 256) {
      const int row = i / C, c = i % C;
      bs[row * (C + 1) + c] = (j0 + row < r) ? b[((long long)u * T2 + j0 + row) * C + c] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* br = bs + lane * (C + 1);
    for (int c = 0; c < C; ++c) {
      const float bv = br[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = as[(wave + 4 * q) * C + c] - bv;
        acc[q] = acc[q] + d * d;
      }
    }
    if (j0 + lane < r) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + wave + 4 * q;
        if (i < n) cost[((long long)u * T1 + i) * T2 + j0 + lane] = sqrtf(acc[q]);
      }
    }
  }
}

// One wavefront per utterance.  LDS: ring[64][64] | colD[T1] | colS[T1] | (DIRS) dring[64][64] bytes.
//   ring  the strip's costs, a row per slot: lane t stores the 256-byte row segment's element t as the row arrives and reads
//         it back t steps later (ring[(s - t) % 64][t]: bank t, conflict-free); the global loads behind it run DT_CH rows
//         ahead in registers, so a step waits for LDS and never for memory.
//   col   (D, S)[i] of the strip's last column, left by lane 63 for lane 0 of the next strip.  Lane 0 gets them back 64
//         rows at a time (one read by all lanes, then a readlane per step); row i is read at step i and overwritten at
//         step i + 63 of the same strip, so the column is updated in place.
// DIRS: the predecessor taken at every cell is kept as well (0 diagonal, 1 up, 2 left; a byte per cell of dirs [B][T1][T2]).
//   dring [64][64] bytes behind the columns, the mirror of `ring`: lane t drops the code of cell (i, j0 + t) into
//         dring[i % 64][t]; at step s every lane of the strip is done with row s - (W - 1), and the wavefront stores that
//         row's W codes as one contiguous segment before lane 0 takes the slot again 64 rows later.  Without the ring
//         every step's byte stores would touch 64 different rows.
template <bool DIRS>
__global__ __launch_bounds__(64) void dtw_kernel(const float* __restrict__ cost, const int* __restrict__ lens1,
                                                 const int* __restrict__ lens2, float* __restrict__ total,
                                                 int* __restrict__ steps, unsigned char* __restrict__ dirs, int T1,
                                                 int T2) {
  extern __shared__ float sm[];
  float* ring = sm;
  float* colD = sm + DT_STRIP * DT_STRIP;
  int* colS = reinterpret_cast<int*>(colD + T1);
  unsigned char* dring = reinterpret_cast<unsigned char*>(colS + T1);  // (DIRS only: the launch reserves it)
  const int u = blockIdx.x, lane = threadIdx.x;
  const int n = dt_clamp_len(lens1[u], T1), r = dt_clamp_len(lens2[u], T2);
  if (n == 0 || r == 0) {
    if (lane == 0) {
      total[u] = 0.f;
      steps[u] = 0;
    }
    return;
  }
  const float* cb = cost + (long long)u * T1 * T2;
  unsigned char* db = DIRS ? dirs + (long long)u * T1 * T2 : nullptr;
  float upD = INFINITY;  // the lane's previous result: D / S of the cell above
  int upS = 0;
  int W = 0;
  for (int j0 = 0; j0 < r; j0 += DT_STRIP) {
    W = min(DT_STRIP, r - j0);       // columns of this strip
    const bool col_ok = lane < W;
    const int jl = j0 + (col_ok ? lane : W - 1);  // (a lane without a column loads the last one: nothing outside the box)
    const int nsteps = n + W - 1;
    const bool first = j0 == 0;
    upD = INFINITY;
    upS = 0;
    // cell (0, 0) has no predecessor and takes its cost as it is: a diagonal predecessor of cost 0 and 0 cells does that
    float dgD = (first && lane == 0) ? 0.f : INFINITY;
    int dgS = 0;
    __syncthreads();  // the last strip's column is complete
    ring[lane] = cb[jl];  // row 0
    float nx[DT_CH], cur[DT_CH];
    auto fetch = [&](int i0) {  // rows i0 .. i0 + DT_CH - 1, clamped to the last row (the surplus is never used)
#pragma unroll
      for (int k = 0; k < DT_CH; ++k) {
        const int i = i0 + k < n ? i0 + k : n - 1;
        nx[k] = cb[(long long)i * T2 + jl];
      }
    };
    fetch(1);
    float c = ring[((DT_STRIP - lane) & 63) * DT_STRIP + lane];  // step 0: row -t of lane t (only lane 0's is a cell)
    for (int s0 = 0; s0 < nsteps; s0 += DT_STRIP) {
      float lcD = INFINITY;  // lane k: the left neighbour of lane 0 at step s0 + k
      int lcS = 0;
      if (!first && s0 + lane < n) {
        lcD = colD[s0 + lane];
        lcS = colS[s0 + lane];
      }
      for (int k0 = 0; k0 < DT_STRIP && s0 + k0 < nsteps; k0 += DT_CH) {
        const int base = s0 + k0;
#pragma unroll
        for (int k = 0; k < DT_CH; ++k) cur[k] = nx[k];  // rows base + 1 .. base + DT_CH
        if (base + 1 + DT_CH < n) fetch(base + 1 + DT_CH);
#pragma unroll
        for (int k = 0; k < DT_CH; ++k) {
          const int s = base + k;
          if (s >= nsteps) break;  // uniform
          // row s + 1 takes the slot of row s - 63, which lane 63 has just used; the cell of the next step is read now
          ring[((s + 1) & 63) * DT_STRIP + lane] = cur[k];
          const float cnext = ring[((s + 1 - lane) & 63) * DT_STRIP + lane];
          const int i = s - lane;
          const float l0D = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lcD), k0 + k));
          const int l0S = __builtin_amdgcn_readlane(lcS, k0 + k);
          const float lfD = fs2_wave_shr1(upD, l0D);
          const int lfS = fs2_wave_shr1(upS, l0S);
          float best = dgD;
          int bs = dgS;
          unsigned char code = 0;
          if (upD < best) {
            best = upD;
            bs = upS;
            code = 1;
          }
          if (lfD < best) {
            best = lfD;
            bs = lfS;
            code = 2;
          }
          dgD = lfD;
          dgS = lfS;
          if (col_ok && i >= 0 && i < n) {
            upD = c + best;
            upS = bs + 1;
            if (lane == DT_STRIP - 1) {
              colD[i] = upD;
              colS[i] = upS;
            }
            if constexpr (DIRS) dring[(i & 63) * DT_STRIP + lane] = code;
          }
          if constexpr (DIRS) {
            // row s - (W - 1) is complete: lane t finished it at step s - (W - 1) + t <= s.  0 <= s - (W - 1) < n holds for
            // every step from W - 1 on (s <= n + W - 2), so every row of the strip leaves exactly once
            const int done = s - (W - 1);
            if (done >= 0 && col_ok) db[(long long)done * T2 + jl] = dring[(done & 63) * DT_STRIP + lane];
          }
          c = cnext;
        }
      }
    }
  }
  // the last strip's lane W - 1 owns column r - 1 and has kept row n - 1's result
  if (lane == W - 1) {
    total[u] = upD;
    steps[u] = upS;
  }
}

// The backtrack through `dirs`, one wavefront per utterance.  The walk is a chain of dependent reads, so it runs out of
// LDS: the wavefront fetches the DP_ROWS x 64 tile of codes and costs whose lower right corner is the walk's cell (a lane
// per column, every load of the tile in flight at once), then follows the path through the tile -- at least DP_ROWS moves
// -- before it pays a memory latency again.  All lanes walk together (uniform reads: LDS broadcasts), lane 0 writes a row's
// three results when the walk leaves the row.  A code the recursion cannot have written (dirs is the caller's memory)
// cannot lead outside the box: column 0 only goes up, row 0 only goes left, anything but 1 and 2 is a diagonal.
constexpr int DP_ROWS = 32;

__global__ __launch_bounds__(64) void dtw_path_kernel(const float* __restrict__ cost, const unsigned char* __restrict__ dirs,
                                                      const int* __restrict__ lens1, const int* __restrict__ lens2,
                                                      int* __restrict__ ref_first, int* __restrict__ ref_last,
                                                      float* __restrict__ frame_cost, int T1, int T2) {
  __shared__ float ct[DP_ROWS * DT_STRIP];
  __shared__ unsigned char dt[DP_ROWS * DT_STRIP];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int n = dt_clamp_len(lens1[u], T1), r = dt_clamp_len(lens2[u], T2);
  if (n == 0 || r == 0) return;
  const float* cb = cost + (long long)u * T1 * T2;
  const unsigned char* db = dirs + (long long)u * T1 * T2;
  const long long ob = (long long)u * T1;
  int i = n - 1, j = r - 1, last = j;
  float fc = 0.f;
  bool fresh = true;  // the walk has just entered row i: its sum starts from this cell's cost
  for (;;) {
    const int i0 = max(i - (DP_ROWS - 1), 0), j0 = max(j - (DT_STRIP - 1), 0);  // the tile: rows i0 .. i, columns j0 .. j
    __syncthreads();
    if (j0 + lane <= j) {
      for (int k = 0; k <= i - i0; ++k) {
        const long long at = (long long)(i0 + k) * T2 + j0 + lane;
        ct[k * DT_STRIP + lane] = cb[at];
        dt[k * DT_STRIP + lane] = db[at];
      }
    }
    __syncthreads();
    while (i >= i0 && j >= j0) {
      const int at = (i - i0) * DT_STRIP + (j - j0);
      const float c = ct[at];
      int d = __builtin_amdgcn_readfirstlane((int)dt[at]);
      fc = fresh ? c : fc + c;
      fresh = false;
      if (j == 0) d = 1;
      else if (i == 0) d = 2;
      if (d == 2) {
        --j;
        continue;
      }
      if (lane == 0) {
        ref_first[ob + i] = j;
        ref_last[ob + i] = last;
        frame_cost[ob + i] = fc;
      }
      if (i == 0) return;  // (0, 0): the path is complete
      --i;
      if (d != 1) --j;
      last = j;
      fresh = true;
    }
  }
}

}  // namespace

extern "C" int fs2hip_frame_dist(const float* a, const int* a_lens, const float* b, const int* b_lens, float* cost, int B,
                                 int T1, int T2, int C, void* stream) {
  if (!a || !a_lens || !b || !b_lens || !cost || B <= 0 || B > 65535 || T1 <= 0 || T2 <= 0 || C <= 0) return FS2HIP_EINVAL;
  if (C > FS2_FRAME_DIST_MAX_C) return FS2HIP_EINVAL;
  const size_t smem = (size_t)(DT_ROWS * C + DT_STRIP * (C + 1)) * sizeof(float);
  frame_dist_kernel<<<dim3((T1 + DT_ROWS - 1) / DT_ROWS, B), dim3(256), smem, (hipStream_t)stream>>>(a, a_lens, b, b_lens,
                                                                                                   cost, T1, T2, C);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_dtw(const float* cost, const int* lens1, const int* lens2, float* total, int* steps, int B, int T1,
                          int T2, void* stream) {
  if (!cost || !lens1 || !lens2 || !total || !steps || B <= 0 || T1 <= 0 || T2 <= 0) return FS2HIP_EINVAL;
  if (T1 > FS2_DTW_MAX_T1) return FS2HIP_EINVAL;
  const size_t smem = (size_t)(DT_STRIP * DT_STRIP + 2 * (size_t)T1) * sizeof(float);
  dtw_kernel<false><<<dim3(B), dim3(64), smem, (hipStream_t)stream>>>(cost, lens1, lens2, total, steps, nullptr, T1, T2);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_dtw_dirs(const float* cost, const int* lens1, const int* lens2, float* total, int* steps,
                               unsigned char* dirs, int B, int T1, int T2, void* stream) {
  if (!cost || !lens1 || !lens2 || !total || !steps || !dirs || B <= 0 || T1 <= 0 || T2 <= 0) return FS2HIP_EINVAL;
  if (T1 > FS2_DTW_PATH_MAX_T1) return FS2HIP_EINVAL;
  const size_t smem = (size_t)(DT_STRIP * DT_STRIP + 2 * (size_t)T1) * sizeof(float) + DT_STRIP * DT_STRIP;
  dtw_kernel<true><<<dim3(B), dim3(64), smem, (hipStream_t)stream>>>(cost, lens1, lens2, total, steps, dirs, T1, T2);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_dtw_path(const float* cost, const unsigned char* dirs, const int* lens1, const int* lens2,
                               int* ref_first, int* ref_last, float* frame_cost, int B, int T1, int T2, void* stream) {
  if (!cost || !dirs || !lens1 || !lens2 || !ref_first || !ref_last || !frame_cost || B <= 0 || T1 <= 0 || T2 <= 0)
    return FS2HIP_EINVAL;
  dtw_path_kernel<<<dim3(B), dim3(64), 0, (hipStream_t)stream>>>(cost, dirs, lens1, lens2, ref_first, ref_last, frame_cost,
                                                                 T1, T2);
  FS2_LAUNCH_CHECK();
  return 0;
}
