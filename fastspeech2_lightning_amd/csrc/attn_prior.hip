// The aligner's attention prior from the lengths (the reference's data pipeline stores it per utterance as
// attn/<name>-attn-prior.pt; synthetic.beta_binomial_prior is this project's definition of it):
//
//   prior[b][i][k] = betabinom(n = P - 1, a = scaling * (i + 1), b' = scaling * (M - i)).pmf(k)     i < M, k < P
//                  = exp( lgamma(n+1) - lgamma(k+1) - lgamma(n-k+1) + lgamma(k+a) + lgamma(n-k+b') - lgamma(n+a+b')
//                         - (lgamma(a) + lgamma(b') - lgamma(a+b')) )
//                  = 0 on the padding (i >= M or k >= P)
//
// fp64 throughout, one rounding to fp32 at the store: the lgamma terms reach about 7 000 at 1291 x 200 (one fp32 ulp there
// is 5e-4) and cancel to a log-probability of order 1 to 100.
//
// One wavefront per (b, i) row, lanes striding k (as attn_softmax_kernel walks the same tensor); a workgroup takes ROWS
// rows of ONE utterance.  Of the nine lgamma values five do not depend on k: lanes 0..4 fetch one each and a wave sum
// hands the row constant to every lane.  Three forms, which give the same bits (the same lgamma values summed in the same
// order) and differ in where the values come from:
//   IN_PLACE  every lgamma evaluated where it is used: four per element;
//   K_TABLE   lgamma(k+1) and lgamma(n-k+1) depend on k only: lfact[j] = lgamma(j + 1), j <= n, is built once per workgroup
//             in LDS -- two per element;
//   INT_TABLE scaling == 1 (what the model uses): a and b' are whole numbers, so EVERY argument is one and every term is an
//             entry of lfact[j], j <= n + M -- none per element, (M + P) / 256 per thread to build the table, which
//             32 rows share.
// Measured on the MI355X (profiles/attn_prior_kernel.md).
#include "common.h"

namespace {

enum { IN_PLACE = 0, K_TABLE = 1, INT_TABLE = 2 };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int MODE, int ROWS>
__global__ __launch_bounds__(256) void attn_prior_kernel(const int* __restrict__ mel_lens, const int* __restrict__ src_lens,
                                                          float* __restrict__ prior, int Tm, int Ts, int chunks,
                                                          double scaling) {
  extern __shared__ double lfact[];  // lfact[j] = lgamma(j + 1): j < P (K_TABLE), j < P + M (INT_TABLE)
  const int b = blockIdx.x / chunks, i0 = (blockIdx.x % chunks) * ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int M = mel_lens[b], P = src_lens[b];
  M = M < 0 ? 0 : (M > Tm ? Tm : M);
  P = P < 0 ? 0 : (P > Ts ? Ts : P);
  const int n = P - 1;
  if (MODE != IN_PLACE) {
    if (i0 < M) {  // (uniform per workgroup; a workgroup of padding rows needs no table)
      const int entries = MODE == INT_TABLE ? P + M : P;
      for (int j = threadIdx.x; j < entries; j += 256) lfact[j] = lgamma((double)j + 1.0);
    }
    __syncthreads();
  }
  float* out = prior + (long long)b * Tm * Ts;
  for (int r = wave; r < ROWS; r += 4) {
    const int i = i0 + r;
    if (i >= Tm) break;
    float* row = out + (long long)i * Ts;
    if (i >= M || P == 0) {
      for (int k = lane; k < Ts; k += 64) row[k] = 0.f;
      continue;
    }
    const double a = scaling * (double)(i + 1), bb = scaling * (double)(M - i);
    // the row's constant: + lgamma(n+1) - lgamma(n+a+b') - lgamma(a) - lgamma(b') + lgamma(a+b'), a term per lane
    double c = 0.0;
    if (lane < 5) {
      double v;
      if (MODE == INT_TABLE) {  // a = i + 1, b' = M - i
        v = lfact[lane == 0 ? n : lane == 1 ? n + M : lane == 2 ? i : lane == 3 ? M - i - 1 : M];
      } else {
        v = lgamma(lane == 0 ? (double)n + 1.0 : lane == 1 ? (double)n + a + bb : lane == 2 ? a : lane == 3 ? bb : a + bb);
      }
      c = (lane == 0 || lane == 4) ? v : -v;
    }
    c = wave_sum_f64(c);
    for (int k = lane; k < Ts; k += 64) {
      float p = 0.f;
      if (k < P) {
        double lk, lnk, la, lb;  // lgamma of k + 1, n - k + 1, k + a, n - k + b'
        if (MODE == IN_PLACE) {
          lk = lgamma((double)k + 1.0);
          lnk = lgamma((double)(n - k) + 1.0);
        } else {
          lk = lfact[k];
          lnk = lfact[n - k];
        }
        if (MODE == INT_TABLE) {
          la = lfact[k + i];                  // k + a - 1 <= n + M - 1
          lb = lfact[n - k + M - i - 1];      // n - k + b' - 1 <= n + M - 1
        } else {
          la = lgamma((double)k + a);
          lb = lgamma((double)(n - k) + bb);
        }
        p = (float)exp(c - lk - lnk + la + lb);
      }
      row[k] = p;
    }
  }
}

template <int MODE, int ROWS>
int launch(const int* mel_lens, const int* src_lens, float* prior, int B, int Tm, int Ts, float scaling, size_t smem,
           hipStream_t s) {
  const int chunks = (Tm + ROWS - 1) / ROWS;
  const long long blocks = (long long)B * chunks;
  if (blocks > 0x7fffffffLL) return FS2HIP_EINVAL;
  attn_prior_kernel<MODE, ROWS><<<dim3((unsigned)blocks), dim3(256), smem, s>>>(mel_lens, src_lens, prior, Tm, Ts, chunks,
                                                                                 (double)scaling);
  FS2_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int fs2hip_attn_prior(const int* mel_lens, const int* src_lens, float* prior, int B, int Tm, int Ts, float scaling,
                                 void* stream) {
  if (!mel_lens || !src_lens || !prior || B <= 0 || Tm <= 0 || Ts <= 0 || !(scaling > 0.f)) return FS2HIP_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  // FS2_ATTN_PRIOR_TABLE = 0 / 1: at most the in-place / the k-table form (measurement aid, tests); a table that does not
  // fit 48 KB of LDS falls back the same way
  const char* env = getenv("FS2_ATTN_PRIOR_TABLE");
  const int most = env ? atoi(env) : INT_TABLE;
  const size_t lds = 48 * 1024, k_bytes = (size_t)Ts * sizeof(double), int_bytes = ((size_t)Ts + Tm) * sizeof(double);
  if (most >= INT_TABLE && scaling == 1.f && int_bytes <= lds)
    return launch<INT_TABLE, 32>(mel_lens, src_lens, prior, B, Tm, Ts, scaling, int_bytes, s);
  if (most >= K_TABLE && k_bytes <= lds) return launch<K_TABLE, 16>(mel_lens, src_lens, prior, B, Tm, Ts, scaling, k_bytes, s);
  return launch<IN_PLACE, 16>(mel_lens, src_lens, prior, B, Tm, Ts, scaling, 0, s);
}
