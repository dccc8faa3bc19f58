// BatchNorm1d over the channel (last) dimension of a dense [M][C] matrix (M = B*T rows, padding
// rows included -- the reference normalises over them too), training and evaluation mode, fused
// with the activation (+dropout) that follows it.
// Replaces nn.BatchNorm1d (+SiLU) in torchaudio's Conformer conv module (call sites
// fs2/model.py:193, :241) and nn.BatchNorm1d + tanh + F.dropout in PostNet (fs2/layers.py:204-212).
//
//   statistics : colstats (or the depthwise-conv kernel's fused partials)  -> partial[nparts][2][C] = per-part
//                (mean, sum of squared deviations), computed on pivot-shifted values
//   finalize   : Chan merge of the parts in fp64 (64 channels x 16 part lanes per workgroup),
//                running-stat update, per-channel scale/shift
//   apply      : out = dropout(act(y*scale + shift))                         (one pass)
//   backward   : reduce (sum dz, sum dz*xhat) -> finalize (dgamma, dbeta, means) -> apply
// The statistics passes sweep whole rows (contiguous >= 1 KiB per wavefront instruction).
// The *_lens kernels are the same passes over the valid positions of a [B][H][W][C] tensor only (lengths in device memory).
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int CS_ROWS = 32;   // rows per workgroup in the column-statistics passes (more for very tall matrices,
                              // so that the fp64 finish never walks more than ~2048 partial rows: cs_rows())
__host__ __device__ inline int cs_rows(int M) { return CS_ROWS * ((M + CS_ROWS * 2048 - 1) / (CS_ROWS * 2048)); }

// thread -> (row lane rl, float4 column c4): tpr = C/4 threads per row, rpi = 256/tpr rows per pass
struct WideMap {
  int tpr, rpi;
};

// four consecutive elements starting at element index e (a multiple of 4) of a tensor that is fp32 (IB = false) or
// bf16 (IB = true) in memory
template <bool IB>
__device__ __forceinline__ float4 bn_ld4(const void* p, long long e) {
  if constexpr (IB) {
    const uint2 u = *reinterpret_cast<const uint2*>((const unsigned short*)p + e);
    return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                       __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
  } else {
    return *reinterpret_cast<const float4*>((const float*)p + e);
  }
}

// Per-stripe (mean, M2 = sum of squared deviations) per channel.  Sums are taken of d = y - pivot with the stripe's
// first row as the pivot, so M2 = sum d^2 - (sum d)^2 / n subtracts two numbers of the size of the variance, not of
// the squared mean (a plain E[y^2] - E[y]^2 in fp32 loses the variance of a channel whose |mean| >> std; torch's
// BatchNorm is Welford).  bn_finalize merges the stripes with Chan's formula in fp64.
template <bool IB>
__global__ __launch_bounds__(256) void colstats_wide_kernel(const void* __restrict__ y, int M, int C,
                                                             float* __restrict__ partial, WideMap wm) {
  __shared__ float4 red[2][256];
  const int tid = threadIdx.x;
  const int rl = tid / wm.tpr, c4 = tid - rl * wm.tpr;
  const int rows = cs_rows(M);
  const int r0 = blockIdx.x * rows, r1 = min(M, r0 + rows);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0), pv = make_float4(0, 0, 0, 0);
  if (rl < wm.rpi) {
    pv = bn_ld4<IB>(y, (long long)r0 * C + c4 * 4);
    auto add = [&](float4 v) {
      v.x -= pv.x; v.y -= pv.y; v.z -= pv.z; v.w -= pv.w;
      s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
      s2.x += v.x * v.x; s2.y += v.y * v.y; s2.z += v.z * v.z; s2.w += v.w * v.w;
    };
    int r = r0 + rl;
    for (; r + 3 * wm.rpi < r1; r += 4 * wm.rpi) {  // four rows' loads in flight per thread, added in row order
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = bn_ld4<IB>(y, (long long)(r + u * wm.rpi) * C + c4 * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) add(v[u]);
    }
    for (; r < r1; r += wm.rpi) add(bn_ld4<IB>(y, (long long)r * C + c4 * 4));
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < wm.rpi; ++l) {
      float4 a = red[0][l * wm.tpr + c4], b = red[1][l * wm.tpr + c4];
      s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
      s2.x += b.x; s2.y += b.y; s2.z += b.z; s2.w += b.w;
    }
    const float inv = 1.f / (float)(r1 - r0);
    float4 mean, m2;
    mean.x = pv.x + s1.x * inv; m2.x = fmaxf(s2.x - s1.x * s1.x * inv, 0.f);
    mean.y = pv.y + s1.y * inv; m2.y = fmaxf(s2.y - s1.y * s1.y * inv, 0.f);
    mean.z = pv.z + s1.z * inv; m2.z = fmaxf(s2.z - s1.z * s1.z * inv, 0.f);
    mean.w = pv.w + s1.w * inv; m2.w = fmaxf(s2.w - s1.w * s1.w * inv, 0.f);
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 0) * C + c4 * 4) = mean;
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * C + c4 * 4) = m2;
  }
}

// The finalize kernels: one 1024-thread workgroup per 16 channels, thread = (channel tid & 15, part lane tid >> 4):
// 64 part lanes with four independent loads in flight each (these kernels are pure latency: a few hundred parts per
// channel), fp64 sums merged in a fixed order -- the lane pairs of a wavefront, then the 16 wavefronts through LDS.
constexpr int FIN_CH = 16, FIN_LANES = 64;
// every thread gets the block's sum of v for its channel
__device__ __forceinline__ double fin_sum(double v, double (&red)[16][FIN_CH]) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  const int ch = threadIdx.x & 15, w = threadIdx.x >> 6;
  __syncthreads();  // (the previous call's readers are done with red)
  if ((threadIdx.x & 63) < 16) red[w][ch] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int l = 0; l < 16; ++l) s += red[l][ch];
  return s;
}
// sum over this thread's parts of f(p, partial[p][0][c], partial[p][1][c]) -> (a, b)
template <class F>
__device__ __forceinline__ void fin_parts(const float* __restrict__ partial, int nparts, int C, int c, F&& f, double& a,
                                          double& b) {
  a = 0.0;
  b = 0.0;
  if (c >= C) return;
  int p = threadIdx.x >> 4;
  for (; p + 3 * FIN_LANES < nparts; p += 4 * FIN_LANES) {
    float u[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u[k] = partial[((long long)(p + k * FIN_LANES) * 2 + 0) * C + c];
      v[k] = partial[((long long)(p + k * FIN_LANES) * 2 + 1) * C + c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) f(p + k * FIN_LANES, u[k], v[k], a, b);
  }
  float u[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (p + k * FIN_LANES < nparts) {
      u[k] = partial[((long long)(p + k * FIN_LANES) * 2 + 0) * C + c];
      v[k] = partial[((long long)(p + k * FIN_LANES) * 2 + 1) * C + c];
    }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (p + k * FIN_LANES < nparts) f(p + k * FIN_LANES, u[k], v[k], a, b);
}

// rows of part p (bn_finalize): the parts tile groups of group_rows rows (one group = the whole matrix for colstats,
// one utterance for the depthwise conv's fused statistics) in stripes of part_rows

// stats layout (per channel): [0]=scale (gamma*invstd) [1]=shift (beta-mean*scale) [2]=mean [3]=invstd [4]=eps
// training: Chan's parallel merge of the per-part (n, mean, M2) in fp64 -- mean = sum n_p mean_p / N, then
// M2 = sum [M2_p + n_p (mean_p - mean)^2]
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ partial, int nparts,
                                                            long long count, int part_rows, int group_rows,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ rmean,
                                                            float* __restrict__ rvar, float momentum, float eps,
                                                            int training, float* __restrict__ stats, int C) {
  __shared__ double red[16][FIN_CH];
  const int c = blockIdx.x * FIN_CH + (threadIdx.x & 15);
  const bool writer = threadIdx.x < FIN_CH && c < C;
  float mean = 0.f, invstd = 0.f;
  if (training) {
    const int ppg = (group_rows + part_rows - 1) / part_rows;
    auto cnt = [&](int p) { return (double)min(part_rows, group_rows - (p % ppg) * part_rows); };
    double a, b;
    fin_parts(partial, nparts, C, c, [&](int p, float u, float, double& x, double&) { x += cnt(p) * (double)u; }, a, b);
    const double mu = fin_sum(a, red) / (double)count;
    fin_parts(partial, nparts, C, c, [&](int p, float u, float v, double& x, double&) {
      const double d = (double)u - mu;
      x += (double)v + cnt(p) * d * d;
    }, a, b);
    const double m2 = fin_sum(a, red);
    if (!writer) return;
    double var = m2 / (double)count;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    invstd = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {
      double unbiased = count > 1 ? var * (double)count / (double)(count - 1) : var;
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
    }
  } else {
    if (!writer) return;
    mean = rmean[c];
    invstd = 1.f / sqrtf(rvar[c] + eps);
  }
  const float sc = gamma[c] * invstd;
  stats[0 * C + c] = sc;
  stats[1 * C + c] = beta[c] - mean * sc;
  stats[2 * C + c] = mean;
  stats[3 * C + c] = invstd;
  stats[4 * C + c] = eps;  // (read by bn_bwd_small_kernel, which recomputes the variance in fp64)
}

// four fp32 -> four bf16 (round to nearest even), 8 bytes
typedef __bf16 bn_bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_bf16x4(void* dst, long long i4, float4 v) {
  const f32x4 f = {v.x, v.y, v.z, v.w};
  reinterpret_cast<bn_bf16x4*>(dst)[i4] = __builtin_convertvector(f, bn_bf16x4);
}

// out_b (may be null): a bf16 copy of the output for a GEMM that takes bf16 operands from memory (operand_bf16 == 3)
// IB: y is a bf16 tensor (the depthwise convolution's bf16 result)
template <bool IB>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const void* __restrict__ y, const float* __restrict__ stats,
                                                          float* __restrict__ out, void* __restrict__ out_b, long long n4,
                                                          int C, int act, Fs2Drop drop_in) {
  const Fs2Drop drop = fs2_resolve_drop(drop_in);
  const int c4n = C >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    float4 v = bn_ld4<IB>(y, i * 4);
    float4 sc = reinterpret_cast<const float4*>(stats)[c4];
    float4 sh = reinterpret_cast<const float4*>(stats + C)[c4];
    float4 o;
    o.x = fs2_act(act, fmaf(v.x, sc.x, sh.x)) * fs2_drop_factor(drop, (unsigned long long)(i * 4 + 0));
    o.y = fs2_act(act, fmaf(v.y, sc.y, sh.y)) * fs2_drop_factor(drop, (unsigned long long)(i * 4 + 1));
    o.z = fs2_act(act, fmaf(v.z, sc.z, sh.z)) * fs2_drop_factor(drop, (unsigned long long)(i * 4 + 2));
    o.w = fs2_act(act, fmaf(v.w, sc.w, sh.w)) * fs2_drop_factor(drop, (unsigned long long)(i * 4 + 3));
    if (out) reinterpret_cast<float4*>(out)[i] = o;   // (null: the activations exist only as the bf16 operand)
    if (out_b) store_bf16x4(out_b, i, o);
  }
}

__device__ __forceinline__ float dz_of(float dout, float v, float sc, float sh, int act, const Fs2Drop& drop,
                                       unsigned long long idx) {
  return dout * fs2_drop_factor(drop, idx) * fs2_dact(act, fmaf(v, sc, sh));
}

// (without dropout: the same value, the factor being exactly 1)
__device__ __forceinline__ float dz_of(float dout, float v, float sc, float sh, int act) {
  return dout * fs2_dact(act, fmaf(v, sc, sh));
}

// dz = dout * dropmask * act'(y*scale+shift) ; partial[blk][0][C] = sum dz, [1] = sum dz * xhat
template <bool IB, bool DB>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const void* __restrict__ dout, const void* __restrict__ y,
                                                             const float* __restrict__ stats, int M, int C, int act,
                                                             Fs2Drop drop_in, float* __restrict__ partial, WideMap wm) {
  const Fs2Drop drop = fs2_resolve_drop(drop_in);
  __shared__ float4 red[2][256];
  const int tid = threadIdx.x;
  const int rl = tid / wm.tpr, c4 = tid - rl * wm.tpr;
  const int rows = cs_rows(M);
  const int r0 = blockIdx.x * rows, r1 = min(M, r0 + rows);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0);
  if (rl < wm.rpi) {
    const float4 sc = reinterpret_cast<const float4*>(stats)[c4], sh = reinterpret_cast<const float4*>(stats + C)[c4];
    const float4 mu = reinterpret_cast<const float4*>(stats + 2 * C)[c4], is = reinterpret_cast<const float4*>(stats + 3 * C)[c4];
    auto add = [&](long long idx, const float4& v, const float4& d) {
      float dz;
      dz = dz_of(d.x, v.x, sc.x, sh.x, act, drop, idx + 0); s1.x += dz; s2.x += dz * (v.x - mu.x) * is.x;
      dz = dz_of(d.y, v.y, sc.y, sh.y, act, drop, idx + 1); s1.y += dz; s2.y += dz * (v.y - mu.y) * is.y;
      dz = dz_of(d.z, v.z, sc.z, sh.z, act, drop, idx + 2); s1.z += dz; s2.z += dz * (v.z - mu.z) * is.z;
      dz = dz_of(d.w, v.w, sc.w, sh.w, act, drop, idx + 3); s1.w += dz; s2.w += dz * (v.w - mu.w) * is.w;
    };
    int r = r0 + rl;
    // a part is one workgroup per 64 rows, i.e. about five wavefronts per CU: four rows' loads in flight per thread
    // (the sums are added in the same row order as before)
    for (; r + 3 * wm.rpi < r1; r += 4 * wm.rpi) {
      long long idx[4];
      float4 v[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        idx[u] = (long long)(r + u * wm.rpi) * C + c4 * 4;
        v[u] = bn_ld4<IB>(y, idx[u]);
        d[u] = bn_ld4<DB>(dout, idx[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) add(idx[u], v[u], d[u]);
    }
    for (; r < r1; r += wm.rpi) {
      const long long idx = (long long)r * C + c4 * 4;
      add(idx, bn_ld4<IB>(y, idx), bn_ld4<DB>(dout, idx));
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < wm.rpi; ++l) {
      float4 a = red[0][l * wm.tpr + c4], b = red[1][l * wm.tpr + c4];
      s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
      s2.x += b.x; s2.y += b.y; s2.z += b.z; s2.w += b.w;
    }
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 0) * C + c4 * 4) = s1;
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * C + c4 * 4) = s2;
  }
}

// dgamma = sum dz*xhat, dbeta = sum dz; coef[0][c] = mean(dz), coef[1][c] = mean(dz*xhat)
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nparts,
                                                                long long count, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, float* __restrict__ coef, int C) {
  __shared__ double red[16][FIN_CH];
  const int c = blockIdx.x * FIN_CH + (threadIdx.x & 15);
  double a, b;
  fin_parts(partial, nparts, C, c, [&](int, float u, float v, double& x, double& y) { x += (double)u; y += (double)v; }, a, b);
  const double s1 = fin_sum(a, red), s2 = fin_sum(b, red);
  if (threadIdx.x >= FIN_CH || c >= C) return;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  coef[c] = (float)(s1 / (double)count);
  coef[C + c] = (float)(s2 / (double)count);
}

// dy = scale * (dz - mean(dz) - xhat * mean(dz*xhat))   [training]   or scale * dz   [eval]
template <bool IB, bool DB>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const void* __restrict__ dout, const void* __restrict__ y,
                                                            const float* __restrict__ stats, const float* __restrict__ coef,
                                                            float* __restrict__ dy, void* __restrict__ dy_b, long long n4,
                                                            int C, int act, Fs2Drop drop_in, int training) {
  const Fs2Drop drop = fs2_resolve_drop(drop_in);
  const int c4n = C >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    const float4 sc = reinterpret_cast<const float4*>(stats)[c4], sh = reinterpret_cast<const float4*>(stats + C)[c4];
    const float4 v = bn_ld4<IB>(y, i * 4);
    const float4 d = bn_ld4<DB>(dout, i * 4);
    float4 dz;
    dz.x = dz_of(d.x, v.x, sc.x, sh.x, act, drop, (unsigned long long)(i * 4 + 0));
    dz.y = dz_of(d.y, v.y, sc.y, sh.y, act, drop, (unsigned long long)(i * 4 + 1));
    dz.z = dz_of(d.z, v.z, sc.z, sh.z, act, drop, (unsigned long long)(i * 4 + 2));
    dz.w = dz_of(d.w, v.w, sc.w, sh.w, act, drop, (unsigned long long)(i * 4 + 3));
    if (training) {
      const float4 mu = reinterpret_cast<const float4*>(stats + 2 * C)[c4], is = reinterpret_cast<const float4*>(stats + 3 * C)[c4];
      const float4 k1 = reinterpret_cast<const float4*>(coef)[c4], k2 = reinterpret_cast<const float4*>(coef + C)[c4];
      dz.x = dz.x - k1.x - (v.x - mu.x) * is.x * k2.x;
      dz.y = dz.y - k1.y - (v.y - mu.y) * is.y * k2.y;
      dz.z = dz.z - k1.z - (v.z - mu.z) * is.z * k2.z;
      dz.w = dz.w - k1.w - (v.w - mu.w) * is.w * k2.w;
    }
    const float4 o = make_float4(sc.x * dz.x, sc.y * dz.y, sc.z * dz.z, sc.w * dz.w);
    if (dy) reinterpret_cast<float4*>(dy)[i] = o;
    if (dy_b) store_bf16x4(dy_b, i, o);
  }
}

// Training-mode backward of a batch of FEW rows (the last GST convolution sees B * 2 of them), one thread per channel,
// in fp64.  dy = scale * (dz - mean(dz) - xhat * mean(dz * xhat)) removes from dz its components along 1 and xhat: with
// M rows that leaves M - 2 of M dimensions, and with two rows nothing but (dz_0 - dz_1) / 2 * eps / (var + eps) --
// terms of size 1 cancelling to 1e-3 or less, of which the fp32 kernels above (fp32 mean and invstd, fp32 xhat) keep
// three digits.  Here mean and variance are taken again from y in fp64, so xhat, both means and the difference carry
// fp64 rounding; dz itself (and the activation's argument, which must decide as the forward pass did) stays fp32.
constexpr int BN_SMALL_ROWS = 16;
__global__ __launch_bounds__(64) void bn_bwd_small_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                           const float* __restrict__ stats, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ dy, int M, int C,
                                                           int act, Fs2Drop drop_in) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const Fs2Drop drop = fs2_resolve_drop(drop_in);
  const float sc = stats[c], sh = stats[C + c];
  const double eps = (double)stats[4 * C + c];
  double mu = 0.0, m2 = 0.0;
  for (int r = 0; r < M; ++r) mu += (double)y[(long long)r * C + c];
  mu /= (double)M;
  for (int r = 0; r < M; ++r) {
    const double d = (double)y[(long long)r * C + c] - mu;
    m2 += d * d;
  }
  const double invstd = 1.0 / sqrt(m2 / (double)M + eps);
  double s1 = 0.0, s2 = 0.0;
  for (int r = 0; r < M; ++r) {
    const long long idx = (long long)r * C + c;
    const double dz = (double)dz_of(dout[idx], y[idx], sc, sh, act, drop, (unsigned long long)idx);
    s1 += dz;
    s2 += dz * (((double)y[idx] - mu) * invstd);
  }
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  const double k1 = s1 / (double)M, k2 = s2 / (double)M;
  for (int r = 0; r < M; ++r) {
    const long long idx = (long long)r * C + c;
    const double dz = (double)dz_of(dout[idx], y[idx], sc, sh, act, drop, (unsigned long long)idx);
    dy[idx] = (float)((double)sc * (dz - k1 - ((double)y[idx] - mu) * invstd * k2));
  }
}

// ---- BatchNorm over the VALID positions of y [B][H][W][C] only (length-aware training of the GST style encoder) ----
// Utterance b keeps its first L = clamp(lens[b], 0, H) rows of H: seen as a [B * H * W][C] matrix, ONE contiguous range
// of L * W rows starting at row b * H * W.  Every utterance's H * W rows are tiled in stripes of `pr` rows (ppu stripes
// per utterance, part index b * ppu + p); a stripe's row count min(pr, L * W - p * pr) -- possibly 0 -- and the total
// count come from lens in device memory, and no row at or beyond L * W is ever addressed.  The arithmetic is that of
// the kernels above: pivot-shifted per-stripe sums, Chan merge in fp64.
struct LensMap {
  int H, W, HW, pr, ppu;
};
__device__ __forceinline__ int lens_valid_rows(const int* __restrict__ lens, int b, const LensMap& lm) {
  const int l = lens[b];
  return (l < 0 ? 0 : (l > lm.H ? lm.H : l)) * lm.W;
}
__device__ __forceinline__ long long lens_count(const int* __restrict__ lens, int B, const LensMap& lm) {
  long long n = 0;
  for (int b = 0; b < B; ++b) n += lens_valid_rows(lens, b, lm);
  return n;
}

__global__ __launch_bounds__(256) void colstats_lens_kernel(const float* __restrict__ y, const int* __restrict__ lens,
                                                             int C, float* __restrict__ partial, WideMap wm, LensMap lm) {
  __shared__ float4 red[2][256];
  const int tid = threadIdx.x;
  const int rl = tid / wm.tpr, c4 = tid - rl * wm.tpr;
  const int b = blockIdx.x / lm.ppu, p = blockIdx.x - b * lm.ppu;
  const int nv = lens_valid_rows(lens, b, lm);
  const int r0 = p * lm.pr, r1 = min(nv, r0 + lm.pr);
  if (r1 <= r0) {  // (uniform over the workgroup) an empty stripe: count 0, never read
    if (rl == 0) {
      *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 0) * C + c4 * 4) = make_float4(0, 0, 0, 0);
      *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * C + c4 * 4) = make_float4(0, 0, 0, 0);
    }
    return;
  }
  const float* yb = y + (long long)b * lm.HW * C;
  float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0), pv = make_float4(0, 0, 0, 0);
  if (rl < wm.rpi) {
    pv = *reinterpret_cast<const float4*>(yb + (long long)r0 * C + c4 * 4);
    for (int r = r0 + rl; r < r1; r += wm.rpi) {
      float4 v = *reinterpret_cast<const float4*>(yb + (long long)r * C + c4 * 4);
      v.x -= pv.x; v.y -= pv.y; v.z -= pv.z; v.w -= pv.w;
      s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
      s2.x += v.x * v.x; s2.y += v.y * v.y; s2.z += v.z * v.z; s2.w += v.w * v.w;
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < wm.rpi; ++l) {
      float4 a = red[0][l * wm.tpr + c4], e = red[1][l * wm.tpr + c4];
      s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
      s2.x += e.x; s2.y += e.y; s2.z += e.z; s2.w += e.w;
    }
    const float inv = 1.f / (float)(r1 - r0);
    float4 mean, m2;
    mean.x = pv.x + s1.x * inv; m2.x = fmaxf(s2.x - s1.x * s1.x * inv, 0.f);
    mean.y = pv.y + s1.y * inv; m2.y = fmaxf(s2.y - s1.y * s1.y * inv, 0.f);
    mean.z = pv.z + s1.z * inv; m2.z = fmaxf(s2.z - s1.z * s1.z * inv, 0.f);
    mean.w = pv.w + s1.w * inv; m2.w = fmaxf(s2.w - s1.w * s1.w * inv, 0.f);
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 0) * C + c4 * 4) = mean;
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * C + c4 * 4) = m2;
  }
}

// bn_finalize_kernel's training branch with the stripes' counts and the total count N taken from lens.  N = 0 (no
// valid position at all): mean 0, variance 0, running buffers untouched.
__global__ __launch_bounds__(1024) void bn_finalize_lens_kernel(const float* __restrict__ partial,
                                                                 const int* __restrict__ lens, int B,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ rmean,
                                                                 float* __restrict__ rvar, float momentum, float eps,
                                                                 float* __restrict__ stats, int C, LensMap lm) {
  __shared__ double red[16][FIN_CH];
  const int c = blockIdx.x * FIN_CH + (threadIdx.x & 15);
  const bool writer = threadIdx.x < FIN_CH && c < C;
  const long long count = lens_count(lens, B, lm);
  const int nparts = B * lm.ppu;
  auto cnt = [&](int p) {
    const int b = p / lm.ppu;
    return (double)max(0, min(lm.pr, lens_valid_rows(lens, b, lm) - (p - b * lm.ppu) * lm.pr));
  };
  double a, e;
  fin_parts(partial, nparts, C, c, [&](int p, float u, float, double& x, double&) { x += cnt(p) * (double)u; }, a, e);
  const double sum = fin_sum(a, red);
  const double mu = count > 0 ? sum / (double)count : 0.0;
  fin_parts(partial, nparts, C, c, [&](int p, float u, float v, double& x, double&) {
    const double d = (double)u - mu;
    x += (double)v + cnt(p) * d * d;
  }, a, e);
  const double m2 = fin_sum(a, red);
  if (!writer) return;
  double var = count > 0 ? m2 / (double)count : 0.0;
  if (var < 0.0) var = 0.0;
  const float mean = (float)mu, invstd = (float)(1.0 / sqrt(var + (double)eps));
  if (rmean && count > 0) {
    double unbiased = count > 1 ? var * (double)count / (double)(count - 1) : var;
    rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
  }
  const float sc = gamma[c] * invstd;
  stats[0 * C + c] = sc;
  stats[1 * C + c] = beta[c] - mean * sc;
  stats[2 * C + c] = mean;
  stats[3 * C + c] = invstd;
  stats[4 * C + c] = eps;
}

// bn_bwd_reduce_kernel over the valid rows of a stripe (no dropout): partial[part][0][C] = sum dz, [1] = sum dz * xhat
__global__ __launch_bounds__(256) void bn_bwd_reduce_lens_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                                  const float* __restrict__ stats,
                                                                  const int* __restrict__ lens, int C, int act,
                                                                  float* __restrict__ partial, WideMap wm, LensMap lm) {
  __shared__ float4 red[2][256];
  const int tid = threadIdx.x;
  const int rl = tid / wm.tpr, c4 = tid - rl * wm.tpr;
  const int b = blockIdx.x / lm.ppu, p = blockIdx.x - b * lm.ppu;
  const int nv = lens_valid_rows(lens, b, lm);
  const int r0 = p * lm.pr, r1 = min(nv, r0 + lm.pr);
  float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0);
  if (rl < wm.rpi && r0 < r1) {
    const float4 sc = reinterpret_cast<const float4*>(stats)[c4], sh = reinterpret_cast<const float4*>(stats + C)[c4];
    const float4 mu = reinterpret_cast<const float4*>(stats + 2 * C)[c4], is = reinterpret_cast<const float4*>(stats + 3 * C)[c4];
    for (int r = r0 + rl; r < r1; r += wm.rpi) {
      const long long idx = ((long long)b * lm.HW + r) * C + c4 * 4;
      const float4 v = *reinterpret_cast<const float4*>(y + idx), d = *reinterpret_cast<const float4*>(dout + idx);
      float dz;
      dz = dz_of(d.x, v.x, sc.x, sh.x, act); s1.x += dz; s2.x += dz * (v.x - mu.x) * is.x;
      dz = dz_of(d.y, v.y, sc.y, sh.y, act); s1.y += dz; s2.y += dz * (v.y - mu.y) * is.y;
      dz = dz_of(d.z, v.z, sc.z, sh.z, act); s1.z += dz; s2.z += dz * (v.z - mu.z) * is.z;
      dz = dz_of(d.w, v.w, sc.w, sh.w, act); s1.w += dz; s2.w += dz * (v.w - mu.w) * is.w;
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < wm.rpi; ++l) {
      float4 a = red[0][l * wm.tpr + c4], e = red[1][l * wm.tpr + c4];
      s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
      s2.x += e.x; s2.y += e.y; s2.z += e.z; s2.w += e.w;
    }
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 0) * C + c4 * 4) = s1;
    *reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * C + c4 * 4) = s2;
  }
}

// bn_bwd_finalize_kernel with the count N taken from lens (N = 0: the sums are 0 and so are the means)
__global__ __launch_bounds__(1024) void bn_bwd_finalize_lens_kernel(const float* __restrict__ partial,
                                                                     const int* __restrict__ lens, int B,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                     float* __restrict__ coef, int C, LensMap lm) {
  __shared__ double red[16][FIN_CH];
  const int c = blockIdx.x * FIN_CH + (threadIdx.x & 15);
  const long long count = lens_count(lens, B, lm);
  double a, e;
  fin_parts(partial, B * lm.ppu, C, c, [&](int, float u, float v, double& x, double& y) { x += (double)u; y += (double)v; }, a, e);
  const double s1 = fin_sum(a, red), s2 = fin_sum(e, red);
  if (threadIdx.x >= FIN_CH || c >= C) return;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  const double n = count > 0 ? (double)count : 1.0;
  coef[c] = (float)(s1 / n);
  coef[C + c] = (float)(s2 / n);
}

// The training-mode backward of FEW valid rows in fp64, one thread per channel: bn_bwd_small_kernel (see there for why)
// over the valid rows.  Returns at once when there are more than BN_SMALL_ROWS of them, or none.
__global__ __launch_bounds__(64) void bn_bwd_small_lens_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                                const float* __restrict__ stats,
                                                                const int* __restrict__ lens, int B,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ dy, int C, int act, LensMap lm) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const long long M = lens_count(lens, B, lm);
  if (M > BN_SMALL_ROWS || M == 0) return;
  const float sc = stats[c], sh = stats[C + c];
  const double eps = (double)stats[4 * C + c];
  auto rows = [&](auto&& f) {
    for (int b = 0; b < B; ++b) {
      const int nv = lens_valid_rows(lens, b, lm);
      for (int r = 0; r < nv; ++r) f(((long long)b * lm.HW + r) * C + c);
    }
  };
  double mu = 0.0, m2 = 0.0;
  rows([&](long long idx) { mu += (double)y[idx]; });
  mu /= (double)M;
  rows([&](long long idx) {
    const double d = (double)y[idx] - mu;
    m2 += d * d;
  });
  const double invstd = 1.0 / sqrt(m2 / (double)M + eps);
  double s1 = 0.0, s2 = 0.0;
  rows([&](long long idx) {
    const double dz = (double)dz_of(dout[idx], y[idx], sc, sh, act);
    s1 += dz;
    s2 += dz * (((double)y[idx] - mu) * invstd);
  });
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  const double k1 = s1 / (double)M, k2 = s2 / (double)M;
  rows([&](long long idx) {
    const double dz = (double)dz_of(dout[idx], y[idx], sc, sh, act);
    dy[idx] = (float)((double)sc * (dz - k1 - ((double)y[idx] - mu) * invstd * k2));
  });
}

// dy = scale * (dz - mean(dz) - xhat * mean(dz * xhat)) on the valid rows, 0 on the others (whose dout and y are never
// read).  With N <= BN_SMALL_ROWS valid rows the valid rows are bn_bwd_small_lens_kernel's and are left alone here.
__global__ __launch_bounds__(256) void bn_bwd_apply_lens_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ coef,
                                                                 const int* __restrict__ lens, int B,
                                                                 float* __restrict__ dy, long long n4, int C, int act,
                                                                 LensMap lm) {
  const int c4n = C >> 2;
  const long long count = lens_count(lens, B, lm);
  const bool small = count > 0 && count <= BN_SMALL_ROWS;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / c4n;
    const int c4 = (int)(i - row * c4n);
    const int b = (int)(row / lm.HW);
    if ((int)(row - (long long)b * lm.HW) >= lens_valid_rows(lens, b, lm)) {
      reinterpret_cast<float4*>(dy)[i] = make_float4(0, 0, 0, 0);
      continue;
    }
    if (small) continue;
    const float4 sc = reinterpret_cast<const float4*>(stats)[c4], sh = reinterpret_cast<const float4*>(stats + C)[c4];
    const float4 v = reinterpret_cast<const float4*>(y)[i], d = reinterpret_cast<const float4*>(dout)[i];
    const float4 mu = reinterpret_cast<const float4*>(stats + 2 * C)[c4], is = reinterpret_cast<const float4*>(stats + 3 * C)[c4];
    const float4 k1 = reinterpret_cast<const float4*>(coef)[c4], k2 = reinterpret_cast<const float4*>(coef + C)[c4];
    float4 dz;
    dz.x = dz_of(d.x, v.x, sc.x, sh.x, act) - k1.x - (v.x - mu.x) * is.x * k2.x;
    dz.y = dz_of(d.y, v.y, sc.y, sh.y, act) - k1.y - (v.y - mu.y) * is.y * k2.y;
    dz.z = dz_of(d.z, v.z, sc.z, sh.z, act) - k1.z - (v.z - mu.z) * is.z * k2.z;
    dz.w = dz_of(d.w, v.w, sc.w, sh.w, act) - k1.w - (v.w - mu.w) * is.w * k2.w;
    reinterpret_cast<float4*>(dy)[i] = make_float4(sc.x * dz.x, sc.y * dz.y, sc.z * dz.z, sc.w * dz.w);
  }
}

bool wide_ok(int C, WideMap& wm) {
  if ((C % 4) || C > 1024) return false;
  wm.tpr = C / 4;
  wm.rpi = 256 / wm.tpr;
  return true;
}

// the stripes of the length-aware kernels: as tall as colstats takes them for the whole [B * H * W][C] matrix
bool lens_map(int B, int H, int W, LensMap& lm) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > 0x7fffffffLL) return false;
  lm.H = H;
  lm.W = W;
  lm.HW = H * W;
  lm.pr = cs_rows(B * lm.HW);
  lm.ppu = (lm.HW + lm.pr - 1) / lm.pr;
  return true;
}

}  // namespace

extern "C" int fs2hip_colstats_parts(int M) { return M > 0 ? (M + cs_rows(M) - 1) / cs_rows(M) : 0; }
extern "C" int fs2hip_colstats_part_rows(int M) { return M > 0 ? cs_rows(M) : 0; }

extern "C" int fs2hip_colstats_b(const void* y, int M, int C, float* partial, int in_bf16, void* stream);
extern "C" int fs2hip_colstats(const float* y, int M, int C, float* partial, void* stream) {
  return fs2hip_colstats_b(y, M, C, partial, 0, stream);
}

// in_bf16: y is a bf16 tensor
extern "C" int fs2hip_colstats_b(const void* y, int M, int C, float* partial, int in_bf16, void* stream) {
  WideMap wm;
  if (M <= 0 || C <= 0 || !wide_ok(C, wm) || ((uintptr_t)y % (in_bf16 ? 8 : 16)) || ((uintptr_t)partial % 16)) return FS2HIP_EINVAL;
  const dim3 grid(fs2hip_colstats_parts(M));
  return fs2_pick_bool(in_bf16 != 0, [&](auto ib) {
    colstats_wide_kernel<ib><<<grid, dim3(256), 0, (hipStream_t)stream>>>(y, M, C, partial, wm);
    return fs2_launched();
  });
}

extern "C" int fs2hip_bn_finalize(const float* partial, int nparts, long long count, int part_rows, int group_rows,
                                  const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  float momentum, float eps, int training, float* stats, int C, void* stream) {
  if (C <= 0 || (training && (nparts <= 0 || count <= 0 || !partial)) || (!training && (!running_mean || !running_var)))
    return FS2HIP_EINVAL;
  if (training) {  // the parts must tile `count` rows exactly: groups of group_rows rows in stripes of part_rows
    if (part_rows <= 0 || group_rows <= 0 || count % group_rows) return FS2HIP_EINVAL;
    const long long ppg = (group_rows + part_rows - 1) / part_rows;
    if (ppg * (count / group_rows) != nparts) return FS2HIP_EINVAL;
  }
  bn_finalize_kernel<<<dim3((C + FIN_CH - 1) / FIN_CH), dim3(1024), 0, (hipStream_t)stream>>>(
      partial, nparts, count, part_rows, group_rows, gamma, beta, running_mean, running_var, momentum, eps, training,
      stats, C);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_bn_act_fwd_b(const void* y, const float* stats, float* out, void* out_bf16, int M, int C, int act,
                                   float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                   int in_bf16, void* stream);
extern "C" int fs2hip_bn_act_fwd(const float* y, const float* stats, float* out, int M, int C, int act, float drop_p,
                                 unsigned long long drop_seed, const unsigned long long* drop_step, void* stream) {
  return fs2hip_bn_act_fwd_b(y, stats, out, nullptr, M, C, act, drop_p, drop_seed, drop_step, 0, stream);
}

// in_bf16: y is a bf16 tensor
extern "C" int fs2hip_bn_act_fwd_b(const void* y, const float* stats, float* out, void* out_bf16, int M, int C, int act,
                                   float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                   int in_bf16, void* stream) {
  if (M <= 0 || C <= 0 || (C % 4) || ((uintptr_t)y % (in_bf16 ? 8 : 16)) || ((uintptr_t)out % 16) ||
      ((uintptr_t)stats % 16) || ((uintptr_t)out_bf16 % 8) || (!out && !out_bf16))
    return FS2HIP_EINVAL;
  const long long n4 = (long long)M * C / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const Fs2Drop drop = fs2_make_drop(drop_p, drop_seed, drop_step);
  return fs2_pick_bool(in_bf16 != 0, [&](auto ib) {
    bn_act_fwd_kernel<ib><<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(y, stats, out, out_bf16, n4, C, act, drop);
    return fs2_launched();
  });
}

// partial: [fs2hip_colstats_parts(M)][2][C]; coef: [2][C] scratch (16-byte aligned)
extern "C" int fs2hip_bn_act_bwd_b(const void* dout, const void* y, const float* stats, float* partial, float* coef,
                                   float* dgamma, float* dbeta, float* dy, void* dy_bf16, int M, int C, int act,
                                   float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                   int training, int in_bf16, void* stream);
extern "C" int fs2hip_bn_act_bwd(const float* dout, const float* y, const float* stats, float* partial, float* coef,
                                 float* dgamma, float* dbeta, float* dy, int M, int C, int act, float drop_p,
                                 unsigned long long drop_seed, const unsigned long long* drop_step, int training,
                                 void* stream) {
  return fs2hip_bn_act_bwd_b(dout, y, stats, partial, coef, dgamma, dbeta, dy, nullptr, M, C, act, drop_p, drop_seed,
                             drop_step, training, 0, stream);
}

// in_bf16 bit 0: y is a bf16 tensor; bit 1: dout is
extern "C" int fs2hip_bn_act_bwd_b(const void* dout, const void* y, const float* stats, float* partial, float* coef,
                                   float* dgamma, float* dbeta, float* dy, void* dy_bf16, int M, int C, int act,
                                   float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                   int training, int in_bf16, void* stream) {
  if (((uintptr_t)dy_bf16 % 8) || (!dy && !dy_bf16)) return FS2HIP_EINVAL;
  WideMap wm;
  if (M <= 0 || C <= 0 || !wide_ok(C, wm)) return FS2HIP_EINVAL;
  if (((uintptr_t)dout % ((in_bf16 & 2) ? 8 : 16)) || ((uintptr_t)y % ((in_bf16 & 1) ? 8 : 16)) || ((uintptr_t)stats % 16) || ((uintptr_t)partial % 16) ||
      ((uintptr_t)coef % 16) || ((uintptr_t)dy % 16))
    return FS2HIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const Fs2Drop drop = fs2_make_drop(drop_p, drop_seed, drop_step);
  if (training && M <= BN_SMALL_ROWS && !(in_bf16 & 3) && dy && !dy_bf16) {
    bn_bwd_small_kernel<<<dim3((C + 63) / 64), dim3(64), 0, s>>>((const float*)dout, (const float*)y, stats, dgamma, dbeta,
                                                              dy, M, C, act, drop);
    FS2_LAUNCH_CHECK();
    return 0;
  }
  const int nparts = fs2hip_colstats_parts(M);
  // IB: y is bf16; DB: dout is
  return fs2_pick_bool(in_bf16 & 1, [&](auto ib) {
    return fs2_pick_bool(in_bf16 & 2, [&](auto db) {
      bn_bwd_reduce_kernel<ib, db><<<dim3(nparts), dim3(256), 0, s>>>(dout, y, stats, M, C, act, drop, partial, wm);
      FS2_LAUNCH_CHECK();
      bn_bwd_finalize_kernel<<<dim3((C + FIN_CH - 1) / FIN_CH), dim3(1024), 0, s>>>(partial, nparts, (long long)M, dgamma, dbeta, coef, C);
      FS2_LAUNCH_CHECK();
      const long long n4 = (long long)M * C / 4;
      long long blocks = (n4 + 255) / 256;
      if (blocks > 8192) blocks = 8192;
      bn_bwd_apply_kernel<ib, db><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(dout, y, stats, coef, dy, dy_bf16, n4, C, act, drop, training);
      return fs2_launched();
    });
  });
}

// ---- BatchNorm over the valid positions only (the kernels above; include/fs2hip.h) ----
extern "C" int fs2hip_bn_lens_parts(int B, int H, int W) {
  LensMap lm;
  return lens_map(B, H, W, lm) ? B * lm.ppu : 0;
}

// partial: [fs2hip_bn_lens_parts(B, H, W)][2][C] scratch (16-byte aligned)
extern "C" int fs2hip_bn_stats_lens(const float* y, const int* lens, float* partial, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, float* stats,
                                    int B, int H, int W, int C, void* stream) {
  WideMap wm;
  LensMap lm;
  if (!y || !lens || !partial || !gamma || !beta || !stats || !lens_map(B, H, W, lm) || C <= 0 || !wide_ok(C, wm) ||
      (!running_mean != !running_var) || ((uintptr_t)y % 16) || ((uintptr_t)partial % 16))
    return FS2HIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  colstats_lens_kernel<<<dim3(B * lm.ppu), dim3(256), 0, s>>>(y, lens, C, partial, wm, lm);
  FS2_LAUNCH_CHECK();
  bn_finalize_lens_kernel<<<dim3((C + FIN_CH - 1) / FIN_CH), dim3(1024), 0, s>>>(partial, lens, B, gamma, beta, running_mean,
                                                                              running_var, momentum, eps, stats, C, lm);
  FS2_LAUNCH_CHECK();
  return 0;
}

// partial as above; coef: [2][C] scratch (16-byte aligned)
extern "C" int fs2hip_bn_act_bwd_lens(const float* dout, const float* y, const float* stats, const int* lens, float* partial,
                                      float* coef, float* dgamma, float* dbeta, float* dy, int B, int H, int W, int C,
                                      int act, void* stream) {
  WideMap wm;
  LensMap lm;
  if (!dout || !y || !stats || !lens || !partial || !coef || !dgamma || !dbeta || !dy || !lens_map(B, H, W, lm) || C <= 0 ||
      !wide_ok(C, wm) || ((uintptr_t)dout % 16) || ((uintptr_t)y % 16) || ((uintptr_t)stats % 16) ||
      ((uintptr_t)partial % 16) || ((uintptr_t)coef % 16) || ((uintptr_t)dy % 16))
    return FS2HIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  bn_bwd_reduce_lens_kernel<<<dim3(B * lm.ppu), dim3(256), 0, s>>>(dout, y, stats, lens, C, act, partial, wm, lm);
  FS2_LAUNCH_CHECK();
  bn_bwd_finalize_lens_kernel<<<dim3((C + FIN_CH - 1) / FIN_CH), dim3(1024), 0, s>>>(partial, lens, B, dgamma, dbeta, coef, C, lm);
  FS2_LAUNCH_CHECK();
  const long long n4 = (long long)B * lm.HW * C / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  bn_bwd_apply_lens_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(dout, y, stats, coef, lens, B, dy, n4, C, act, lm);
  FS2_LAUNCH_CHECK();
  bn_bwd_small_lens_kernel<<<dim3((C + 63) / 64), dim3(64), 0, s>>>(dout, y, stats, lens, B, dgamma, dbeta, dy, C, act, lm);
  FS2_LAUNCH_CHECK();
  return 0;
}
