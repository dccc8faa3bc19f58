// Depthwise Conv1d over time on the dense (B, T, C) layout, optionally fused with the GLU that
// precedes it and with the per-channel sum / sum-of-squares BatchNorm needs after it.
// Replaces: torchaudio Conformer conv module's GLU + depthwise Conv1d(k) (+ the statistics pass of
// BatchNorm1d) (call sites fs2/model.py:193, :241) and the depthwise half of
// DepthwiseSeparableConv1d (fs2/blocks.py:8-13).  HBM-bound: each input element is read once
// (+ halo from L2), lanes run along channels so every row access is a contiguous 256-byte line.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int RUN = 16;  // consecutive time steps per thread

// element loads / stores of a tensor that is fp32 (XB = false) or bf16 (XB = true) in memory
__device__ __forceinline__ unsigned short dw_bf16(float v) {
  return __builtin_bit_cast(unsigned short, (__bf16)v);  // round to nearest even, NaN stays NaN
}
template <bool XB>
__device__ __forceinline__ float dw_ld(const void* p, long long i) {
  if constexpr (XB) return __builtin_bit_cast(float, (unsigned)((const unsigned short*)p)[i] << 16);
  else return ((const float*)p)[i];
}

// x: [B*T][ldx]; value at column c, gate (GLU) at column C + c.  XB: x and y are bf16 tensors (precision "bf16-mixed"
// with bf16 activation storage: what autocast hands a convolution); the statistics are those of the ROUNDED outputs,
// which is what BatchNorm then normalises.
template <int K, bool GLU, bool STATS, bool XB = false, bool YB = XB>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const void* __restrict__ x, int ldx,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          void* __restrict__ y, float* __restrict__ partial, int B,
                                                          int T, int C) {
  constexpr int PAD = (K - 1) / 2, WIN = RUN + K - 1;
  __shared__ float red[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int t0 = blockIdx.y * (4 * RUN) + wave * RUN;
  const int b = blockIdx.z;
  const bool cok = c < C;
  float wk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wk[k] = cok ? w[k * C + c] : 0.f;
  const float bs = (cok && bias) ? bias[c] : 0.f;
  float a[WIN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) {
    int t = t0 - PAD + i;
    float v = 0.f;
    if (cok && t >= 0 && t < T) {
      const long long row = ((long long)b * T + t) * ldx;
      v = dw_ld<XB>(x, row + c);
      if (GLU) v *= fs2_sigmoid(dw_ld<XB>(x, row + C + c));
    }
    a[i] = v;
  }
  // BatchNorm statistics of this thread's run as (n, mean, M2): sums of (y - pivot), pivot = the run's first output
  // (bn.hip explains why not sum / sum of squares)
  float s1 = 0.f, s2 = 0.f, pivot = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    if (cok && t < T) {
      float acc = bs;
#pragma unroll
      for (int k = 0; k < K; ++k) acc = fmaf(wk[k], a[o + k], acc);
      if constexpr (YB) {
        const unsigned short r = dw_bf16(acc);
        ((unsigned short*)y)[((long long)b * T + t) * C + c] = r;
        acc = __builtin_bit_cast(float, (unsigned)r << 16);
      } else {
        ((float*)y)[((long long)b * T + t) * C + c] = acc;
      }
      if (STATS) {
        if (o == 0) pivot = acc;
        const float d = acc - pivot;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  if (STATS) {
    const int nw = max(0, min(RUN, T - t0));  // rows of this wavefront's run (uniform over its lanes)
    const float inv = nw > 0 ? 1.f / (float)nw : 0.f;
    red[wave][0][lane] = pivot + s1 * inv;
    red[wave][1][lane] = fmaxf(s2 - s1 * s1 * inv, 0.f);
    __syncthreads();
    if (wave == 0 && cok) {
      float n = 0.f, mean = 0.f, m2 = 0.f;  // Chan merge of the four runs
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float nr = (float)max(0, min(RUN, T - (t0 + w * RUN)));
        if (nr > 0.f) {
          const float delta = red[w][0][lane] - mean, nt = n + nr;
          mean += delta * (nr / nt);
          m2 += red[w][1][lane] + delta * delta * (n * nr / nt);
          n = nt;
        }
      }
      long long blk = (long long)b * gridDim.y + blockIdx.y;
      partial[(blk * 2 + 0) * C + c] = mean;
      partial[(blk * 2 + 1) * C + c] = m2;
    }
  }
}

// dy [B*T][C]; x as in the forward; dx has the layout of x.  partial [blk][K+1][C]: dw taps, dbias.
// DXB: dx is written as bf16 (the operand of the pointwise convolution's data- and weight-gradient GEMMs)
// XB: dy and x are bf16 tensors
template <int K, bool GLU, bool DXB = false, bool XB = false>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                          int ldx, const float* __restrict__ w, void* __restrict__ dxv,
                                                          float* __restrict__ partial, int B, int T, int C) {
  constexpr int PAD = (K - 1) / 2, WIN = RUN + K - 1;
  __shared__ float red[4][K + 1][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int t0 = blockIdx.y * (4 * RUN) + wave * RUN;
  const int b = blockIdx.z;
  const bool cok = c < C;
  float wk[K], dwk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wk[k] = cok ? w[k * C + c] : 0.f;
    dwk[k] = 0.f;
  }
  float a[WIN], g[WIN], vc[RUN], sc[RUN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) {
    int t = t0 - PAD + i;
    float v = 0.f, d = 0.f, vv = 0.f, sg = 0.f;
    if (cok && t >= 0 && t < T) {
      const long long row = ((long long)b * T + t) * ldx;
      vv = dw_ld<XB>(x, row + c);
      v = vv;
      if (GLU) {
        sg = fs2_sigmoid(dw_ld<XB>(x, row + C + c));
        v = vv * sg;
      }
      d = dw_ld<XB>(dy, ((long long)b * T + t) * C + c);
    }
    a[i] = v;
    g[i] = d;
    if (i >= PAD && i < PAD + RUN) {
      vc[i - PAD] = vv;
      sc[i - PAD] = sg;
    }
  }
  float db = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    // da[t] = sum_k w[k] * dy[t - k + PAD]
    float da = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) da = fmaf(wk[k], g[o + (K - 1 - k)], da);
    const float gy = g[o + PAD];
    db += gy;
#pragma unroll
    for (int k = 0; k < K; ++k) dwk[k] = fmaf(gy, a[o + k], dwk[k]);
    if (cok && t < T) {
      if constexpr (DXB) {
        unsigned short* row = (unsigned short*)dxv + ((long long)b * T + t) * ldx;
        if (GLU) {
          row[c] = dw_bf16(da * sc[o]);
          row[C + c] = dw_bf16(da * vc[o] * sc[o] * (1.f - sc[o]));
        } else {
          row[c] = dw_bf16(da);
        }
      } else {
        float* row = (float*)dxv + ((long long)b * T + t) * ldx;
        if (GLU) {
          row[c] = da * sc[o];
          row[C + c] = da * vc[o] * sc[o] * (1.f - sc[o]);
        } else {
          row[c] = da;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) red[wave][k][lane] = dwk[k];
  red[wave][K][lane] = db;
  __syncthreads();
  if (wave == 0 && cok) {
    long long blk = (long long)b * gridDim.y + blockIdx.y;
#pragma unroll
    for (int k = 0; k <= K; ++k)
      partial[(blk * (K + 1) + k) * C + c] = red[0][k][lane] + red[1][k][lane] + red[2][k][lane] + red[3][k][lane];
  }
}

// ---- tiled GLU forms ------------------------------------------------------------------------------------------------
// The kernels above give every thread its own window of rows: one 2- or 4-byte element per lane and load instruction,
// and the GLU (a sigmoid) of the K - 1 halo rows is recomputed by each of the four wavefronts of a workgroup.  Measured
// at the decoder's shape they run at 2 TB/s whether the tensors are fp32 or bf16 -- bound by load instructions, not
// bytes.  Here a workgroup first brings its (4 RUN + K - 1) rows x 64 channels through LDS: 16 bytes per lane and load
// (eight channels of one row), the GLU applied once per element, a = value * sigmoid(gate) kept as fp32; then every
// thread runs the same per-channel loop as above with its window read from LDS.  Same arithmetic in the same order:
// the results are the bits of the kernels above.  Needs C % 64 == 0 and ldx % 8 == 0.
template <bool XB>
__device__ __forceinline__ void dw_ld8(const void* p, long long e, float (&v)[8]) {
  if constexpr (XB) {
    const uint4 u = *reinterpret_cast<const uint4*>((const unsigned short*)p + e);
    const unsigned q[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __builtin_bit_cast(float, q[j] << 16);
      v[2 * j + 1] = __builtin_bit_cast(float, q[j] & 0xffff0000u);
    }
  } else {
    const float4 a = *reinterpret_cast<const float4*>((const float*)p + e);
    const float4 b = *reinterpret_cast<const float4*>((const float*)p + e + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
__device__ __forceinline__ void dw_st8(float* dst, const float (&v)[8]) {
  *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// eight consecutive channels of a staged result row -> global memory, as fp32 (32 bytes) or bf16 (16 bytes)
template <bool OB>
__device__ __forceinline__ void dw_st8_global(void* dst, long long e, const float* src) {
  const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
  if constexpr (OB) {
    uint4 u;
    u.x = (unsigned)dw_bf16(a.x) | ((unsigned)dw_bf16(a.y) << 16);
    u.y = (unsigned)dw_bf16(a.z) | ((unsigned)dw_bf16(a.w) << 16);
    u.z = (unsigned)dw_bf16(b.x) | ((unsigned)dw_bf16(b.y) << 16);
    u.w = (unsigned)dw_bf16(b.z) | ((unsigned)dw_bf16(b.w) << 16);
    *reinterpret_cast<uint4*>((unsigned short*)dst + e) = u;
  } else {
    *reinterpret_cast<float4*>((float*)dst + e) = a;
    *reinterpret_cast<float4*>((float*)dst + e + 4) = b;
  }
}
// the same from registers
template <bool OB>
__device__ __forceinline__ void dw_st8_global_r(void* dst, long long e, const float (&v)[8]) {
  if constexpr (OB) {
    uint4 u;
    u.x = (unsigned)dw_bf16(v[0]) | ((unsigned)dw_bf16(v[1]) << 16);
    u.y = (unsigned)dw_bf16(v[2]) | ((unsigned)dw_bf16(v[3]) << 16);
    u.z = (unsigned)dw_bf16(v[4]) | ((unsigned)dw_bf16(v[5]) << 16);
    u.w = (unsigned)dw_bf16(v[6]) | ((unsigned)dw_bf16(v[7]) << 16);
    *reinterpret_cast<uint4*>((unsigned short*)dst + e) = u;
  } else {
    *reinterpret_cast<float4*>((float*)dst + e) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>((float*)dst + e + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

template <int K, bool STATS, bool XB>
__global__ __launch_bounds__(256) void dwconv_glu_fwd_tile_kernel(const void* __restrict__ x, int ldx,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ bias, void* __restrict__ y,
                                                                   float* __restrict__ partial, int B, int T, int C) {
  constexpr int PAD = (K - 1) / 2, WIN = RUN + K - 1, TT = 4 * RUN, ROWS = TT + K - 1;
  __shared__ __attribute__((aligned(16))) float as[ROWS][64];
  __shared__ __attribute__((aligned(16))) float ys[TT][64];  // results, staged for whole-row stores
  __shared__ float red[4][2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64, c = c0 + lane;
  const int tbase = blockIdx.y * TT, t0 = tbase + wave * RUN;
  const int b = blockIdx.z;
  {
    const int sub = tid & 7;
#pragma unroll
    for (int r = tid >> 3; r < ROWS; r += 32) {
      const int t = tbase - PAD + r;
      float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < T) {
        const long long row = ((long long)b * T + t) * ldx + c0 + 8 * sub;
        float v8[8], g8[8];
        dw_ld8<XB>(x, row, v8);
        dw_ld8<XB>(x, row + C, g8);
#pragma unroll
        for (int j = 0; j < 8; ++j) a8[j] = v8[j] * fs2_sigmoid(g8[j]);
      }
      dw_st8(&as[r][8 * sub], a8);
    }
  }
  float wk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wk[k] = w[k * C + c];
  const float bs = bias ? bias[c] : 0.f;
  __syncthreads();
  float a[WIN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) a[i] = as[wave * RUN + i][lane];
  float s1 = 0.f, s2 = 0.f, pivot = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    if (t < T) {
      float acc = bs;
#pragma unroll
      for (int k = 0; k < K; ++k) acc = fmaf(wk[k], a[o + k], acc);
      if constexpr (XB) acc = __builtin_bit_cast(float, (unsigned)dw_bf16(acc) << 16);  // (the stored value)
      ys[wave * RUN + o][lane] = acc;
      if (STATS) {
        if (o == 0) pivot = acc;
        const float d = acc - pivot;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  if (STATS) {
    const int nw = max(0, min(RUN, T - t0));
    const float inv = nw > 0 ? 1.f / (float)nw : 0.f;
    red[wave][0][lane] = pivot + s1 * inv;
    red[wave][1][lane] = fmaxf(s2 - s1 * s1 * inv, 0.f);
  }
  __syncthreads();
  {
    const int sub = tid & 7;
#pragma unroll
    for (int r = tid >> 3; r < TT; r += 32) {
      const int t = tbase + r;
      if (t < T) dw_st8_global<XB>(y, ((long long)b * T + t) * C + c0 + 8 * sub, &ys[r][8 * sub]);
    }
  }
  if (STATS) {
    if (wave == 0) {
      float n = 0.f, mean = 0.f, m2 = 0.f;  // Chan merge of the four runs (as above)
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4) {
        const float nr = (float)max(0, min(RUN, T - (tbase + w4 * RUN)));
        if (nr > 0.f) {
          const float delta = red[w4][0][lane] - mean, nt = n + nr;
          mean += delta * (nr / nt);
          m2 += red[w4][1][lane] + delta * delta * (n * nr / nt);
          n = nt;
        }
      }
      long long blk = (long long)b * gridDim.y + blockIdx.y;
      partial[(blk * 2 + 0) * C + c] = mean;
      partial[(blk * 2 + 1) * C + c] = m2;
    }
  }
}

template <int K, bool XB>
__global__ __launch_bounds__(256) void dwconv_glu_bwd_tile_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                                   int ldx, const float* __restrict__ w,
                                                                   void* __restrict__ dxv, float* __restrict__ partial,
                                                                   int B, int T, int C, int dx_b) {
  constexpr int PAD = (K - 1) / 2, WIN = RUN + K - 1, TT = 4 * RUN, ROWS = TT + K - 1;
  __shared__ __attribute__((aligned(16))) float as[ROWS][64];  // value * sigmoid(gate)
  __shared__ __attribute__((aligned(16))) float gs[ROWS][64];  // dy
  __shared__ __attribute__((aligned(16))) float vs[TT][64];    // value, centre rows
  __shared__ __attribute__((aligned(16))) float ss[TT][64];    // sigmoid(gate), centre rows
  __shared__ float red[4][K + 1][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64, c = c0 + lane;
  const int tbase = blockIdx.y * TT, t0 = tbase + wave * RUN;
  const int b = blockIdx.z;
  {
    const int sub = tid & 7;
#pragma unroll
    for (int r = tid >> 3; r < ROWS; r += 32) {
      const int t = tbase - PAD + r;
      float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float v8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < T) {
        const long long row = ((long long)b * T + t) * ldx + c0 + 8 * sub;
        float g8[8];
        dw_ld8<XB>(x, row, v8);
        dw_ld8<XB>(x, row + C, g8);
        dw_ld8<XB>(dy, ((long long)b * T + t) * C + c0 + 8 * sub, d8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s8[j] = fs2_sigmoid(g8[j]);
          a8[j] = v8[j] * s8[j];
        }
      }
      dw_st8(&as[r][8 * sub], a8);
      dw_st8(&gs[r][8 * sub], d8);
      if (r >= PAD && r < PAD + TT) {
        dw_st8(&vs[r - PAD][8 * sub], v8);
        dw_st8(&ss[r - PAD][8 * sub], s8);
      }
    }
  }
  float wk[K], dwk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wk[k] = w[k * C + c];
    dwk[k] = 0.f;
  }
  __syncthreads();
  float a[WIN], g[WIN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) {
    a[i] = as[wave * RUN + i][lane];
    g[i] = gs[wave * RUN + i][lane];
  }
  float db = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    float da = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) da = fmaf(wk[k], g[o + (K - 1 - k)], da);
    const float gy = g[o + PAD];
    db += gy;
#pragma unroll
    for (int k = 0; k < K; ++k) dwk[k] = fmaf(gy, a[o + k], dwk[k]);
    {  // the two halves of dx replace the value / sigmoid this thread has just read (its own rows, its own column)
      const float vc = vs[wave * RUN + o][lane], sc = ss[wave * RUN + o][lane];
      vs[wave * RUN + o][lane] = da * sc;
      ss[wave * RUN + o][lane] = da * vc * sc * (1.f - sc);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) red[wave][k][lane] = dwk[k];
  red[wave][K][lane] = db;
  __syncthreads();
  {
    const int sub = tid & 7;
#pragma unroll
    for (int r = tid >> 3; r < TT; r += 32) {
      const int t = tbase + r;
      if (t < T) {
        const long long row = ((long long)b * T + t) * ldx + c0 + 8 * sub;
        if (dx_b) {
          dw_st8_global<true>(dxv, row, &vs[r][8 * sub]);
          dw_st8_global<true>(dxv, row + C, &ss[r][8 * sub]);
        } else {
          dw_st8_global<false>(dxv, row, &vs[r][8 * sub]);
          dw_st8_global<false>(dxv, row + C, &ss[r][8 * sub]);
        }
      }
    }
  }
  if (wave == 0) {
    long long blk = (long long)b * gridDim.y + blockIdx.y;
#pragma unroll
    for (int k = 0; k <= K; ++k)
      partial[(blk * (K + 1) + k) * C + c] = red[0][k][lane] + red[1][k][lane] + red[2][k][lane] + red[3][k][lane];
  }
}

// ---- any odd width up to KMAX: run-time K ---------------------------------------------------------------------------
// The kernels above hold the taps and each thread's window in registers sized by K (more than 300 VGPRs in the
// backward pass at K = 63).  Here the workgroup's window -- (4 RUN + K - 1) rows x 64 channels, fp32 -- sits in LDS, the
// taps are read from global memory (256 bytes per tap and wavefront, L1-resident), and every thread walks the taps at
// run time in chunks of KC: per chunk KC taps and a (RUN + KC - 1)-row slice of its window in registers.  The loops
// over outputs and taps are only interchanged: every output, data gradient and tap gradient takes its terms in the
// order of the kernels above, so for the six built widths the results are their bits.  The tap gradients are reduced
// across the four wavefronts one chunk at a time, through KC rows of LDS.  LDS (dynamic, all of it): 256 (4 RUN + K - 1)
// bytes (+ 2 KB of statistics) forward, twice that backward: at most 63 KB, at K = 63.
constexpr int KMAX = 63, KC = 16;

__host__ __device__ constexpr int dwg_rows(int K) { return 4 * RUN + K - 1; }

// acc[o] = bias, then acc[o] = fmaf(w[k], a[o + k], acc[o]) for k ascending.  win: the thread's window (row stride 64).
__device__ __forceinline__ void dwg_conv(const float* win, const float* __restrict__ w, int C, int c, bool cok, int K,
                                         float bs, float (&acc)[RUN]) {
#pragma unroll
  for (int o = 0; o < RUN; ++o) acc[o] = bs;
  for (int kc = 0; kc < K; kc += KC) {
    float wk[KC], aw[RUN + KC - 1];
#pragma unroll
    for (int j = 0; j < KC; ++j) wk[j] = (cok && kc + j < K) ? w[(kc + j) * C + c] : 0.f;
#pragma unroll
    for (int i = 0; i < RUN + KC - 1; ++i) aw[i] = win[min(kc + i, K + RUN - 2) * 64];
#pragma unroll
    for (int j = 0; j < KC; ++j)
      if (kc + j < K) {
#pragma unroll
        for (int o = 0; o < RUN; ++o) acc[o] = fmaf(wk[j], aw[o + j], acc[o]);
      }
  }
}

// da[o] = 0, then da[o] = fmaf(w[k], g[o + K - 1 - k], da[o]) for k ascending.  gwin: the thread's window of dy.
__device__ __forceinline__ void dwg_dgrad(const float* gwin, const float* __restrict__ w, int C, int c, bool cok, int K,
                                          float (&da)[RUN]) {
#pragma unroll
  for (int o = 0; o < RUN; ++o) da[o] = 0.f;
  for (int kc = 0; kc < K; kc += KC) {
    const int base = K - KC - kc;  // gw[i] = g[base + i]; rows below 0 are never used
    float wk[KC], gw[RUN + KC - 1];
#pragma unroll
    for (int j = 0; j < KC; ++j) wk[j] = (cok && kc + j < K) ? w[(kc + j) * C + c] : 0.f;
#pragma unroll
    for (int i = 0; i < RUN + KC - 1; ++i) gw[i] = gwin[max(base + i, 0) * 64];
#pragma unroll
    for (int j = 0; j < KC; ++j)
      if (kc + j < K) {
#pragma unroll
        for (int o = 0; o < RUN; ++o) da[o] = fmaf(wk[j], gw[o + KC - 1 - j], da[o]);
      }
  }
}

// Tap gradients (dw[k]: fmaf(gy[o], a[o + k], .) over o ascending) and dbias (gy summed over o), each summed over the
// four wavefronts (0 + 1 + 2 + 3, as above) into partial [blk][K + 1][C].  red: 4 KC x 64 floats of LDS that nothing
// else uses meanwhile; win: the thread's window of a.  Called by the whole workgroup; every read of win is over when
// it returns.
__device__ __forceinline__ void dwg_wgrad(const float* win, const float (&gy)[RUN], float* red, float* __restrict__ partial,
                                          long long blk, int C, int c, bool cok, int K, int lane, int wave) {
  for (int kc = 0; kc < K; kc += KC) {
    float aw[RUN + KC - 1];
#pragma unroll
    for (int i = 0; i < RUN + KC - 1; ++i) aw[i] = win[min(kc + i, K + RUN - 2) * 64];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      float dwk = 0.f;
      if (kc + j < K) {
#pragma unroll
        for (int o = 0; o < RUN; ++o) dwk = fmaf(gy[o], aw[o + j], dwk);
      }
      red[(wave * KC + j) * 64 + lane] = dwk;
    }
    __syncthreads();
    for (int j = wave; j < KC; j += 4)
      if (cok && kc + j < K)
        partial[(blk * (K + 1) + kc + j) * C + c] = red[(0 * KC + j) * 64 + lane] + red[(1 * KC + j) * 64 + lane] +
                                                    red[(2 * KC + j) * 64 + lane] + red[(3 * KC + j) * 64 + lane];
    __syncthreads();
  }
  float db = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) db += gy[o];
  red[wave * 64 + lane] = db;
  __syncthreads();
  if (wave == 0 && cok) partial[(blk * (K + 1) + K) * C + c] = red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
}

// BatchNorm statistics of the workgroup's four runs -> partial [blk][2][C], as in dwconv_fwd_kernel
__device__ __forceinline__ void dwg_stats(float (*red)[2][64], float* __restrict__ partial, float s1, float s2,
                                          float pivot, int T, int tbase, int t0, int C, int c, bool cok, int lane,
                                          int wave) {
  const int nw = max(0, min(RUN, T - t0));
  const float inv = nw > 0 ? 1.f / (float)nw : 0.f;
  red[wave][0][lane] = pivot + s1 * inv;
  red[wave][1][lane] = fmaxf(s2 - s1 * s1 * inv, 0.f);
  __syncthreads();
  if (wave == 0 && cok) {
    float n = 0.f, mean = 0.f, m2 = 0.f;  // Chan merge of the four runs
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float nr = (float)max(0, min(RUN, T - (tbase + w * RUN)));
      if (nr > 0.f) {
        const float delta = red[w][0][lane] - mean, nt = n + nr;
        mean += delta * (nr / nt);
        m2 += red[w][1][lane] + delta * delta * (n * nr / nt);
        n = nt;
      }
    }
    long long blk = (long long)blockIdx.z * gridDim.y + blockIdx.y;
    partial[(blk * 2 + 0) * C + c] = mean;
    partial[(blk * 2 + 1) * C + c] = m2;
  }
}

// the workgroup's rows of a = value (* sigmoid(gate)) for this thread's channel: one element per lane and load
template <bool GLU, bool XB>
__device__ __forceinline__ void dwg_stage(float* as, const void* __restrict__ x, int ldx, int b, int T, int C, int c,
                                          bool cok, int tbase, int PAD, int ROWS, int lane, int wave) {
#pragma unroll 4
  for (int r = wave; r < ROWS; r += 4) {
    const int t = tbase - PAD + r;
    float v = 0.f;
    if (cok && t >= 0 && t < T) {
      const long long row = ((long long)b * T + t) * ldx;
      v = dw_ld<XB>(x, row + c);
      if (GLU) v *= fs2_sigmoid(dw_ld<XB>(x, row + C + c));
    }
    as[r * 64 + lane] = v;
  }
}

// per-thread-window form (any C): the variants of dwconv_fwd_kernel
template <bool GLU, bool STATS, bool XB = false, bool YB = XB>
__global__ __launch_bounds__(256) void dwconv_fwd_generic_kernel(const void* __restrict__ x, int ldx,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias, void* __restrict__ y,
                                                                  float* __restrict__ partial, int B, int T, int C,
                                                                  int K) {
  extern __shared__ __attribute__((aligned(16))) float dwg_lds[];  // as [ROWS][64] | red [4][2][64]
  const int PAD = (K - 1) / 2, ROWS = dwg_rows(K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int tbase = blockIdx.y * (4 * RUN), t0 = tbase + wave * RUN;
  const int b = blockIdx.z;
  const bool cok = c < C;
  float* as = dwg_lds;
  dwg_stage<GLU, XB>(as, x, ldx, b, T, C, c, cok, tbase, PAD, ROWS, lane, wave);
  const float bs = (cok && bias) ? bias[c] : 0.f;
  __syncthreads();
  float acc[RUN];
  dwg_conv(as + wave * RUN * 64 + lane, w, C, c, cok, K, bs, acc);
  float s1 = 0.f, s2 = 0.f, pivot = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    if (cok && t < T) {
      float v = acc[o];
      if constexpr (YB) {
        const unsigned short r = dw_bf16(v);
        ((unsigned short*)y)[((long long)b * T + t) * C + c] = r;
        v = __builtin_bit_cast(float, (unsigned)r << 16);
      } else {
        ((float*)y)[((long long)b * T + t) * C + c] = v;
      }
      if (STATS) {
        if (o == 0) pivot = v;
        const float d = v - pivot;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  if (STATS)
    dwg_stats(reinterpret_cast<float(*)[2][64]>(dwg_lds + ROWS * 64), partial, s1, s2, pivot, T, tbase, t0, C, c, cok,
              lane, wave);
}

// the variants of dwconv_bwd_kernel
template <bool GLU, bool DXB = false, bool XB = false>
__global__ __launch_bounds__(256) void dwconv_bwd_generic_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                                  int ldx, const float* __restrict__ w,
                                                                  void* __restrict__ dxv, float* __restrict__ partial,
                                                                  int B, int T, int C, int K) {
  extern __shared__ __attribute__((aligned(16))) float dwg_lds[];  // as [ROWS][64] | gs [ROWS][64] (then: red)
  const int PAD = (K - 1) / 2, ROWS = dwg_rows(K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int tbase = blockIdx.y * (4 * RUN), t0 = tbase + wave * RUN;
  const int b = blockIdx.z;
  const bool cok = c < C;
  float *as = dwg_lds, *gs = dwg_lds + ROWS * 64;
  dwg_stage<GLU, XB>(as, x, ldx, b, T, C, c, cok, tbase, PAD, ROWS, lane, wave);
#pragma unroll 4
  for (int r = wave; r < ROWS; r += 4) {
    const int t = tbase - PAD + r;
    gs[r * 64 + lane] = (cok && t >= 0 && t < T) ? dw_ld<XB>(dy, ((long long)b * T + t) * C + c) : 0.f;
  }
  __syncthreads();
  float da[RUN], gy[RUN];
  dwg_dgrad(gs + wave * RUN * 64 + lane, w, C, c, cok, K, da);
#pragma unroll
  for (int o = 0; o < RUN; ++o) gy[o] = gs[(wave * RUN + o + PAD) * 64 + lane];
  __syncthreads();  // gs becomes the tap-gradient reduction buffer
  dwg_wgrad(as + wave * RUN * 64 + lane, gy, gs, partial, (long long)b * gridDim.y + blockIdx.y, C, c, cok, K, lane,
            wave);
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    if (cok && t < T) {  // value and gate read again (L2), the sigmoid recomputed: the values of dwconv_bwd_kernel
      const long long xrow = ((long long)b * T + t) * ldx;
      const float vc = dw_ld<XB>(x, xrow + c), sc = GLU ? fs2_sigmoid(dw_ld<XB>(x, xrow + C + c)) : 0.f;
      if constexpr (DXB) {
        unsigned short* row = (unsigned short*)dxv + xrow;
        if (GLU) {
          row[c] = dw_bf16(da[o] * sc);
          row[C + c] = dw_bf16(da[o] * vc * sc * (1.f - sc));
        } else {
          row[c] = dw_bf16(da[o]);
        }
      } else {
        float* row = (float*)dxv + xrow;
        if (GLU) {
          row[c] = da[o] * sc;
          row[C + c] = da[o] * vc * sc * (1.f - sc);
        } else {
          row[c] = da[o];
        }
      }
    }
  }
}

// the workgroup's rows of value * sigmoid(gate) (and of dy, when gs is given): 16 bytes per lane and load
template <bool XB>
__device__ __forceinline__ void dwg_stage8(float* as, float* gs, const void* __restrict__ x, const void* __restrict__ dy,
                                           int ldx, int b, int T, int C, int c0, int tbase, int PAD, int ROWS, int tid) {
  const int sub = tid & 7;
  for (int r = tid >> 3; r < ROWS; r += 32) {
    const int t = tbase - PAD + r;
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < T) {
      const long long row = ((long long)b * T + t) * ldx + c0 + 8 * sub;
      float v8[8], g8[8];
      dw_ld8<XB>(x, row, v8);
      dw_ld8<XB>(x, row + C, g8);
#pragma unroll
      for (int j = 0; j < 8; ++j) a8[j] = v8[j] * fs2_sigmoid(g8[j]);
      if (gs) dw_ld8<XB>(dy, ((long long)b * T + t) * C + c0 + 8 * sub, d8);
    }
    dw_st8(&as[r * 64 + 8 * sub], a8);
    if (gs) dw_st8(&gs[r * 64 + 8 * sub], d8);
  }
}

// tiled form (C % 64 == 0, ldx % 8 == 0): the variants of dwconv_glu_fwd_tile_kernel
template <bool STATS, bool XB>
__global__ __launch_bounds__(256) void dwconv_glu_fwd_tile_generic_kernel(const void* __restrict__ x, int ldx,
                                                                           const float* __restrict__ w,
                                                                           const float* __restrict__ bias,
                                                                           void* __restrict__ y,
                                                                           float* __restrict__ partial, int B, int T,
                                                                           int C, int K) {
  // as [ROWS][64] (then: the results, [4 RUN][64]) | red [4][2][64]
  extern __shared__ __attribute__((aligned(16))) float dwg_lds[];
  const int PAD = (K - 1) / 2, ROWS = dwg_rows(K), TT = 4 * RUN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64, c = c0 + lane;
  const int tbase = blockIdx.y * TT, t0 = tbase + wave * RUN;
  const int b = blockIdx.z;
  float* as = dwg_lds;
  dwg_stage8<XB>(as, nullptr, x, nullptr, ldx, b, T, C, c0, tbase, PAD, ROWS, tid);
  const float bs = bias ? bias[c] : 0.f;
  __syncthreads();
  float acc[RUN];
  dwg_conv(as + wave * RUN * 64 + lane, w, C, c, true, K, bs, acc);
  __syncthreads();  // as becomes the result tile
  float s1 = 0.f, s2 = 0.f, pivot = 0.f;
#pragma unroll
  for (int o = 0; o < RUN; ++o) {
    int t = t0 + o;
    if (t < T) {
      float v = acc[o];
      if constexpr (XB) v = __builtin_bit_cast(float, (unsigned)dw_bf16(v) << 16);  // (the stored value)
      as[(wave * RUN + o) * 64 + lane] = v;
      if (STATS) {
        if (o == 0) pivot = v;
        const float d = v - pivot;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  if (STATS)
    dwg_stats(reinterpret_cast<float(*)[2][64]>(dwg_lds + ROWS * 64), partial, s1, s2, pivot, T, tbase, t0, C, c, true,
              lane, wave);
  else
    __syncthreads();
  const int sub = tid & 7;
#pragma unroll
  for (int r = tid >> 3; r < TT; r += 32) {
    const int t = tbase + r;
    if (t < T) dw_st8_global<XB>(y, ((long long)b * T + t) * C + c0 + 8 * sub, &as[r * 64 + 8 * sub]);
  }
}

// the variants of dwconv_glu_bwd_tile_kernel
template <bool XB>
__global__ __launch_bounds__(256) void dwconv_glu_bwd_tile_generic_kernel(const void* __restrict__ dy,
                                                                           const void* __restrict__ x, int ldx,
                                                                           const float* __restrict__ w,
                                                                           void* __restrict__ dxv,
                                                                           float* __restrict__ partial, int B, int T,
                                                                           int C, int dx_b, int K) {
  // as [ROWS][64] (then: da, [4 RUN][64]) | gs [ROWS][64] (then: red)
  extern __shared__ __attribute__((aligned(16))) float dwg_lds[];
  const int PAD = (K - 1) / 2, ROWS = dwg_rows(K), TT = 4 * RUN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64, c = c0 + lane;
  const int tbase = blockIdx.y * TT;
  const int b = blockIdx.z;
  float *as = dwg_lds, *gs = dwg_lds + ROWS * 64;
  dwg_stage8<XB>(as, gs, x, dy, ldx, b, T, C, c0, tbase, PAD, ROWS, tid);
  __syncthreads();
  float da[RUN], gy[RUN];
  dwg_dgrad(gs + wave * RUN * 64 + lane, w, C, c, true, K, da);
#pragma unroll
  for (int o = 0; o < RUN; ++o) gy[o] = gs[(wave * RUN + o + PAD) * 64 + lane];
  __syncthreads();  // gs becomes the tap-gradient reduction buffer
  dwg_wgrad(as + wave * RUN * 64 + lane, gy, gs, partial, (long long)b * gridDim.y + blockIdx.y, C, c, true, K, lane,
            wave);
#pragma unroll
  for (int o = 0; o < RUN; ++o) as[(wave * RUN + o) * 64 + lane] = da[o];
  __syncthreads();
  // dx = (da * s, da * v * s * (1 - s)) by rows, 16 bytes per lane; value and gate read again (L2), the sigmoid
  // recomputed: the values of dwconv_glu_bwd_tile_kernel
  const int sub = tid & 7;
#pragma unroll
  for (int r = tid >> 3; r < TT; r += 32) {
    const int t = tbase + r;
    if (t < T) {
      const long long row = ((long long)b * T + t) * ldx + c0 + 8 * sub;
      float v8[8], g8[8], d8[8], h8[8];
      dw_ld8<XB>(x, row, v8);
      dw_ld8<XB>(x, row + C, g8);
      const float4 p = *reinterpret_cast<const float4*>(&as[r * 64 + 8 * sub]);
      const float4 q = *reinterpret_cast<const float4*>(&as[r * 64 + 8 * sub + 4]);
      const float dd[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float sc = fs2_sigmoid(g8[j]), vc = v8[j];
        d8[j] = dd[j] * sc;
        h8[j] = dd[j] * vc * sc * (1.f - sc);
      }
      if (dx_b) {
        dw_st8_global_r<true>(dxv, row, d8);
        dw_st8_global_r<true>(dxv, row + C, h8);
      } else {
        dw_st8_global_r<false>(dxv, row, d8);
        dw_st8_global_r<false>(dxv, row + C, h8);
      }
    }
  }
}

bool dw_env_flag(const char* name, int value) {  // read at every call: tests and measurements flip them inside a process
  const char* e = getenv(name);
  return e && (atoi(e) != 0) == (value != 0);
}
bool dw_force_generic() { return dw_env_flag("FS2_DWCONV_GENERIC", 1); }  // every width on the run-time-K kernels
bool dw_tiles_off() { return dw_env_flag("FS2_DWCONV_TILE", 0); }  // the per-thread-window kernels everywhere
bool dw_generic_width(int K) { return K >= 1 && K <= KMAX && (K & 1); }

// The forms there are kernels for; the entry points refuse the others, the launchers instantiate nothing for them.
// Forward, io 0: fp32 tensors; 1: bf16 tensors -- the Conformer convolution module's GLU form only; 2: fp32 in, bf16 out
// -- the variance predictors' plain depthwise layer feeding a bf16-storage GEMM, without statistics.
constexpr bool dw_fwd_form(bool glu, bool stats, int io) {
  return io == 0 || (io == 1 && glu) || (io == 2 && !glu && !stats);
}
// Backward, x_bf16: dy and x are bf16 tensors -- the GLU form with a bf16 result only.
constexpr bool dw_bwd_form(bool glu, bool dx_bf16, bool x_bf16) { return !x_bf16 || (glu && dx_bf16); }

// The width as a constant for the six instantiated ones; 0: any other width, or FS2_DWCONV_GENERIC=1 -- the run-time-K
// kernels, which take K as their last argument and stage their windows in dynamic LDS.
template <class F>
int dw_pick_width(int K, F&& f) {
  return fs2_pick_int<0, 3, 5, 7, 9, 15, 31>(dw_force_generic() ? 0 : K, f);
}
size_t dw_fwd_shm(int K) { return (size_t)(dwg_rows(K) * 64 + 4 * 2 * 64) * sizeof(float); }
size_t dw_bwd_shm(int K) { return (size_t)(2 * dwg_rows(K) * 64) * sizeof(float); }

struct DwLaunch {
  dim3 grid;
  hipStream_t s;
  int B, T, C, K;
};
DwLaunch dw_launch(int B, int T, int C, int K, void* stream) {
  return {dim3((C + 63) / 64, (T + 4 * RUN - 1) / (4 * RUN), B), (hipStream_t)stream, B, T, C, K};
}

int dw_fwd_plain(const DwLaunch& l, const void* x, int ldx, const float* w, const float* bias, void* y, float* partial,
                 bool glu, bool stats, int io) {
  return dw_pick_width(l.K, [&](auto kc) {
    return fs2_pick_bool(glu, [&](auto g) {
      return fs2_pick_bool(stats, [&](auto st) {
        return fs2_pick_int<0, 1, 2>(io, [&](auto ioc) {
          constexpr bool XB = ioc == 1, YB = ioc != 0;
          if constexpr (!dw_fwd_form(g, st, ioc)) {
            return (int)FS2HIP_EINVAL;
          } else if constexpr (kc == 0) {
            if (!dw_generic_width(l.K)) return (int)FS2HIP_EINVAL;
            dwconv_fwd_generic_kernel<g, st, XB, YB><<<l.grid, dim3(256), dw_fwd_shm(l.K), l.s>>>(x, ldx, w, bias, y, partial,
                                                                                                 l.B, l.T, l.C, l.K);
            return fs2_launched();
          } else {
            dwconv_fwd_kernel<kc, g, st, XB, YB><<<l.grid, dim3(256), 0, l.s>>>(x, ldx, w, bias, y, partial, l.B, l.T, l.C);
            return fs2_launched();
          }
        });
      });
    });
  });
}

// the LDS-tiled GLU kernels: x_bf16 = x and y are bf16 tensors
int dw_fwd_tile(const DwLaunch& l, const void* x, int ldx, const float* w, const float* bias, void* y, float* partial,
                bool stats, bool x_bf16) {
  return dw_pick_width(l.K, [&](auto kc) {
    return fs2_pick_bool(stats, [&](auto st) {
      return fs2_pick_bool(x_bf16, [&](auto xb) {
        if constexpr (kc == 0) {
          if (!dw_generic_width(l.K)) return (int)FS2HIP_EINVAL;
          dwconv_glu_fwd_tile_generic_kernel<st, xb><<<l.grid, dim3(256), dw_fwd_shm(l.K), l.s>>>(x, ldx, w, bias, y, partial,
                                                                                                 l.B, l.T, l.C, l.K);
        } else {
          dwconv_glu_fwd_tile_kernel<kc, st, xb><<<l.grid, dim3(256), 0, l.s>>>(x, ldx, w, bias, y, partial, l.B, l.T, l.C);
        }
        return fs2_launched();
      });
    });
  });
}

int dw_bwd_plain(const DwLaunch& l, const void* dy, const void* x, int ldx, const float* w, void* dx, float* partial,
                 bool glu, bool dx_bf16, bool x_bf16) {
  return dw_pick_width(l.K, [&](auto kc) {
    return fs2_pick_bool(glu, [&](auto g) {
      return fs2_pick_bool(dx_bf16, [&](auto dxb) {
        return fs2_pick_bool(x_bf16, [&](auto xb) {
          if constexpr (!dw_bwd_form(g, dxb, xb)) {
            return (int)FS2HIP_EINVAL;
          } else if constexpr (kc == 0) {
            if (!dw_generic_width(l.K)) return (int)FS2HIP_EINVAL;
            dwconv_bwd_generic_kernel<g, dxb, xb><<<l.grid, dim3(256), dw_bwd_shm(l.K), l.s>>>(dy, x, ldx, w, dx, partial, l.B,
                                                                                              l.T, l.C, l.K);
            return fs2_launched();
          } else {
            dwconv_bwd_kernel<kc, g, dxb, xb><<<l.grid, dim3(256), 0, l.s>>>(dy, x, ldx, w, dx, partial, l.B, l.T, l.C);
            return fs2_launched();
          }
        });
      });
    });
  });
}

// the LDS-tiled GLU kernels: the type of dx is a run-time argument of theirs
int dw_bwd_tile(const DwLaunch& l, const void* dy, const void* x, int ldx, const float* w, void* dx, float* partial,
                int dx_bf16, bool x_bf16) {
  return dw_pick_width(l.K, [&](auto kc) {
    return fs2_pick_bool(x_bf16, [&](auto xb) {
      if constexpr (kc == 0) {
        if (!dw_generic_width(l.K)) return (int)FS2HIP_EINVAL;
        dwconv_glu_bwd_tile_generic_kernel<xb><<<l.grid, dim3(256), dw_bwd_shm(l.K), l.s>>>(dy, x, ldx, w, dx, partial, l.B,
                                                                                           l.T, l.C, dx_bf16, l.K);
      } else {
        dwconv_glu_bwd_tile_kernel<kc, xb><<<l.grid, dim3(256), 0, l.s>>>(dy, x, ldx, w, dx, partial, l.B, l.T, l.C, dx_bf16);
      }
      return fs2_launched();
    });
  });
}

}  // namespace

extern "C" int fs2hip_dwconv_blocks(int B, int T) { return B * ((T + 4 * RUN - 1) / (4 * RUN)); }
extern "C" int fs2hip_dwconv_part_rows(void) { return 4 * RUN; }

extern "C" int fs2hip_dwconv_fwd_b(const void* x, int ldx, const float* w, const float* bias, void* y, float* partial,
                                   int B, int T, int C, int K, int glu, int stats, int io_bf16, void* stream);
extern "C" int fs2hip_dwconv_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, float* partial,
                                 int B, int T, int C, int K, int glu, int stats, void* stream) {
  return fs2hip_dwconv_fwd_b(x, ldx, w, bias, y, partial, B, T, C, K, glu, stats, 0, stream);
}

// io_bf16 = 1: x and y are bf16 tensors (GLU form only); 2: x fp32, y bf16 (plain form, no statistics)
extern "C" int fs2hip_dwconv_fwd_b(const void* x, int ldx, const float* w, const float* bias, void* y, float* partial,
                                   int B, int T, int C, int K, int glu, int stats, int io_bf16, void* stream) {
  if (B <= 0 || T <= 0 || C <= 0 || ldx < (glu ? 2 * C : C)) return FS2HIP_EINVAL;
  if (stats && !partial) return FS2HIP_EINVAL;
  if (io_bf16 < 0 || io_bf16 > 2 || !dw_fwd_form(glu, stats, io_bf16)) return FS2HIP_EINVAL;
  const DwLaunch l = dw_launch(B, T, C, K, stream);
  if (glu && !dw_tiles_off() && (C % 64) == 0 && (ldx % 8) == 0 && ((uintptr_t)x % 16) == 0)
    return dw_fwd_tile(l, x, ldx, w, bias, y, partial, stats, io_bf16 == 1);
  return dw_fwd_plain(l, x, ldx, w, bias, y, partial, glu, stats, io_bf16);
}

// partial: [fs2hip_dwconv_blocks(B,T)][K+1][C]; dw [K][C], dbias [C] are finished here
extern "C" int fs2hip_dwconv_bwd_b(const void* dy, const void* x, int ldx, const float* w, void* dx, int dx_bf16,
                                   float* partial, float* dw, float* dbias, int B, int T, int C, int K, int glu,
                                   void* stream);
extern "C" int fs2hip_dwconv_bwd(const float* dy, const float* x, int ldx, const float* w, float* dx, float* partial,
                                 float* dw, float* dbias, int B, int T, int C, int K, int glu, void* stream) {
  return fs2hip_dwconv_bwd_b(dy, x, ldx, w, dx, 0, partial, dw, dbias, B, T, C, K, glu, stream);
}

// dx_bf16 bit 0: dx (layout of x, leading dimension ldx) is written as bf16; bit 1: dy and x are bf16 tensors
extern "C" int fs2hip_dwconv_bwd_b(const void* dy, const void* x, int ldx, const float* w, void* dx, int dx_bf16,
                                   float* partial, float* dw, float* dbias, int B, int T, int C, int K, int glu,
                                   void* stream) {
  if (B <= 0 || T <= 0 || C <= 0 || ldx < (glu ? 2 * C : C) || !partial) return FS2HIP_EINVAL;
  const bool x_bf16 = dx_bf16 & 2;
  if (!dw_bwd_form(glu, dx_bf16 & 1, x_bf16)) return FS2HIP_EINVAL;
  const DwLaunch l = dw_launch(B, T, C, K, stream);
  const bool tile = glu && !dw_tiles_off() && (C % 64) == 0 && (ldx % 8) == 0 && ((uintptr_t)x % 16) == 0 &&
                    ((uintptr_t)dy % 16) == 0;
  const int launched = tile ? dw_bwd_tile(l, dy, x, ldx, w, dx, partial, dx_bf16 & 1, x_bf16)
                            : dw_bwd_plain(l, dy, x, ldx, w, dx, partial, glu, dx_bf16 != 0, x_bf16);
  if (launched) return launched;
  if (!dw) return 0;  // partial sums only: the caller finishes them with fs2hip_reduce_rows_multi (same sums, same order)
  const int nblk = fs2hip_dwconv_blocks(B, T);
  const long long stride = (long long)(K + 1) * C;
  // (one launch for both when they take the row-parallel path of fs2hip_reduce_slabs anyway: same sums, same order)
  if (dbias && stride <= 16384 && nblk >= 8)
    return fs2_reduce_rows(partial, nblk, (int)stride, stride, dw, K * C, dbias, (hipStream_t)stream);
  int rc = fs2hip_reduce_slabs(partial, dw, (long long)K * C, nblk, stride, stream);
  if (rc) return rc;
  if (dbias) rc = fs2hip_reduce_slabs(partial + (long long)K * C, dbias, C, nblk, stride, stream);
  return rc;
}
