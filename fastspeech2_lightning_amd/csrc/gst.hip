// GST style encoder kernels (reference fs2/gst/model.py:103-257, fs2/gst/attn.py:48-194) -- BASELINE config 5.
// The whole branch is ~0.3 % of the step's FLOPs (6 small stride-2 convs over the mel, an 11-step GRU(128),
// a 10-token attention), so these are simple VALU kernels laid out for coalescing, not MFMA work:
//   conv2d_s2       : 3x3, stride 2, pad 1, no bias, channels-last [B][H][W][C]; weights [kh][kw][ci][co]
//   gru_gate        : r, z, n gates + state update of one time step (the two matmuls run on the GEMM kernel)
//   gst_attn        : softmax(q k^T / sqrt(d_k)) v of one query per utterance against the style tokens
//   gru_last_state  : the whole inference recurrence in one launch, a step count per utterance (length-aware inference)
//   conv_s2_lens    : the row counts an utterance keeps after each stride-2 convolution
//   gru_fwd_states  : gru_last_state kept for training: also writes every step's state and gates (168 VGPRs, no scratch)
//   gru_bwd_states  : the whole backward through time in one launch, w_hh columns in registers (152 VGPRs, no scratch)
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void conv2d_s2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             float* __restrict__ y, int B, int H, int W, int Cin,
                                                             int Ho, int Wo, int Cout) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * Ho * Wo * Cout;
  if (idx >= total) return;
  const int co = (int)(idx % Cout);
  long long row = idx / Cout;
  const int wo = (int)(row % Wo);
  row /= Wo;
  const int ho = (int)(row % Ho), b = (int)(row / Ho);
  float acc = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int hi = 2 * ho + kh - 1;
    if (hi < 0 || hi >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int wi = 2 * wo + kw - 1;
      if (wi < 0 || wi >= W) continue;
      const float* xp = x + (((long long)b * H + hi) * W + wi) * Cin;
      const float* wp = w + (long long)(kh * 3 + kw) * Cin * Cout + co;
      for (int ci = 0; ci < Cin; ++ci) acc = fmaf(xp[ci], wp[(long long)ci * Cout], acc);
    }
  }
  y[idx] = acc;
}

// The reference encoder's FIRST layer (fs2/gst/model.py:103-139: Conv2d(1, 32, 3, stride 2) over the mel "image"): one
// input channel, so a thread of the generic kernel above loaded 9 + 9 scalars for ONE output and the launch -- 53 M
// threads for the configs[4] batch -- took 419 us to write 211 MB (round 5 profile; the style encoder's forward pass is
// what the main stream waits for at its join).  Here a thread makes four neighbouring output channels of a pixel: the
// nine taps once, nine 16-byte weight loads, one 16-byte store; the same fmaf sequence per output (taps outside the
// image skipped, in the same order), so the results are the generic kernel's bit for bit.
__global__ __launch_bounds__(256) void conv2d_s2_fwd_c1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                float* __restrict__ y, int B, int H, int W, int Ho, int Wo,
                                                                int Cout) {
  const int c4n = Cout >> 2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * Ho * Wo * c4n;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n);
  long long row = idx / c4n;
  const int wo = (int)(row % Wo);
  row /= Wo;
  const int ho = (int)(row % Ho), b = (int)(row / Ho);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int hi = 2 * ho + kh - 1;
    if (hi < 0 || hi >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int wi = 2 * wo + kw - 1;
      if (wi < 0 || wi >= W) continue;
      const float xv = x[((long long)b * H + hi) * W + wi];
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (kh * 3 + kw) * Cout + 4 * c4);
      acc[0] = fmaf(xv, wv[0], acc[0]);
      acc[1] = fmaf(xv, wv[1], acc[1]);
      acc[2] = fmaf(xv, wv[2], acc[2]);
      acc[3] = fmaf(xv, wv[3], acc[3]);
    }
  }
  *reinterpret_cast<f32x4*>(y + idx * 4) = acc;
}

// dx[b,hi,wi,ci] = sum over (kh,kw) with hi = 2ho+kh-1, wi = 2wo+kw-1 of sum_co dy[b,ho,wo,co] * w[kh][kw][ci][co]
__global__ __launch_bounds__(256) void conv2d_s2_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                  float* __restrict__ dx, int B, int H, int W, int Cin,
                                                                  int Ho, int Wo, int Cout) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * H * W * Cin;
  if (idx >= total) return;
  const int ci = (int)(idx % Cin);
  long long row = idx / Cin;
  const int wi = (int)(row % W);
  row /= W;
  const int hi = (int)(row % H), b = (int)(row / H);
  float acc = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int h2 = hi + 1 - kh;
    if (h2 < 0 || (h2 & 1) || (h2 >> 1) >= Ho) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int w2 = wi + 1 - kw;
      if (w2 < 0 || (w2 & 1) || (w2 >> 1) >= Wo) continue;
      const float* dp = dy + (((long long)b * Ho + (h2 >> 1)) * Wo + (w2 >> 1)) * Cout;
      const float* wp = w + ((long long)(kh * 3 + kw) * Cin + ci) * Cout;
      for (int co = 0; co < Cout; ++co) acc = fmaf(dp[co], wp[co], acc);
    }
  }
  dx[idx] = acc;
}

constexpr int CW_ROWS = 2048;  // output rows per partial of the weight gradient
// partial[chunk][kh][kw][ci][co] = sum over the chunk's output rows of x[...] * dy[row][co]
__global__ __launch_bounds__(256) void conv2d_s2_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    float* __restrict__ partial, int B, int H, int W,
                                                                    int Cin, int Ho, int Wo, int Cout) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int nw = 9 * Cin * Cout;
  if (e >= nw) return;
  const int co = e % Cout, ci = (e / Cout) % Cin, k = e / (Cout * Cin);
  const int kh = k / 3, kw = k % 3;
  const long long rows = (long long)B * Ho * Wo;
  const long long r0 = (long long)blockIdx.y * CW_ROWS, r1 = min(rows, r0 + CW_ROWS);
  float acc = 0.f;
  for (long long r = r0; r < r1; ++r) {
    const int wo = (int)(r % Wo);
    const long long t = r / Wo;
    const int ho = (int)(t % Ho), b = (int)(t / Ho);
    const int hi = 2 * ho + kh - 1, wi = 2 * wo + kw - 1;
    if (hi < 0 || hi >= H || wi < 0 || wi >= W) continue;
    acc = fmaf(x[(((long long)b * H + hi) * W + wi) * Cin + ci], dy[r * Cout + co], acc);
  }
  partial[(long long)blockIdx.y * nw + e] = acc;
}

// ---- GRU (nn.GRU gate order r, z, n) ----------------------------------------------------------------
// gi: rows of stride gi_stride (input projections incl. b_ih of step t), gh [B][3U] (recurrent incl. b_hh)
// ---- 3x3 stride-2 convolution as GEMM (Cin % 4 == 0): gather the 9 taps of every output pixel into a row of
// col[B*Ho*Wo][9*Cin] (zero where the window leaves the image), multiply by the weight seen as [9*Cin][Cout] on the
// MFMA GEMM; backward data is the GEMM dcol = dy W^T followed by the inverse gather (each input pixel belongs to at
// most four windows).  The direct kernels above reached ~1 TFLOP/s, which made the style encoder 30 % of a
// configs[4]-shaped step; only the first layer (Cin = 1, 9 MACs per output) still uses them.
__global__ __launch_bounds__(256) void im2col_s2_kernel(const float* __restrict__ x, float* __restrict__ col, int B,
                                                         int H, int W, int Cin, int Ho, int Wo) {
  const int c4n = Cin >> 2;
  const long long total = (long long)B * Ho * Wo * 9 * c4n;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c4 = (int)(idx % c4n);
    long long r = idx / c4n;
    const int tap = (int)(r % 9);
    r /= 9;  // output pixel (b, ho, wo)
    const int wo = (int)(r % Wo);
    const long long bh = r / Wo;
    const int ho = (int)(bh % Ho), b = (int)(bh / Ho);
    const int hi = 2 * ho + tap / 3 - 1, wi = 2 * wo + tap % 3 - 1;
    float4 v = make_float4(0, 0, 0, 0);
    if (hi >= 0 && hi < H && wi >= 0 && wi < W)
      v = *reinterpret_cast<const float4*>(x + (((long long)b * H + hi) * W + wi) * Cin + c4 * 4);
    *reinterpret_cast<float4*>(col + r * (9LL * Cin) + (long long)tap * Cin + c4 * 4) = v;
  }
}

// single input channel (the mel itself): rows of 12 floats = 9 taps + 3 zeros, for the weight-gradient GEMM
__global__ __launch_bounds__(256) void im2col_s2_c1_kernel(const float* __restrict__ x, float* __restrict__ col, int B,
                                                            int H, int W, int Ho, int Wo) {
  const long long total = (long long)B * Ho * Wo;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < total; r += (long long)gridDim.x * 256) {
    const int wo = (int)(r % Wo);
    const long long bh = r / Wo;
    const int ho = (int)(bh % Ho), b = (int)(bh / Ho);
    float v[12];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int hi = 2 * ho + tap / 3 - 1, wi = 2 * wo + tap % 3 - 1;
      v[tap] = (hi >= 0 && hi < H && wi >= 0 && wi < W) ? x[((long long)b * H + hi) * W + wi] : 0.f;
    }
    v[9] = v[10] = v[11] = 0.f;
    float4* dst = reinterpret_cast<float4*>(col + r * 12);
    dst[0] = make_float4(v[0], v[1], v[2], v[3]);
    dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    dst[2] = make_float4(v[8], v[9], v[10], v[11]);
  }
}

__global__ __launch_bounds__(256) void col2im_s2_kernel(const float* __restrict__ dcol, float* __restrict__ dx, int B,
                                                         int H, int W, int Cin, int Ho, int Wo) {
  const int c4n = Cin >> 2;
  const long long total = (long long)B * H * W * c4n;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c4 = (int)(idx % c4n);
    long long r = idx / c4n;
    const int wi = (int)(r % W);
    const long long bh = r / W;
    const int hi = (int)(bh % H), b = (int)(bh / H);
    float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h2 = hi + 1 - kh;
      if (h2 < 0 || (h2 & 1) || (h2 >> 1) >= Ho) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w2 = wi + 1 - kw;
        if (w2 < 0 || (w2 & 1) || (w2 >> 1) >= Wo) continue;
        const long long m = ((long long)b * Ho + (h2 >> 1)) * Wo + (w2 >> 1);
        const float4 v = *reinterpret_cast<const float4*>(dcol + m * (9LL * Cin) + (long long)(kh * 3 + kw) * Cin + c4 * 4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    *reinterpret_cast<float4*>(dx + r * Cin + c4 * 4) = acc;
  }
}

__global__ void gru_gate_fwd_kernel(const float* __restrict__ gi, long long gi_stride, const float* __restrict__ gh,
                                    const float* __restrict__ hprev, float* __restrict__ hnew, float* __restrict__ gates,
                                    int B, int U) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * U) return;
  const int b = i / U, j = i % U;
  const float* gib = gi + (long long)b * gi_stride;
  const float* ghb = gh + (long long)b * 3 * U;
  const float r = fs2_sigmoid(gib[j] + ghb[j]);
  const float z = fs2_sigmoid(gib[U + j] + ghb[U + j]);
  const float hn = ghb[2 * U + j];
  const float n = tanhf(gib[2 * U + j] + r * hn);
  hnew[i] = (1.f - z) * n + z * hprev[i];
  float* g = gates + (long long)b * 4 * U;  // saved for the backward: r, z, n, gh_n
  g[j] = r; g[U + j] = z; g[2 * U + j] = n; g[3 * U + j] = hn;
}
// dh: gradient of h_t; outputs dgi (row stride dgi_stride), dgh [B][3U], dhprev = dh * z (the recurrent matmul's
// contribution is added by the caller)
__global__ void gru_gate_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ gates,
                                    const float* __restrict__ hprev, float* __restrict__ dgi, long long dgi_stride,
                                    float* __restrict__ dgh, float* __restrict__ dhprev, int B, int U) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * U) return;
  const int b = i / U, j = i % U;
  const float* g = gates + (long long)b * 4 * U;
  const float r = g[j], z = g[U + j], n = g[2 * U + j], hn = g[3 * U + j];
  const float d = dh[i];
  const float dn = d * (1.f - z) * (1.f - n * n);
  const float dz = d * (hprev[i] - n) * z * (1.f - z);
  const float dr = dn * hn * r * (1.f - r);
  float* a = dgi + (long long)b * dgi_stride;
  float* c = dgh + (long long)b * 3 * U;
  a[j] = dr; a[U + j] = dz; a[2 * U + j] = dn;
  c[j] = dr; c[U + j] = dz; c[2 * U + j] = dn * r;
  dhprev[i] = d * z;
}

// ---- the whole inference recurrence in one launch, a step count per utterance (fs2hip_gru_last_state) ----
// One workgroup per utterance, one thread per gate row: thread j keeps row j of w_hh [3U][U] in registers for all steps
// (128 VGPRs; loaded once), h [U] and the 3U recurrent sums live in LDS.  A step is: every thread's dot product of its row
// with h (k ascending, one fmaf chain -- the result of a row is a function of that utterance's gi alone, whatever the
// batch), a barrier, the gates on the first U threads, a barrier.  gi rows at and beyond the utterance's step count are
// never addressed.  The step's three gi values are requested before the dot product and used after it.
constexpr int GRU_U = 128;
__global__ __launch_bounds__(3 * GRU_U) void gru_last_state_kernel(const float* __restrict__ gi,
                                                                    const float* __restrict__ w_hh,
                                                                    const float* __restrict__ b_hh,
                                                                    const int* __restrict__ steps,
                                                                    float* __restrict__ h_out, int T) {
  constexpr int U = GRU_U;
  __shared__ __attribute__((aligned(16))) float sh[U];
  __shared__ float sgh[3 * U];
  const int b = blockIdx.x, j = threadIdx.x;
  int n = steps[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  if (n == 0) {  // (uniform over the workgroup)
    if (j < U) h_out[(long long)b * U + j] = 0.f;
    return;
  }
  float w[U];
  const f32x4* wrow = reinterpret_cast<const f32x4*>(w_hh + (long long)j * U);
#pragma unroll
  for (int k4 = 0; k4 < U / 4; ++k4) {
    const f32x4 v = wrow[k4];
    w[4 * k4] = v[0]; w[4 * k4 + 1] = v[1]; w[4 * k4 + 2] = v[2]; w[4 * k4 + 3] = v[3];
  }
  const float bias = b_hh[j];
  float h = 0.f;  // thread j < U: element j of the state
  if (j < U) sh[j] = 0.f;
  __syncthreads();
  const float* gib = gi + (long long)b * T * 3 * U;
  const f32x4* sh4 = reinterpret_cast<const f32x4*>(sh);
  for (int t = 0; t < n; ++t) {
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (j < U) {
      const float* g = gib + (long long)t * 3 * U;
      gr = g[j]; gz = g[U + j]; gn = g[2 * U + j];
    }
    float acc = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < U / 4; ++k4) {
      const f32x4 hv = sh4[k4];
      acc = fmaf(hv[0], w[4 * k4], acc);
      acc = fmaf(hv[1], w[4 * k4 + 1], acc);
      acc = fmaf(hv[2], w[4 * k4 + 2], acc);
      acc = fmaf(hv[3], w[4 * k4 + 3], acc);
    }
    sgh[j] = acc + bias;
    __syncthreads();
    if (j < U) {
      const float r = fs2_sigmoid(gr + sgh[j]);
      const float z = fs2_sigmoid(gz + sgh[U + j]);
      const float c = tanhf(gn + r * sgh[2 * U + j]);
      h = (1.f - z) * c + z * h;
      sh[j] = h;
    }
    __syncthreads();
  }
  if (j < U) h_out[(long long)b * U + j] = h;
}

// ---- the same recurrence kept for training (fs2hip_gru_fwd_states): gru_last_state_kernel, step for step and in its
// arithmetic order (the final state is bit-equal), which also writes hs [B][T+1][U] (hs[b][0] = 0, hs[b][t+1] = the state
// after step t) and gates [B][T][4U] = (r, z, n, gh_n) as gru_gate_fwd_kernel saves them.  Rows beyond the utterance's
// step count are written as zeros: a weight-gradient GEMM over all rows multiplies them by zero gradient rows.
__global__ __launch_bounds__(3 * GRU_U) void gru_fwd_states_kernel(const float* __restrict__ gi,
                                                                    const float* __restrict__ w_hh,
                                                                    const float* __restrict__ b_hh,
                                                                    const int* __restrict__ steps, float* __restrict__ hs,
                                                                    float* __restrict__ gates, float* __restrict__ h_out,
                                                                    int T) {
  constexpr int U = GRU_U;
  __shared__ __attribute__((aligned(16))) float sh[U];
  __shared__ float sgh[3 * U];
  const int b = blockIdx.x, j = threadIdx.x;
  int n = steps[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  float* hsb = hs + (long long)b * (T + 1) * U;
  float* gtb = gates + (long long)b * T * 4 * U;
  // the rows no step writes: hs[b][0], hs[b][n + 1 ..], gates[b][n ..]
  for (int i = j; i < (T + 1) * U; i += 3 * U)
    if (i < U || i >= (n + 1) * U) hsb[i] = 0.f;
  for (int i = n * 4 * U + j; i < T * 4 * U; i += 3 * U) gtb[i] = 0.f;
  if (n == 0) {  // (uniform over the workgroup)
    if (j < U) h_out[(long long)b * U + j] = 0.f;
    return;
  }
  float w[U];
  const f32x4* wrow = reinterpret_cast<const f32x4*>(w_hh + (long long)j * U);
#pragma unroll
  for (int k4 = 0; k4 < U / 4; ++k4) {
    const f32x4 v = wrow[k4];
    w[4 * k4] = v[0]; w[4 * k4 + 1] = v[1]; w[4 * k4 + 2] = v[2]; w[4 * k4 + 3] = v[3];
  }
  const float bias = b_hh[j];
  float h = 0.f;  // thread j < U: element j of the state
  if (j < U) sh[j] = 0.f;
  __syncthreads();
  const float* gib = gi + (long long)b * T * 3 * U;
  const f32x4* sh4 = reinterpret_cast<const f32x4*>(sh);
  for (int t = 0; t < n; ++t) {
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (j < U) {
      const float* g = gib + (long long)t * 3 * U;
      gr = g[j]; gz = g[U + j]; gn = g[2 * U + j];
    }
    float acc = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < U / 4; ++k4) {
      const f32x4 hv = sh4[k4];
      acc = fmaf(hv[0], w[4 * k4], acc);
      acc = fmaf(hv[1], w[4 * k4 + 1], acc);
      acc = fmaf(hv[2], w[4 * k4 + 2], acc);
      acc = fmaf(hv[3], w[4 * k4 + 3], acc);
    }
    sgh[j] = acc + bias;
    __syncthreads();
    if (j < U) {
      const float hn = sgh[2 * U + j];
      const float r = fs2_sigmoid(gr + sgh[j]);
      const float z = fs2_sigmoid(gz + sgh[U + j]);
      const float c = tanhf(gn + r * hn);
      h = (1.f - z) * c + z * h;
      sh[j] = h;
      float* g = gtb + (long long)t * 4 * U;
      g[j] = r; g[U + j] = z; g[2 * U + j] = c; g[3 * U + j] = hn;
      hsb[(long long)(t + 1) * U + j] = h;
    }
    __syncthreads();
  }
  if (j < U) h_out[(long long)b * U + j] = h;
}

// ---- the whole backward through time in one launch (fs2hip_gru_bwd_states), one workgroup per utterance ----
// Thread (g, k) = threadIdx g * U + k keeps COLUMN k of gate block g of w_hh [3U][U] in 128 registers (strided loads,
// coalesced over k, once).  A step, from the utterance's last down to 0: the first U threads take the gate derivatives
// of gru_gate_bwd_kernel from dh (a register), the saved gates and h_{t-1}, write dgi[b][t] and dgh[b][t] and leave dgh in
// LDS; a barrier; every thread's dot product of its column with its gate block's dgh (broadcast LDS reads, i ascending,
// one fmaf chain); a barrier; dh_{t-1}[k] = dh[k] * z[k] + ((part_r[k] + part_z[k]) + part_n[k]).  Rows at and beyond
// the step count -- row T of dgh included, which pairs with hs[b][T] in the recurrent weight gradient -- are exact zeros.
// Nothing is read from another utterance: a row's outputs are bit-equal whatever the batch.
__global__ __launch_bounds__(3 * GRU_U) void gru_bwd_states_kernel(const float* __restrict__ dh_last,
                                                                    const float* __restrict__ hs,
                                                                    const float* __restrict__ gates,
                                                                    const float* __restrict__ w_hh,
                                                                    const int* __restrict__ steps, float* __restrict__ dgi,
                                                                    float* __restrict__ dgh, float* __restrict__ dh0,
                                                                    int T) {
  constexpr int U = GRU_U;
  __shared__ __attribute__((aligned(16))) float sd[3 * U];
  __shared__ float sp[3 * U];
  const int b = blockIdx.x, j = threadIdx.x;
  int n = steps[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  float* dgib = dgi + (long long)b * T * 3 * U;
  float* dghb = dgh + (long long)b * (T + 1) * 3 * U;
  for (int i = n * 3 * U + j; i < T * 3 * U; i += 3 * U) dgib[i] = 0.f;
  for (int i = n * 3 * U + j; i < (T + 1) * 3 * U; i += 3 * U) dghb[i] = 0.f;
  float d = j < U ? dh_last[(long long)b * U + j] : 0.f;
  if (n == 0) {  // (uniform over the workgroup) no step: h_last = h0
    if (j < U) dh0[(long long)b * U + j] = d;
    return;
  }
  const int gb = j / U, k = j - gb * U;
  float w[U];
#pragma unroll
  for (int i = 0; i < U; ++i) w[i] = w_hh[(long long)(gb * U + i) * U + k];
  const float* hsb = hs + (long long)b * (T + 1) * U;
  const float* gtb = gates + (long long)b * T * 4 * U;
  const f32x4* sd4 = reinterpret_cast<const f32x4*>(sd + gb * U);
  for (int t = n - 1; t >= 0; --t) {
    float z = 0.f;
    if (j < U) {
      const float* g = gtb + (long long)t * 4 * U;
      const float r = g[j], c = g[2 * U + j], hn = g[3 * U + j];
      z = g[U + j];
      const float dn = d * (1.f - z) * (1.f - c * c);
      const float dz = d * (hsb[(long long)t * U + j] - c) * z * (1.f - z);
      const float dr = dn * hn * r * (1.f - r);
      float* a = dgib + (long long)t * 3 * U;
      float* e = dghb + (long long)t * 3 * U;
      a[j] = dr; a[U + j] = dz; a[2 * U + j] = dn;
      e[j] = dr; e[U + j] = dz; e[2 * U + j] = dn * r;
      sd[j] = dr; sd[U + j] = dz; sd[2 * U + j] = dn * r;
    }
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int i4 = 0; i4 < U / 4; ++i4) {
      const f32x4 v = sd4[i4];
      acc = fmaf(v[0], w[4 * i4], acc);
      acc = fmaf(v[1], w[4 * i4 + 1], acc);
      acc = fmaf(v[2], w[4 * i4 + 2], acc);
      acc = fmaf(v[3], w[4 * i4 + 3], acc);
    }
    sp[j] = acc;
    __syncthreads();
    if (j < U) d = d * z + ((sp[j] + sp[U + j]) + sp[2 * U + j]);
  }
  if (j < U) dh0[(long long)b * U + j] = d;
}

// table[l][b], l = 0 .. n: the row counts an utterance of lens[b] frames has after l stride-2 convolutions
__global__ void conv_s2_lens_kernel(const int* __restrict__ lens, int* __restrict__ table, int B, int n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int v = lens[b];
  table[b] = v;
  for (int l = 1; l <= n; ++l) {
    v = v > 0 ? (v - 1) / 2 + 1 : 0;
    table[(long long)l * B + b] = v;
  }
}

// ---- style-token attention: one query per utterance, NT tokens, HEADS x 64 dims (one wavefront per head) ----
constexpr int GST_MAX_TOKENS = 32;
__global__ __launch_bounds__(256) void gst_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, float* __restrict__ p,
                                                            float* __restrict__ ctx, int B, int NT, int heads) {
  const int b = blockIdx.x, h = threadIdx.x >> 6, d = threadIdx.x & 63;
  if (h >= heads) return;
  const int F = heads * 64;
  const float qv = q[(long long)b * F + h * 64 + d];
  float s[GST_MAX_TOKENS];
  float m = -INFINITY;
  for (int j = 0; j < NT; ++j) {
    s[j] = fs2_wave_sum(qv * k[(long long)j * F + h * 64 + d]) * 0.125f;  // 1/sqrt(64)
    m = fmaxf(m, s[j]);
  }
  float den = 0.f;
  for (int j = 0; j < NT; ++j) { s[j] = expf(s[j] - m); den += s[j]; }
  float acc = 0.f;
  for (int j = 0; j < NT; ++j) {
    const float pj = s[j] / den;
    if (d == 0) p[((long long)b * heads + h) * NT + j] = pj;
    acc = fmaf(pj, v[(long long)j * F + h * 64 + d], acc);
  }
  ctx[(long long)b * F + h * 64 + d] = acc;
}
// dq [B][F]; dk_part, dv_part [B][NT][F] (summed over the batch by the caller)
__global__ __launch_bounds__(256) void gst_attn_bwd_kernel(const float* __restrict__ dctx, const float* __restrict__ q,
                                                            const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ p, float* __restrict__ dq,
                                                            float* __restrict__ dk_part, float* __restrict__ dv_part,
                                                            int B, int NT, int heads) {
  const int b = blockIdx.x, h = threadIdx.x >> 6, d = threadIdx.x & 63;
  if (h >= heads) return;
  const int F = heads * 64;
  const long long o = (long long)b * F + h * 64 + d;
  const float dc = dctx[o], qv = q[o];
  const float* pb = p + ((long long)b * heads + h) * NT;
  float dp[GST_MAX_TOKENS];
  float dot = 0.f;
  for (int j = 0; j < NT; ++j) {
    dp[j] = fs2_wave_sum(dc * v[(long long)j * F + h * 64 + d]);
    dot += pb[j] * dp[j];
  }
  float acc = 0.f;
  for (int j = 0; j < NT; ++j) {
    const float ds = pb[j] * (dp[j] - dot) * 0.125f;
    acc = fmaf(ds, k[(long long)j * F + h * 64 + d], acc);
    dk_part[((long long)b * NT + j) * F + h * 64 + d] = ds * qv;
    dv_part[((long long)b * NT + j) * F + h * 64 + d] = pb[j] * dc;
  }
  dq[o] = acc;
}

// out = act(x)
__global__ void act_apply_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, int act) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = fs2_act(act, x[i]);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int fs2hip_conv2d_s2_fwd(const float* x, const float* w, float* y, int B, int H, int W, int Cin, int Cout,
                                    void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return FS2HIP_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)B * Ho * Wo * Cout;
  if (Cin == 1 && (Cout % 4) == 0 && !((uintptr_t)w % 16) && !((uintptr_t)y % 16) && total / 4 < 0x7fffffffLL * 256) {
    conv2d_s2_fwd_c1_kernel<<<dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, S_>>>(x, w, y, B, H, W, Ho, Wo, Cout);
    FS2_LAUNCH_CHECK();
    return 0;
  }
  conv2d_s2_fwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_>>>(x, w, y, B, H, W, Cin, Ho, Wo, Cout);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_conv2d_s2_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout,
                                         void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return FS2HIP_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long total = (long long)B * H * W * Cin;
  conv2d_s2_bwd_data_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_>>>(dy, w, dx, B, H, W, Cin, Ho, Wo, Cout);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_im2col_s2(const float* x, float* col, int B, int H, int W, int Cin, void* stream) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  if (Cin == 1 && B > 0 && H > 0 && W > 0 && !((uintptr_t)col % 16)) {  // col[M][12]
    long long nb = ((long long)B * Ho * Wo + 255) / 256;
    if (nb > 65535 * 16) nb = 65535 * 16;
    im2col_s2_c1_kernel<<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>(x, col, B, H, W, Ho, Wo);
    FS2_LAUNCH_CHECK();
    return 0;
  }
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 3) || ((uintptr_t)x % 16) || ((uintptr_t)col % 16)) return FS2HIP_EINVAL;
  long long blocks = ((long long)B * Ho * Wo * 9 * (Cin >> 2) + 255) / 256;
  if (blocks > 65535 * 16) blocks = 65535 * 16;
  im2col_s2_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(x, col, B, H, W, Cin, Ho, Wo);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_col2im_s2(const float* dcol, float* dx, int B, int H, int W, int Cin, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 3) || ((uintptr_t)dx % 16) || ((uintptr_t)dcol % 16)) return FS2HIP_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  long long blocks = ((long long)B * H * W * (Cin >> 2) + 255) / 256;
  if (blocks > 65535 * 16) blocks = 65535 * 16;
  col2im_s2_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(dcol, dx, B, H, W, Cin, Ho, Wo);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_conv2d_s2_wgrad_parts(int B, int H, int W) {
  const long long rows = (long long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
  return (int)((rows + CW_ROWS - 1) / CW_ROWS);
}

// partial: parts * 9*Cin*Cout floats; dw [3][3][Cin][Cout] is finished here
extern "C" int fs2hip_conv2d_s2_bwd_weight(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W,
                                           int Cin, int Cout, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return FS2HIP_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int nw = 9 * Cin * Cout, parts = fs2hip_conv2d_s2_wgrad_parts(B, H, W);
  conv2d_s2_bwd_weight_kernel<<<dim3((nw + 255) / 256, parts), dim3(256), 0, S_>>>(x, dy, partial, B, H, W, Cin, Ho, Wo, Cout);
  FS2_LAUNCH_CHECK();
  return fs2hip_reduce_slabs(partial, dw, nw, parts, nw, stream);
}

extern "C" int fs2hip_gru_gate_fwd(const float* gi, long long gi_stride, const float* gh, const float* hprev, float* hnew,
                                   float* gates, int B, int U, void* stream) {
  if (B <= 0 || U <= 0) return FS2HIP_EINVAL;
  gru_gate_fwd_kernel<<<dim3((B * U + 255) / 256), dim3(256), 0, S_>>>(gi, gi_stride, gh, hprev, hnew, gates, B, U);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gru_gate_bwd(const float* dh, const float* gates, const float* hprev, float* dgi, long long dgi_stride,
                                   float* dgh, float* dhprev, int B, int U, void* stream) {
  if (B <= 0 || U <= 0) return FS2HIP_EINVAL;
  gru_gate_bwd_kernel<<<dim3((B * U + 255) / 256), dim3(256), 0, S_>>>(dh, gates, hprev, dgi, dgi_stride, dgh, dhprev, B, U);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gru_last_state(const float* gi, const float* w_hh, const float* b_hh, const int* steps, float* h_out,
                                     int B, int T, int U, void* stream) {
  if (!gi || !w_hh || !b_hh || !steps || !h_out || B <= 0 || T <= 0 || U != GRU_U || ((uintptr_t)w_hh % 16))
    return FS2HIP_EINVAL;
  gru_last_state_kernel<<<dim3(B), dim3(3 * GRU_U), 0, S_>>>(gi, w_hh, b_hh, steps, h_out, T);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gru_fwd_states(const float* gi, const float* w_hh, const float* b_hh, const int* steps, float* hs,
                                     float* gates, float* h_out, int B, int T, int U, void* stream) {
  if (!gi || !w_hh || !b_hh || !steps || !hs || !gates || !h_out || B <= 0 || T <= 0 || U != GRU_U ||
      ((uintptr_t)w_hh % 16))
    return FS2HIP_EINVAL;
  gru_fwd_states_kernel<<<dim3(B), dim3(3 * GRU_U), 0, S_>>>(gi, w_hh, b_hh, steps, hs, gates, h_out, T);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gru_bwd_states(const float* dh_last, const float* hs, const float* gates, const float* w_hh,
                                     const int* steps, float* dgi, float* dgh, float* dh0, int B, int T, int U,
                                     void* stream) {
  if (!dh_last || !hs || !gates || !w_hh || !steps || !dgi || !dgh || !dh0 || B <= 0 || T <= 0 || U != GRU_U)
    return FS2HIP_EINVAL;
  gru_bwd_states_kernel<<<dim3(B), dim3(3 * GRU_U), 0, S_>>>(dh_last, hs, gates, w_hh, steps, dgi, dgh, dh0, T);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_conv_s2_lens(const int* lens, int* table, int B, int n, void* stream) {
  if (!lens || !table || B <= 0 || n < 0 || n > 8) return FS2HIP_EINVAL;
  conv_s2_lens_kernel<<<dim3((B + 255) / 256), dim3(256), 0, S_>>>(lens, table, B, n);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gst_attn_fwd(const float* q, const float* k, const float* v, float* p, float* ctx, int B, int NT,
                                   int heads, void* stream) {
  if (B <= 0 || NT <= 0 || NT > GST_MAX_TOKENS || heads <= 0 || heads > 4) return FS2HIP_EINVAL;
  gst_attn_fwd_kernel<<<dim3(B), dim3(256), 0, S_>>>(q, k, v, p, ctx, B, NT, heads);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_gst_attn_bwd(const float* dctx, const float* q, const float* k, const float* v, const float* p,
                                   float* dq, float* dk_part, float* dv_part, int B, int NT, int heads, void* stream) {
  if (B <= 0 || NT <= 0 || NT > GST_MAX_TOKENS || heads <= 0 || heads > 4) return FS2HIP_EINVAL;
  gst_attn_bwd_kernel<<<dim3(B), dim3(256), 0, S_>>>(dctx, q, k, v, p, dq, dk_part, dv_part, B, NT, heads);
  FS2_LAUNCH_CHECK();
  return 0;
}

extern "C" int fs2hip_act_apply(const float* x, float* out, long long n, int act, void* stream) {
  if (n <= 0) return FS2HIP_EINVAL;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  act_apply_kernel<<<dim3((unsigned)blocks), dim3(256), 0, S_>>>(x, out, n, act);
  FS2_LAUNCH_CHECK();
  return 0;
}
