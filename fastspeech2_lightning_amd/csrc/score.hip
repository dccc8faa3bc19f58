// Per-utterance loss scores (fs2hip_utterance_losses): what FastSpeech2Loss (fs2/loss.py:19-126) gives for the batch of
// ONE made of utterance b cut to its own lengths, for every utterance of a teacher-forced batch at once -- the table the
// reference's ScorerCallback (fs2/prediction_writing_callback.py:138-211) fills at batch size 1.
//
// A segmented reduction: utterance b's valid region of a term is the contiguous range of len_b * C floats at b * T * C.
// One workgroup owns one (utterance, term) pair and walks that range in passes; nothing is shared between workgroups, so
// there are no atomics and no workspace.  The order of the additions is a function of n = len_b * C alone:
//   - logical elements 4q .. 4q + 3 form quad q, whose value is (f0 + f1) + (f2 + f3) (missing elements of the last quad
//     count as +0);
//   - thread i adds the quads i, i + 512, i + 1024, ... to its accumulator in that order;
//   - the 512 accumulators are folded by the xor butterfly inside each wavefront and the eight wavefront sums are added
//     in wavefront order.
// B, T, the utterance's place in the batch and the alignment of its base address do not enter: a quad is fetched with
// 16-byte loads when the utterance's base is 16-byte aligned and element by element otherwise, into the same registers,
// and the arithmetic behind the loads is one function compiled without contraction.  A row of a batch is therefore
// bit-equal to the same data scored as a batch of one.
// HBM-bound and small (a 700-frame, 80-band utterance is 55 passes of one workgroup); SC_UNROLL quads per thread are in
// flight so that a lone workgroup still keeps a few dozen KiB of loads outstanding.
#include "common.h"

// no a * b + c becomes an fma below: both load paths, and a test's fp32 sum of the columns, must meet the same roundings
#pragma clang fp contract(off)

namespace {

constexpr int SC_THREADS = 512;
constexpr int SC_WAVES = SC_THREADS / FS2_WAVE;
constexpr int SC_UNROLL = 4;
constexpr int SC_COLS = FS2_SCORE_COLUMNS;
constexpr int SC_COL_CTC = 5, SC_COL_BIN = 6, SC_COL_TOTAL = 7;

struct ScoreTable {
  Fs2ScoreMember m[FS2_SCORE_MAX_MEMBERS];
  int n;
  int Tm, Ts;
  float bin_weight;
  const float* soft;  // null: no binarisation term
  const int* hard_idx;
  const int* mel_lens;
};

__device__ __forceinline__ int sc_clamp_len(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

// pred and target of quad q (elements e = 4q .. 4q + 3 of the utterance's range) as far as they exist; the rest stays 0
__device__ __forceinline__ void sc_fetch(const float* __restrict__ p, const float* __restrict__ t,
                                         const int* __restrict__ ti, long long e, long long n, bool vec, float (&pv)[4],
                                         float (&tv)[4]) {
  if (vec && e + 4 <= n) {
    const float4 a = *reinterpret_cast<const float4*>(p + e);
    pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
    if (ti) {
      const int4 c = *reinterpret_cast<const int4*>(ti + e);
      tv[0] = logf((float)c.x + 1.f); tv[1] = logf((float)c.y + 1.f);
      tv[2] = logf((float)c.z + 1.f); tv[3] = logf((float)c.w + 1.f);
    } else {
      const float4 c = *reinterpret_cast<const float4*>(t + e);
      tv[0] = c.x; tv[1] = c.y; tv[2] = c.z; tv[3] = c.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pv[k] = 0.f;
      tv[k] = 0.f;
      if (e + k < n) {
        pv[k] = p[e + k];
        tv[k] = ti ? logf((float)ti[e + k] + 1.f) : t[e + k];
      }
    }
  }
}

// acc + the quad's value; the one place where a term's arithmetic lives (see the head of the file)
__device__ __forceinline__ float sc_add_quad(float acc, const float (&pv)[4], const float (&tv)[4], int kind) {
  float f[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = pv[k] - tv[k];
    f[k] = kind == 0 ? d * d : fabsf(d);
  }
  const float lo = f[0] + f[1], hi = f[2] + f[3];
  const float v = lo + hi;
  return acc + v;
}

// every thread's v -> the workgroup's sum, valid in thread 0
__device__ __forceinline__ float sc_block_sum(float v, float* red) {
  v = fs2_wave_sum(v);
  __syncthreads();  // (red may still be read from a previous call)
  if ((threadIdx.x & (FS2_WAVE - 1)) == 0) red[threadIdx.x / FS2_WAVE] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < SC_WAVES; ++w) s = s + red[w];
  return s;
}

// blockIdx.x = utterance, blockIdx.y = member (tab.n = the binarisation term).  Writes scores[b][column].
__global__ __launch_bounds__(SC_THREADS) void score_terms_kernel(const ScoreTable tab, float* __restrict__ scores) {
  __shared__ float red[SC_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* row = scores + (long long)b * SC_COLS;
  if ((int)blockIdx.y >= tab.n) {
    // fs2/attn/attention_loss.py:65-73 on the utterance's own box: one entry per frame below the length
    const int len = sc_clamp_len(tab.mel_lens[b], tab.Tm);
    const int* __restrict__ hi = tab.hard_idx + (long long)b * tab.Tm;
    const float* __restrict__ soft = tab.soft + (long long)b * tab.Tm * tab.Ts;
    float s = 0.f, cnt = 0.f;
    for (int t = tid; t < len; t += SC_THREADS) {
      const int j = hi[t];
      if (j >= 0 && j < tab.Ts) {
        s = s + logf(fmaxf(soft[(long long)t * tab.Ts + j], 1e-12f));
        cnt = cnt + 1.f;
      }
    }
    s = sc_block_sum(s, red);
    cnt = sc_block_sum(cnt, red);
    if (tid == 0) row[SC_COL_BIN] = cnt > 0.f ? -tab.bin_weight * (s / cnt) : 0.f;
    return;
  }
  const Fs2ScoreMember& m = tab.m[blockIdx.y];
  const int len = sc_clamp_len(m.lens[b], m.T);
  const long long n = (long long)len * m.C, base = (long long)b * m.T * m.C;
  const float* __restrict__ p = m.pred + base;
  const float* __restrict__ t = m.tgt_int ? nullptr : m.tgt + base;
  const int* __restrict__ ti = m.tgt_int ? m.tgt_int + base : nullptr;
  const bool vec = ((((uintptr_t)p) | (ti ? (uintptr_t)ti : (uintptr_t)t)) & 15) == 0;
  const long long quads = (n + 3) >> 2;
  const int kind = m.kind;
  float acc = 0.f;
  long long q = tid;
  for (; q + (long long)(SC_UNROLL - 1) * SC_THREADS < quads; q += (long long)SC_UNROLL * SC_THREADS) {
    float pv[SC_UNROLL][4], tv[SC_UNROLL][4];
#pragma unroll
    for (int u = 0; u < SC_UNROLL; ++u) sc_fetch(p, t, ti, (q + (long long)u * SC_THREADS) * 4, n, vec, pv[u], tv[u]);
#pragma unroll
    for (int u = 0; u < SC_UNROLL; ++u) acc = sc_add_quad(acc, pv[u], tv[u], kind);
  }
  for (; q < quads; q += SC_THREADS) {
    float pv[4], tv[4];
    sc_fetch(p, t, ti, q * 4, n, vec, pv, tv);
    acc = sc_add_quad(acc, pv, tv, kind);
  }
  const float s = sc_block_sum(acc, red);
  if (tid == 0) row[m.column] = n > 0 ? m.weight * (s / (float)n) : 0.f;
}

// One thread per utterance: the columns no workgroup of the first launch wrote (attn_ctc from nll, zeros) and the total,
// the present columns added in LOSS_KEYS order (fs2hip_sum_slots' order, fs2/loss.py:125).
__global__ __launch_bounds__(256) void score_finish_kernel(float* __restrict__ scores, const float* __restrict__ nll,
                                                            float ctc_weight, unsigned written, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float* row = scores + (long long)b * SC_COLS;
  float total = 0.f;
#pragma unroll
  for (int c = 0; c < SC_COL_TOTAL; ++c) {
    float v;
    if (written & (1u << c)) {
      v = row[c];
    } else {
      v = 0.f;
      if (c == SC_COL_CTC && nll) v = ctc_weight * nll[b];
      row[c] = v;
    }
    total = total + v;
  }
  row[SC_COL_TOTAL] = total;
}

}  // namespace

extern "C" int fs2hip_utterance_losses(const Fs2ScoreMember* members, int n, const float* soft, const int* hard_idx,
                                       const int* mel_lens, int Tm, int Ts, float bin_weight, const float* nll,
                                       float ctc_weight, float* scores, int B, void* stream) {
  if (!scores || B <= 0 || n < 0 || n > FS2_SCORE_MAX_MEMBERS || (n > 0 && !members)) return FS2HIP_EINVAL;
  ScoreTable tab = {};
  unsigned written = 0;
  for (int i = 0; i < n; ++i) {
    const Fs2ScoreMember& a = members[i];
    if (!a.pred || !a.lens || (!a.tgt && !a.tgt_int)) return FS2HIP_EINVAL;
    if (a.T <= 0 || a.C <= 0 || (a.kind != 0 && a.kind != 1)) return FS2HIP_EINVAL;
    if (a.column < 0 || a.column >= SC_COL_TOTAL || (written & (1u << a.column))) return FS2HIP_EINVAL;
    written |= 1u << a.column;
    tab.m[i] = a;
  }
  tab.n = n;
  const bool bin = soft || hard_idx;
  if (bin) {
    if (!soft || !hard_idx || !mel_lens || Tm <= 0 || Ts <= 0) return FS2HIP_EINVAL;
    if (written & (1u << SC_COL_BIN)) return FS2HIP_EINVAL;
    written |= 1u << SC_COL_BIN;
    tab.soft = soft;
    tab.hard_idx = hard_idx;
    tab.mel_lens = mel_lens;
    tab.Tm = Tm;
    tab.Ts = Ts;
    tab.bin_weight = bin_weight;
  }
  if (nll && (written & (1u << SC_COL_CTC))) return FS2HIP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int terms = n + (bin ? 1 : 0);
  if (terms > 0) {
    score_terms_kernel<<<dim3((unsigned)B, (unsigned)terms), dim3(SC_THREADS), 0, s>>>(tab, scores);
    FS2_LAUNCH_CHECK();
  }
  score_finish_kernel<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s>>>(scores, nll, ctc_weight, written, B);
  FS2_LAUNCH_CHECK();
  return 0;
}
