// Second-generation fp32 attention kernels for head dims 64 / 128 (the Conformer's 2 x 128): see attention2.hip.
#pragma once
#include "common.h"

struct Attn2Args {
  const float* qkv;   // [B*T][3*D]: q | k | v
  const int* lens;    // [B] valid keys per utterance
  int B, T, H, HD;
  float scale;        // 1/sqrt(HD)
  Fs2Drop drop;       // dropout on the attention probabilities, element index ((b*H + h)*T + q)*Tp + key, Tp = T rounded up to even
  int planes;         // 0: fp32 MFMA.  1: operands rounded to bf16 ("bf16-mixed").  3: three exact bf16 planes ("32-split")
  long long* stamps;  // diagnostic builds only (-DFS2_ATTN_STAMPS, tools/probes/attn2_probe.hip): per-phase cycle sums
};

// Host-side bounds and grid shared by the launchers of both kernel families.
// The dropout element index is 32 bits wide; the mask's rows are padded to an even length (one hash serves two neighbouring
// keys), so the index stride is T + (T & 1) -- the same bound in every forward and backward launcher.
inline bool fs2_attn_drop_index_ok(const Attn2Args& a) {
  return (double)a.B * a.H * a.T * (a.T + (a.T & 1)) < 4294967296.0;
}
// One (utterance, head) slab of kept scores or spilled dS -- T rows of T rounded up to 32 elements -- per buffer resource.
inline bool fs2_attn_slab_ok(int T, size_t elem_bytes) {
  return (long long)T * ((T + 31) & ~31) * (long long)elem_bytes < 0x7fffffffLL;
}
// One workgroup per (block of `rows` query or key rows, head, utterance).
inline dim3 fs2_attn_grid(const Attn2Args& a, int rows = 64) { return dim3(((a.T + rows - 1) / rows) * a.H * a.B); }

// true when the second-generation kernels take the shape (HD in {64, 128}; operand_bf16: 0 fp32, 1 bf16, 2 split)
bool fs2_attn2_supported(int HD, int operand_bf16);
// s_out (fp32 MFMA path, may be null): the masked scores for fs2_attn2_bwd_spill's s_in, B * H * T * (T rounded up to 32) floats
int fs2_attn2_fwd(const Attn2Args& a, float* o, float* lse, hipStream_t s, float* s_out = nullptr);
int fs2_attn2_bwd(const Attn2Args& a, const float* o, const float* dout, const float* lse, float* delta, float* dqkv,
                  hipStream_t s);

// the same backward pass with dS spilled by the dK/dV kernel and dQ = scale * dS . K as a product of its own (fp32 MFMA
// path); `ds` holds fs2_attn2_bwd_spill_elems(a) floats (0: this shape / operand mode does not take the path)
long long fs2_attn2_bwd_spill_elems(const Attn2Args& a);
int fs2_attn2_bwd_spill(const Attn2Args& a, const float* o, const float* dout, const float* lse, float* aux, float* ds,
                        float* dqkv, hipStream_t s, const float* s_in = nullptr);

// bf16-storage family (attention_bf16.hip): qkv / o / dout / dqkv are bf16 tensors of the same shapes; `a.qkv` is unused
bool fs2_attnb_supported(int HD);
int fs2_attnb_fwd(const Attn2Args& a, const void* qkv, void* o, float* lse, hipStream_t s);
int fs2_attnb_bwd(const Attn2Args& a, const void* qkv, const void* o, const void* dout, const float* lse, float* aux,
                  void* dqkv, hipStream_t s, void* ds = nullptr);
