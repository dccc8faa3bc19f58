/* fs2hip -- C ABI of the MI355X (gfx950) kernels behind the FastSpeech2
 * feature-prediction path.
 *
 * The reference (EveryVoiceTTS/FastSpeech2_lightning) has no FFI: its device work
 * is ATen ops called from Python modules.  Each entry point below names the
 * reference call site(s) (file:line, relative to the reference checkout) whose
 * ATen ops it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Dropout: element i keeps iff its 16-bit field (even i: low half, odd i: high half) of
 * hash32(mix64(seed + *drop_step * 0xD1B54A32D192ED03), i >> 1) >= (uint32)(p * 65536 + 0.5), and is then scaled by
 * 1/(1-p) in fp32; mix64 is the splitmix64 finaliser (applied with or without a counter), hash32 the two-round 32-bit
 * mixer fs2_hash32 (csrc/common.h).  tests/layernorm_references.py restates the rule on the host and
 * tests/test_layernorm_gpu.py holds the kernels to it.  The mask is regenerated (never stored) by the backward
 * kernels; `drop_step` is a device-resident counter so that a captured hipGraph draws a fresh mask on every replay.
 *
 * Conventions (all entry points):
 *   - raw device pointers into caller-owned dense row-major buffers; activations
 *     are (B, T, C) = matrices of B*T rows and C contiguous columns, fp32;
 *   - no allocation, no host synchronisation, no global state: everything is
 *     enqueued on `stream` (a hipStream_t passed as void*);
 *   - workspaces are caller-provided;
 *   - return value: 0 on success, otherwise the hipError_t of the launch, or
 *     FS2HIP_EINVAL (-22) when the arguments fail the host-side shape checks.
 */
#ifndef FS2HIP_H
#define FS2HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS2HIP_EINVAL (-22)

/* activation codes */
enum { FS2_ACT_NONE = 0, FS2_ACT_RELU = 1, FS2_ACT_SILU = 2, FS2_ACT_TANH = 3 };

/* GEMM epilogues (v = alpha * acc + bias[n]) */
enum {
  FS2_EPI_STORE = 0, /* C = v                                                         */
  FS2_EPI_ACT = 1,   /* out_pre = v (optional); C = dropout(act(v))                   */
  FS2_EPI_RESID = 2, /* C = resid + res_scale * dropout(v)                            */
  FS2_EPI_DACT = 3   /* C = v * act'(aux) * dropmask   (backward through ACT)         */
};

int fs2hip_version(void); /* 2 since attention has one forward and one backward entry point per family */

/* ------------------------------------------------------------------------------------
 * GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32; bf16 operands on request):  C[Mc][Nc] = epi( sum_r A(m,r) * B(r,n) )
 *
 * Replaces every nn.Linear / pointwise nn.Conv1d / k-tap nn.Conv1d contraction on the
 * path, forward and backward:
 *   torchaudio Conformer FFN / in_proj / out_proj / pointwise convs (call sites
 *   fs2/model.py:193, :241), fs2/blocks.py:14-16 (pointwise), fs2/layers.py:30-38 (k-tap
 *   conv of the variance predictors), fs2/layers.py:204-212 (PostNet convs),
 *   fs2/attn/attention.py:220-227 (aligner projections), fs2/model.py:244 (mel_linear).
 *
 *   a_kcontig = 1: A stored [Mc][R] (lda)      0: A stored [R][Mc] (lda)
 *   b_kcontig = 1: B stored [Nc][R] (ldb)      0: B stored [R][Nc] (ldb)
 *   Conv taps (rows are (b, t), t = row % T):
 *     shift_operand = 0: R = taps * Rper; reduction step (tap, k) reads A row m + s(tap)
 *                        (zero when t + s(tap) is outside [0, T)) and B + tap*b_tap_stride;
 *                        A must be a_kcontig with Rper columns.
 *     shift_operand = 1: (weight gradient) one launch per tap j = blockIdx.z / splitk:
 *                        B row r + s(j) (zero outside), C + j*c_tap_stride.
 *     s(tap) = tap * tap_mul + tap_add.
 *   splitk > 1 (only with a_kcontig = b_kcontig = 0): R is cut in `splitk` chunks, partial
 *     tiles go to workspace[split][taps][Mc*Nc].  With `counters` == NULL fs2hip_reduce_slabs finishes; with
 *     `counters` (FS2_SPLITK_COUNTERS zero-initialised ints, one set per stream that runs split GEMMs) the workgroup
 *     that delivers the LAST slab of an output tile sums the tile's slabs in slab order (the same sum, bit for bit) and
 *     writes C itself, then re-arms the tile's counter: no second launch.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  const float* A;
  const float* B;
  float* C;
  int Mc, Nc, R;
  int lda, ldb, ldc;
  int a_kcontig, b_kcontig;
  int taps, T, tap_mul, tap_add, shift_operand;
  long long b_tap_stride, c_tap_stride;
  const float* bias;
  int epi, act;
  float alpha;
  const float* resid;
  int ldr;
  float res_scale;
  const float* aux;
  int ldaux;
  float* out_pre;
  int ldpre;
  float drop_p;
  unsigned long long drop_seed;
  const unsigned long long* drop_step; /* device step counter mixed into the seed, or NULL */
  int splitk;
  float* workspace;
  int tile; /* 0 = heuristic; workgroup tile chosen by the host autotuner: 1/2/3 = 128x128, 128x64, 64x64 on the
               register-staged BK=16 core, 4..9 = direct-to-LDS BK=32 core (128x128, 128x64, 64x64 with a 3/3/4-stage LDS
               ring; 7/8/9 = 64x64, 128x64, 128x128 with 2 stages and more workgroups per CU), 10/11/12 = persistent
               64x64, 128x64, 128x128, 13/14/15 = persistent 128x128, 128x64, 64x64 whose last partial round of tiles
               is cut along the reduction and finished (sum + the same epilogue) by a second pass (needs `workspace`) */
  long long workspace_floats; /* capacity of `workspace` */
  int* counters; /* splitk > 1: per-output-tile arrival counters (see above), or NULL */
  int operand_bf16; /* 0: fp32 MFMA (the default, the parity path).  1: "bf16-mixed" -- A and B stay fp32 in memory and
                       in LDS, are rounded to bf16 (RNE) in registers and multiplied with v_mfma_f32_32x32x16_bf16;
                       accumulation, bias/epilogue and C stay fp32.  2: "32-split" -- fp32 accuracy on the bf16 pipe:
                       every operand value is cut exactly into three bf16 planes in registers (x = x0 + x1 + x2) and a
                       product is the six partial products a_i b_j with i + j <= 2, accumulated in fp32, smallest first
                       (what is dropped is below the rounding of the fp32 product): the error bound of mode 0 at
                       2.7x its matrix-pipe rate.  Only the direct-to-LDS cores (tile >= 4) carry modes 1 and 2;
                       shapes those cores refuse run in fp32.  3: bf16 operand STORAGE -- A and B point to bf16
                       (k-contiguous rows: a_kcontig = b_kcontig = 1; lda, ldb, R, b_tap_stride in bf16 elements, all
                       multiples of 8, tap widths multiples of 64; no split-K), C, bias and the epilogue tensors stay
                       fp32; tiles 4..9.  4: the bf16-storage core (gemm_bf16.hip, gemm_bf16p.hip; tiles 20, 22..25) -- A and B point to bf16 in
                       ANY of the three orientations (forward a_kcontig = b_kcontig = 1; data gradient a_kcontig = 1 with
                       the weight as stored, b_kcontig = 0; weight gradient both 0, split-K allowed), lda / ldb / R /
                       b_tap_stride / c_tap_stride in elements; R, lda, ldb multiples of 8, the row count of a
                       reduction-major operand a multiple of 8, Nc and ldc multiples of 4; tap widths multiples of 64
                       (shift_operand = 0) / T >= 64 (shift_operand = 1); bias, resid and split-K slabs fp32 */
  int io_bf16;   /* operand_bf16 == 4 only.  bit 0: C and out_pre are bf16 (ldc / ldpre in elements; the activation of
                    FS2_EPI_ACT is applied to the ROUNDED pre-activation, i.e. to what the backward pass reads back);
                    bit 1: aux is bf16 */
  float* colsum; /* weight gradient (a_kcontig = b_kcontig = 0) only, or NULL: receives the column sums of A over the
                    reduction -- the bias gradient dY^T . 1 of the layer whose weight gradient this launch computes -- as
                    colsum[split][Mc] partial sums (splitk rows; the caller adds them).  Direct-to-LDS cores (tiles 4..12)
                    and the bf16-storage core */
} Fs2GemmArgs;
#define FS2_SPLITK_COUNTERS 4096

int fs2hip_gemm(const Fs2GemmArgs* args, void* stream);

/* Up to FS2_GEMM_GROUP_MAX independent GEMMs in ONE launch: args[0 .. n) as for fs2hip_gemm, each with its own shapes,
 * pointers, split-K and epilogue.  Replaces runs of small launches that leave most of the chip idle one at a time: the
 * three variance predictors' pointwise convolutions of one layer (independent in a training step -- their inputs add
 * TARGET embeddings, fs2/variance_adaptor.py:309-352 -- forward, data and weight gradients; fs2/blocks.py:14-16) and the
 * eight weight gradients of one encoder Conformer layer (fs2/model.py:95-107: B x Ts rows, a quarter of a CU round each).
 * Every member computes exactly what fs2hip_gemm would (the member's workgroups run the same tile code on the member's own
 * arguments: same bits).  Members must share one kernel instance: the same operand orientations (a_kcontig, b_kcontig)
 * and operand_bf16 in {0, 4}, taps == 1, counters == NULL, drop_p == 0; `tile` (args[0].tile) is 0 or one of 7 / 8 (fp32)
 * and 22 / 23 / 26 (bf16 storage), the other members' `tile` is ignored.  n == 1 is fs2hip_gemm.  FS2HIP_EINVAL: the
 * members cannot share a launch (the caller launches them one by one); nothing has been enqueued then. */
#define FS2_GEMM_GROUP_MAX 8
int fs2hip_gemm_grouped(const Fs2GemmArgs* args, int n, void* stream);

/* Several row reductions in one launch: out0[c] (c < n0) / out1[c - n0] = sum over `rows` rows of src[r * stride + c],
 * c < n.  Finishes the partial sums of fs2hip_colsum (out == NULL) and fs2hip_layernorm_bwd (dgamma == dbeta == NULL),
 * i.e. the bias and LayerNorm parameter gradients (torch autograd's sum-to-size in the reference), whose only
 * consumer is the optimizer: the host batches them.  njobs <= FS2_REDUCE_MAX_JOBS. */
#define FS2_REDUCE_MAX_JOBS 48
typedef struct {
  const float* src;
  float* out0;
  float* out1;
  long long stride;
  int rows, n, n0, pad_;
} Fs2ReduceJob;
int fs2hip_reduce_rows_multi(const Fs2ReduceJob* jobs, int njobs, void* stream);

/* out[i] = sum_s slabs[s*slab_stride + i], i < n  (split-K / partial-sum finish) */
int fs2hip_reduce_slabs(const float* slabs, float* out, long long n, int nslabs,
                        long long slab_stride, void* stream);

/* The same for up to FS2_REDUCE_MAX_JOBS independent slab sets in one launch (the split-K finishes of
 * a whole backward pass: weight gradients are only read by the optimizer, fs2/model.py:530-549 via
 * Lightning's optimizer step).  `vec` is set by the library. */
typedef struct {
  const float* slabs;
  float* out;
  long long n, stride;
  int nslabs, vec;
} Fs2SlabJob;
int fs2hip_reduce_slabs_multi(const Fs2SlabJob* jobs, int njobs, void* stream);

/* column sums of a [M][N] matrix (bias gradients): partial[gy][N] then reduce_slabs.
 * partial must hold fs2hip_colsum_rows(M) * N floats. */
int fs2hip_colsum_rows(int M);
int fs2hip_colsum(const float* x, int ldx, int M, int N, float* partial, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the last dim (C <= 1024, C % 4 == 0), one wavefront per row.
 * nn.LayerNorm sites: Conformer (ffn/self_attn/conv/final norms), fs2/layers.py:43.
 * fwd: y = (x-mean)*rstd*gamma+beta, saves mean/rstd [M].
 * bwd: dx (+= dx_add if given), partial dgamma/dbeta -> [nblk][2][C] then reduce.
 * ------------------------------------------------------------------------------------ */
int fs2hip_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                         float* mean, float* rstd, int M, int C, float eps, void* stream);
int fs2hip_layernorm_bwd_blocks(int M);
int fs2hip_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, const float* dx_add, float* dx, float* partial,
                         float* dgamma, float* dbeta, int M, int C, void* stream);
/* The same with a second output for the sub-module below in the backward order (every Conformer sub-module is
 * x + scale * Dropout(f(LayerNorm(x))), torchaudio conformer.py; call sites fs2/model.py:95-119): dz = dz_scale *
 * dropmask * dx with the mask of that sub-module's output dropout (element index row * C + c, as fs2hip_axpby draws
 * it), and its column sums -- the gradient of f's last bias.  partial is [fs2hip_layernorm_bwd_blocks(M)][3][C]:
 * rows of dgamma | dbeta | colsum(dz) partial sums, finished by fs2hip_reduce_rows_multi. */
int fs2hip_layernorm_bwd_dz(const float* dy, const float* x, const float* gamma, const float* mean,
                            const float* rstd, const float* dx_add, float* dx, float* dz, float dz_scale,
                            float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                            float* partial, int M, int C, void* stream);
/* The variance predictors' Conv -> ReLU -> LayerNorm -> Dropout layers (fs2/layers.py:30-48, five per predictor, three
 * predictors: fs2/variance_adaptor.py:18-62) in two launches instead of five:
 *   fwd_drop: y = dropout(LayerNorm(x)) (mask at element index row * C + c, as fs2hip_axpby draws it over y);
 *   bwd_pred: dx = relu'(x) . LayerNormBackward(dropmask . dy) with x = the ReLU output the LayerNorm normalised
 *             (relu' = (x > 0)); partial is [fs2hip_layernorm_bwd_blocks(M)][2][C] (dgamma | dbeta partial sums). */
int fs2hip_layernorm_fwd_drop(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                              float* rstd, int M, int C, float eps, float drop_p, unsigned long long drop_seed,
                              const unsigned long long* drop_step, void* stream);
/* dx_bf16 != 0: dx is written as bf16 (bf16 operand storage: the layer's weight- and data-gradient GEMMs read it) */
int fs2hip_layernorm_bwd_pred(const float* dy, const float* x, const float* gamma, const float* mean,
                              const float* rstd, void* dx, int dx_bf16, float* partial, int M, int C, float drop_p,
                              unsigned long long drop_seed, const unsigned long long* drop_step, void* stream);
/* bf16 on either side of a LayerNorm ("bf16-mixed" with bf16 activation storage: the normalised activations and the
 * gradients between GEMMs exist only as the bf16 operands those GEMMs read).
 *   fwd_b: y is bf16.
 *   bwd_x: flags bit 0: dy is bf16 (the result of a data-gradient GEMM); bit 1: dz is bf16.  dz == NULL: no second
 *          output and partial is [nblk][2][C]; else [nblk][3][C] (the column sums are those of the rounded dz).
 *          dx_add, dx stay fp32 (the residual stream).  The caller finishes the partial sums. */
int fs2hip_layernorm_fwd_b(const float* x, const float* gamma, const float* beta, void* y_bf16,
                           float* mean, float* rstd, int M, int C, float eps, void* stream);
int fs2hip_layernorm_bwd_x(const void* dy, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dx_add, float* dx, void* dz, float dz_scale,
                           float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                           float* partial, int M, int C, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-head self-attention with key-padding mask (flash style; fp32 MFMA: v_mfma_f32_32x32x2_f32 for
 * head dims 64 / 128 -- attention2.hip -- and 16x16x4 for head dims 16 / 32 / 256).
 * Replaces nn.MultiheadAttention's scaled-dot-product core inside torchaudio's
 * ConformerLayer (call sites fs2/model.py:193, :241).
 *
 * Any head dimension 1 <= HD <= 256.  The tensors are laid out, and the kernels run, at the padded width
 * HDp = fs2hip_attention_padded_dim(HD): the smallest of 16, 32, 64, 128, 256 that holds HD (0: refused) -- HD itself at
 * those five; the softmax scale is 1/sqrt(HD) of the TRUE head dimension.
 *   qkv  [B*T][3*H*HDp]  in_proj output (q | k | v);  lens [B] int32 (keys >= lens[b] masked)
 *   o, dout [B*T][H*HDp];  lse [B][H][T] (log-sum-exp per query, saved for the backward);  dqkv [B*T][3*H*HDp], fully written
 *   dropout acts on the normalised probabilities (attention dropout), mask regenerated from (seed, b, h, q, k) in the
 *   backward: it does not depend on the head width.
 * fs2hip_attention_pad_heads: [rows][groups*HD] -> [rows][groups*HDp], the pad columns written as zeros (qkv: groups = 3H;
 *   dout and o: groups = H).  fs2hip_attention_unpad_heads: [rows][groups*HDp] -> [rows][groups*HD] (o, dqkv).  Zero columns
 *   of Q and K add exact zeros to every score and zero columns of V give zero output columns, so the results on the padded
 *   tensors are those of the true head dimension.
 * operand_bf16 = 1 ("bf16-mixed"): the operands of all five products (Q, K, V, dO, P, dS) are rounded to bf16 for
 *   v_mfma_f32_16x16x32_bf16; scores, softmax statistics, accumulators and outputs stay fp32.  2 ("32-split"): three exact
 *   bf16 planes for the forward and dQ products.
 * fwd:
 *   scores (optional): when non-null the masked scores (log2 units, scale folded in, -inf at masked keys) are also written
 *     there, kept by the caller until the backward pass.  At least B*H*T*(T rounded up to 32) floats (score_floats = its
 *     size); operand_bf16 0 or 2, HDp 64 / 128.
 * bwd:
 *   aux: scratch of 2*B*H*T + 4 floats ({lse', delta'} pairs per row and head).
 *   ds (optional): non-null selects the backward with dS written out by the dK/dV kernel and dQ = scale * dS . K as a
 *     product of its own -- 5 products per block instead of the 9 of two kernels that each recompute S and dP (DESIGN.md
 *     section 4a).  Scratch of at least B*H*T*(T rounded up to 32) floats (ds_floats = its size); operand_bf16 0 or 2
 *     (the dK/dV kernel is the fp32 one either way), HDp for which fs2hip_attention_bwd_spill_supported() returns 1
 *     (64, 128).  Same results as with ds null up to the rounding of S (the scale is folded into K there, into Q in the
 *     recomputing dQ kernel).
 *   scores (optional, only with ds): the forward pass's; the dK/dV kernel reads them instead of recomputing K.Q^T -- 3 + 1
 *     products per block, and the backward's probabilities are the forward's to the bit.
 * ------------------------------------------------------------------------------------ */
int fs2hip_attention_padded_dim(int HD);
int fs2hip_attention_pad_heads(const float* src, float* dst, int rows, int groups, int HD, int HDp, void* stream);
int fs2hip_attention_unpad_heads(const float* src, float* dst, int rows, int groups, int HDp, int HD, void* stream);
int fs2hip_attention_bwd_spill_supported(int HD);
int fs2hip_attention_fwd(const float* qkv, const int* lens, float* o, float* lse, float* scores,
                         long long score_floats, int B, int T, int H, int HD, float drop_p,
                         unsigned long long drop_seed, const unsigned long long* drop_step, int operand_bf16,
                         void* stream);
int fs2hip_attention_bwd(const float* qkv, const int* lens, const float* o, const float* dout,
                         const float* lse, const float* scores, float* aux, float* ds, long long ds_floats,
                         float* dqkv, int B, int T, int H, int HD, float drop_p, unsigned long long drop_seed,
                         const unsigned long long* drop_step, int operand_bf16, void* stream);

/* The same attention on tensors that ARE bf16 in memory (precision "bf16-mixed" with bf16 activation
 * storage; torch.autocast(bfloat16) around nn.MultiheadAttention, call sites fs2/model.py:193, :241):
 * qkv, o, dout, dqkv are bf16 with the shapes above, lse and the scratch `aux` (2*B*H*T + 4 floats)
 * are fp32.  Head dims for which fs2hip_attention_b_supported() returns 1 (128).  The dropout keep
 * mask is the one fs2hip_attention_fwd generates for the same (drop_p, drop_seed, drop_step).
 *   ds (optional): non-null selects the backward with dS -- masked and rounded to bf16: the operand the dQ product
 *     consumes -- written out by the dK/dV kernel and dQ = scale * dS . K as a product of its own: S, dP and the softmax /
 *     dropout arithmetic are computed once per backward pass instead of twice.  Scratch of at least B*H*T*(T rounded up
 *     to 32) bf16 elements (ds_elems = its size, read only when ds is non-null). */
int fs2hip_attention_b_supported(int HD);
int fs2hip_attention_fwd_b(const void* qkv, const int* lens, void* o, float* lse, int B, int T, int H,
                           int HD, float drop_p, unsigned long long drop_seed,
                           const unsigned long long* drop_step, void* stream);
int fs2hip_attention_bwd_b(const void* qkv, const int* lens, const void* o, const void* dout,
                           const float* lse, float* aux, void* ds, long long ds_elems, void* dqkv,
                           int B, int T, int H, int HD, float drop_p, unsigned long long drop_seed,
                           const unsigned long long* drop_step, void* stream);

/* ------------------------------------------------------------------------------------
 * Depthwise Conv1d over time on (B, T, C), 'same' padding, K in {3,5,7,9,15,31}; w is [K][C].
 * glu = 1: the input has 2C columns (value | gate) and a = value * sigmoid(gate) is formed on
 * the fly (torchaudio conv module: Conv1d(D,2D,1) -> GLU -> depthwise Conv1d).
 * stats = 1: also writes per-workgroup (mean, sum of squared deviations) per channel for BatchNorm:
 *            partial[fs2hip_dwconv_blocks(B,T)][2][C]; a workgroup covers fs2hip_dwconv_part_rows()
 *            time steps of one utterance (bn_finalize: part_rows = that, group_rows = T).
 * Also the depthwise half of fs2/blocks.py:8-13.
 * bwd: dx has the layout of x; partial [blocks][K+1][C]; dw [K][C] and dbias [C] are finished.
 * ------------------------------------------------------------------------------------ */
int fs2hip_dwconv_blocks(int B, int T);
int fs2hip_dwconv_part_rows(void);
int fs2hip_dwconv_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, float* partial,
                      int B, int T, int C, int K, int glu, int stats, void* stream);
int fs2hip_dwconv_bwd(const float* dy, const float* x, int ldx, const float* w, float* dx, float* partial,
                      float* dw, float* dbias, int B, int T, int C, int K, int glu, void* stream);
/* bf16 tensors (precision "bf16-mixed" with bf16 activation storage; what torch.autocast hands the convolution
 * module of torchaudio's ConformerLayer, call sites fs2/model.py:193, :241), GLU form only:
 *   fwd_b, io_bf16 = 1: x and y are bf16 (the BatchNorm statistics are those of the rounded y);
 *          io_bf16 = 2: x fp32, y bf16, plain (non-GLU) form without statistics -- the variance predictors' depthwise
 *          layer (fs2/blocks.py:4-19) feeding its pointwise GEMM's bf16 operand;
 *   bwd_b, dx_bf16 bit 0: dx is written as bf16 (layout and leading dimension of x); bit 1: dy and x are bf16. */
int fs2hip_dwconv_fwd_b(const void* x, int ldx, const float* w, const float* bias, void* y, float* partial,
                        int B, int T, int C, int K, int glu, int stats, int io_bf16, void* stream);
int fs2hip_dwconv_bwd_b(const void* dy, const void* x, int ldx, const float* w, void* dx, int dx_bf16, float* partial,
                        float* dw, float* dbias, int B, int T, int C, int K, int glu, void* stream);

/* ------------------------------------------------------------------------------------
 * BatchNorm1d over the channels of [M][C] (+ activation + dropout), fs2/layers.py:204-212 and
 * the Conformer conv module.  stats is [5][C]: scale, shift, mean, invstd, eps.
 *   colstats   : partial[fs2hip_colstats_parts(M)][2][C] = per-stripe (mean, sum of squared
 *                deviations) over stripes of fs2hip_colstats_part_rows(M) rows, accumulated on
 *                pivot-shifted values (torch's BatchNorm is Welford: a plain E[x^2]-E[x]^2 in fp32
 *                loses the variance of a channel whose |mean| >> std)
 *   finalize   : training: Chan merge of the parts in fp64 (the parts tile `count` rows in groups
 *                of group_rows rows, each in stripes of part_rows) + running-stat update
 *                (momentum, unbiased variance); eval: running statistics
 *   bn_act_fwd : out = dropout(act(y*scale + shift))
 *   bn_act_bwd : dy (grad of y), dgamma, dbeta; partial as colstats, coef [2][C] scratch
 * ------------------------------------------------------------------------------------ */
int fs2hip_colstats_parts(int M);
int fs2hip_colstats_part_rows(int M);
int fs2hip_colstats(const float* y, int M, int C, float* partial, void* stream);
/* the same over a bf16 tensor when in_bf16 != 0 (a convolution's bf16 result under bf16 activation storage) */
int fs2hip_colstats_b(const void* y, int M, int C, float* partial, int in_bf16, void* stream);
int fs2hip_bn_finalize(const float* partial, int nparts, long long count, int part_rows, int group_rows,
                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                       float momentum, float eps, int training, float* stats, int C, void* stream);
int fs2hip_bn_act_fwd(const float* y, const float* stats, float* out, int M, int C, int act, float drop_p,
                      unsigned long long drop_seed, const unsigned long long* drop_step, void* stream);
int fs2hip_bn_act_bwd(const float* dout, const float* y, const float* stats, float* partial, float* coef,
                      float* dgamma, float* dbeta, float* dy, int M, int C, int act, float drop_p,
                      unsigned long long drop_seed, const unsigned long long* drop_step, int training,
                      void* stream);
/* The same two with a bf16 form of the output (out_bf16 / dy_bf16, [M][C] bf16) for a consuming GEMM that reads bf16
 * operands from memory (Fs2GemmArgs.operand_bf16 == 4).  Either output pointer may be NULL (not both): with out / dy
 * NULL the tensor exists only in bf16. */
/* in_bf16: the inputs are bf16 tensors as well -- fwd: y (any non-zero value); bwd: bit 0 y, bit 1 dout. */
int fs2hip_bn_act_fwd_b(const void* y, const float* stats, float* out, void* out_bf16, int M, int C, int act,
                        float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step, int in_bf16,
                        void* stream);
int fs2hip_bn_act_bwd_b(const void* dout, const void* y, const float* stats, float* partial, float* coef,
                        float* dgamma, float* dbeta, float* dy, void* dy_bf16, int M, int C, int act, float drop_p,
                        unsigned long long drop_seed, const unsigned long long* drop_step, int training, int in_bf16,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * Positional table / embeddings / bucketize  (fs2/layers.py:123-140, fs2/model.py:183-193,
 * :233-241, fs2/variance_adaptor.py:197-205)
 * ------------------------------------------------------------------------------------ */
int fs2hip_posenc_table(const float* inv_freq, float* table, int T, int D, void* stream);
int fs2hip_add_posenc(const float* x, const float* table, const int* lens, float* out, int B, int T, int D,
                      void* stream);
int fs2hip_embedding_fwd(const int* idx, const float* W, float* out, int M, int V, int D, void* stream);
/* embedding backward = fs2hip_onehot + fs2hip_gemm (dW = onehot^T @ dy; split-K weight-gradient mode):
 * out[m][v] = (idx[m] == v && v != padding_idx), row length Vp (multiple of 4, >= vocabulary) */
int fs2hip_onehot(const int* idx, float* out, int M, int Vp, int padding_idx, void* stream);
/* out = x + W[lower_bound(bins, val*control)]; idx_out (int32, bit-exact vs torch.bucketize) optional.  A NaN value takes
 * bucket NB, as in torch.bucketize (W has NB + 1 rows). */
int fs2hip_bucket_embed_add(const float* val, float control, const float* bins, int NB, const float* W,
                            const float* x, float* out, int* idx_out, int M, int D, void* stream);
/* The same with the control in device memory (a tensor in InferenceControl): row r uses ctl[r / ctl_div] -- ctl_div = 1:
 * one value per row, ctl_div = rows per utterance: one per utterance -- or, with ctl_idx (int [M], the length
 * regulator's src_idx), ctl[(r / ctl_div) * ctl_T + ctl_idx[r]] with ctl_div = rows (frames) per utterance and ctl
 * [M / ctl_div][ctl_T]; the control is exactly 1 where ctl_idx[r] is not in [0, ctl_T).  scaled (optional, [M]) receives
 * val * control.  -22: ctl NULL, ctl_div <= 0, M % ctl_div != 0, D % 4 != 0, ctl_idx without ctl_T > 0. */
int fs2hip_bucket_embed_add_ctl(const float* val, const float* ctl, int ctl_div, const int* ctl_idx, int ctl_T,
                                const float* bins, int NB, const float* W, const float* x, float* out, int* idx_out,
                                float* scaled, int M, int D, void* stream);

/* ------------------------------------------------------------------------------------
 * LengthRegulator (fs2/variance_adaptor.py:65-81): out[b, t] = x[b, j] for the token j whose
 * duration segment contains frame t (zero rows past the total), bit-exact indexing.
 *   cum [B][Ts] inclusive cumulative durations (written), out_lens [B] = min(total, Tm),
 *   src_idx [B][Tm] source token or -1 (optional), posenc_table [>=Tm][D] added on valid frames
 *   (optional: fuses fs2/model.py:233-241).
 * bwd: dx[b, j] = sum of dy over the token's frame segment (contiguous, no atomics).
 * ------------------------------------------------------------------------------------ */
int fs2hip_length_regulate_fwd(const float* x, const int* dur, const float* posenc_table, float* out,
                               int* cum, int* out_lens, int* src_idx, int B, int Ts, int Tm, int D,
                               void* stream);
int fs2hip_length_regulate_bwd(const float* dy, const int* cum, float* dx, int B, int Ts, int Tm, int D,
                               void* stream);
/* cum [B][Ts] inclusive cumulative durations, out_lens [B] = min(total, Tm) (the first half of the forward).
 * expect_lens / mismatch (both or neither) + optional bad_count: the consistency check of the aligner's durations,
 * fs2/variance_adaptor.py:289-305 -- mismatch[b] = (total of utterance b != expect_lens[b]); each mismatch also adds 1
 * to *bad_count, a persistent device word the host polls instead of the per-utterance flags (no sync in a step). */
int fs2hip_duration_cumsum(const int* dur, int* cum, int* out_lens, const int* expect_lens, int* mismatch,
                           int* bad_count, int B, int Ts, int Tm, void* stream);

/* predictor head (fs2/variance_adaptor.py:53-62): out[m] = (x[m,:].w + b) * (t < lens[b]) */
int fs2hip_rowdot_fwd(const float* x, const float* w, const float* bias, const int* lens, float* out, int M,
                      int T, int C, void* stream);
int fs2hip_rowdot_blocks(int M);
int fs2hip_rowdot_bwd(const float* dout, const float* x, const float* w, const int* lens, float* dx,
                      float* partial, float* dw, float* dbias, int M, int T, int C, void* stream);

/* masked MSE (kind 0) / MAE (kind 1) of fs2/loss.py:44-106 with its padded-mean denominator;
 * tgt_int != NULL: target = log(tgt_int + 1) (duration loss).  Writes loss_out[0] and, if
 * dpred != NULL, d(loss)/d(pred).  partial: >= 1024 floats. */
int fs2hip_masked_loss(const float* pred, const float* tgt, const int* tgt_int, const int* lens, int B, int T,
                       int C, int kind, float weight, float* dpred, float* partial, float* loss_out,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Optimizer (fs2/model.py:530-549 AdamW + fs2/noam.py:20-26 + clip of fs2/cli/train.py:38).
 * `state` is a 32-byte device record { uint64 step; float lr, bc1, bc2, clip_coef, grad_norm, pad }
 * advanced on the device so that a captured hipGraph needs no new arguments per step; its first
 * 8 bytes double as the `drop_step` counter of the dropout kernels.
 * ------------------------------------------------------------------------------------ */
int fs2hip_step_advance(void* state, float base_lr, float warmup, float beta1, float beta2, void* stream);
int fs2hip_grad_clip_coef(const float* grad, long long n, float max_norm, float grad_scale, float* partial,
                          void* state, void* stream);
int fs2hip_adamw_step(float* p, const float* g, float* m, float* v, long long n, const void* state,
                      float beta1, float beta2, float eps, float weight_decay, void* stream);

/* bf16 operand storage (Fs2GemmArgs.operand_bf16 == 3; Lightning's `precision="bf16-mixed"` autocast copies in the
 * reference): dst = bf16(src), round to nearest even, n % 8 == 0; and dst[c][r] = bf16(src[r][c]) for a [rows][cols]
 * matrix with rows ld_src apart, dst rows ld_dst >= rows elements apart (pad columns zeroed), for `batch` matrices
 * stored back to back (the taps of a convolution weight). */
int fs2hip_cast_bf16(const float* src, void* dst, long long n, void* stream);
/* out[(b, t)][tap * C + c] = bf16(x[(b, t + dir * (tap - (taps - 1) / 2))][c]), zero outside [0, T): a k-tap 'same'
 * convolution's input rows side by side (x fp32 or bf16, C % 8 == 0, taps odd).  The PostNet's 80-mel-bin convolutions
 * (fs2/layers.py:143-212: first layer forward, last layer data gradient) then run as ONE plain K = taps * C GEMM on the
 * bf16-storage core; dir = +1 pairs with the weight as [taps * Cin][Cout], dir = -1 (data gradient) with the weight as
 * stored. */
int fs2hip_im2col_taps(const void* x, int x_bf16, void* out_bf16, int B, int T, int C, int taps, int dir, void* stream);
int fs2hip_transpose_cast_bf16(const float* src, int rows, int cols, int ld_src, void* dst, int ld_dst, int batch,
                               void* stream);
/* The same for up to FS2_TRANSPOSE_MAX_JOBS matrices in one launch: dst[c][r] = bf16(src[r][c]), src fp32 [rows][cols]
 * (dense), dst bf16 [cols][rows] (dense).  Keeps the transposed bf16 mirrors of the weights whose DATA gradient runs in
 * the forward orientation (dz . W with W [256][K'] -> W^T [K'][256], the out-projection / second pointwise convolution /
 * second feed-forward weights of a Conformer layer: torchaudio ConformerLayer, call sites fs2/model.py:193, :241), once
 * per optimizer step, beside the bf16 mirror of the flat parameter buffer. */
#define FS2_TRANSPOSE_MAX_JOBS 64
typedef struct {
  const float* src;
  void* dst;
  int rows, cols;
  int fp32_out; /* 0: dst is bf16; 1: dst is fp32 (the "32-true" mirrors of the same weights, tile 32 of fs2hip_gemm) */
  int pad_;
} Fs2TransposeJob;
int fs2hip_transpose_cast_bf16_multi(const Fs2TransposeJob* jobs, int njobs, void* stream);

/* out = a * x * dropmask + b * y (y may be NULL);  out[b,t,:] = x[b,t,:] + e[b,:] */
int fs2hip_axpby(const float* x, const float* y, float* out, long long n, float a, float b, float drop_p,
                 unsigned long long drop_seed, const unsigned long long* drop_step, void* stream);
int fs2hip_add_rowvec(const float* x, const float* e, float* out, int B, int T, int D, void* stream);
/* x *= *scalar (scalar in device memory; a no-op pass when it is exactly 1): the upstream gradient that autograd hands
 * to the node behind FastSpeech2.training_step's loss (fs2/model.py:384-390 returns the loss Lightning differentiates) */
int fs2hip_scale_dev(float* x, long long n, const float* scalar, void* stream);
/* out = dy * act'(aux) (aux = activation output for ReLU, input otherwise); bool mask t < lens[b]
 * (fs2/utils/heavy.py:11-15); out[0] = sum of n loss slots (fs2/loss.py:125) */
int fs2hip_dact_mul(const float* dy, const float* aux, float* out, long long n, int act, void* stream);
/* inference durations (fs2/variance_adaptor.py:360-366): out = int(max(rint(exp(logd) - 1) * control, 0)) */
int fs2hip_duration_round(const float* logd, float control, int* out, int n, void* stream);
/* the same with the control in device memory: element i uses ctl[i / ctl_div] (-22: ctl NULL, ctl_div <= 0,
 * n % ctl_div != 0) */
int fs2hip_duration_round_ctl(const float* logd, const float* ctl, int ctl_div, int* out, int n, void* stream);
int fs2hip_mask_from_lens(const int* lens, unsigned char* mask, int B, int T, void* stream);
int fs2hip_sum_slots(const float* x, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Learned alignment (fs2/attn/attention.py:195-251, fs2/attn/alignment.py:48-74,
 * fs2/attn/attention_loss.py:22-73, fs2/variance_adaptor.py:160-222, :267-268).
 * All attention maps are dense [B][T1 = frames][T2 = tokens] fp32.
 *   attn_dist       logits = -0.0005 * sum_c (q - k)^2      q [B][T1][C], k [B][T2][C]
 *   attn_softmax    logprob = log_softmax(logits) + log(prior + 1e-8); soft = softmax over keys < key_lens[b]
 *   mas             hard 0/1 map, hard_idx [B][T1] (token of each frame, -1 on padding), dur [B][T2] int32;
 *                   `in` = attn_soft (is_log 0) or log-probabilities (is_log 1); DP in fp32 adds/max only:
 *                   bit-exact against mas_width1 on the same input.  dirs_ws: B*T1*ceil(T2/32) uint32.
 *   avg_variance    phone-level mean of a frame-level track over each token's frames (non-zero count)
 *   attn_ctc_loss   AttentionCTCLoss value (loss_out[0], weight applied) and d/d logprob (may be NULL)
 *                   alpha_ws B*T1*(2*T2+1), lse_ws B*T1, nll_ws B floats
 *   attn_bin_loss   AttentionBinarizationLoss value and the coefficient the backward needs
 *   attn_softmax_bwd  d logits from d logprob (CTC) and the binarisation term (hard_idx, bin_coef)
 *   attn_dist_bwd   dq, dk from d logits (either may be NULL)
 * ------------------------------------------------------------------------------------ */
int fs2hip_attn_dist(const float* q, const float* k, float* logits, int B, int T1, int T2, int C, void* stream);
int fs2hip_attn_softmax(const float* logits, const float* prior, const int* key_lens, float* logprob,
                        float* soft, int B, int T1, int T2, void* stream);
int fs2hip_mas(const float* in, int is_log, const int* in_lens, const int* out_lens, float* hard,
               int* hard_idx, int* dur, unsigned* dirs_ws, int B, int Tm, int Ts, void* stream);
int fs2hip_avg_variance(const float* var, const int* cum, float* out, int B, int Tm, int Ts, void* stream);
int fs2hip_attn_ctc_loss(const float* logprob, const int* key_lens, const int* query_lens, float* alpha_ws,
                         float* lse_ws, float* nll_ws, float* dlogprob, float weight, float* loss_out, int B,
                         int Tm, int Ts, void* stream);
int fs2hip_attn_bin_loss(const float* soft, const int* hard_idx, float* partial, float weight, float* loss_out,
                         float* bin_coef, int B, int Tm, int Ts, void* stream);
int fs2hip_attn_softmax_bwd(const float* logits, const float* soft, const float* dlogprob, const int* hard_idx,
                            const float* bin_coef, float* dlogits, int B, int T1, int T2, void* stream);
int fs2hip_attn_dist_bwd(const float* dlogits, const float* q, const float* k, float* dq, float* dk, int B,
                         int T1, int T2, int C, void* stream);

/* ------------------------------------------------------------------------------------
 * GST style encoder (fs2/gst/model.py:103-257, fs2/gst/attn.py:48-194; BASELINE config 5).
 *   conv2d_s2_*     3x3 / stride 2 / pad 1 / no bias Conv2d on channels-last [B][H][W][C];
 *                   weights [kh][kw][Cin][Cout]; output extent (n - 1) / 2 + 1 per spatial dim;
 *                   weight gradient through partial[parts][9*Cin*Cout]
 *   gru_gate_*      one nn.GRU time step (gate order r, z, n): gi rows (stride gi_stride) and gh
 *                   [B][3U] come from the GEMM; gates [B][4U] keeps r, z, n, gh_n for the backward
 *   gst_attn_*      softmax(q k^T / 8) v for one query per utterance against NT <= 32 style tokens,
 *                   `heads` <= 4 heads of 64 dims; dk_part / dv_part are per-utterance [B][NT][F]
 *   act_apply       out = act(x)  (tanh of the style tokens)
 * ------------------------------------------------------------------------------------ */
int fs2hip_conv2d_s2_fwd(const float* x, const float* w, float* y, int B, int H, int W, int Cin, int Cout,
                         void* stream);
int fs2hip_conv2d_s2_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout,
                              void* stream);
/* The same convolution as GEMM operands (Cin % 4 == 0): col[B*Ho*Wo][9*Cin] gathers the 3x3 stride-2 windows (zero
 * outside the image), col2im sums dcol back into dx[B][H][W][Cin].  Weight seen as [9*Cin][Cout].
 * im2col with Cin == 1 writes rows of 12 floats (9 taps + 3 zeros) for the first layer's weight gradient. */
int fs2hip_im2col_s2(const float* x, float* col, int B, int H, int W, int Cin, void* stream);
int fs2hip_col2im_s2(const float* dcol, float* dx, int B, int H, int W, int Cin, void* stream);
int fs2hip_conv2d_s2_wgrad_parts(int B, int H, int W);
int fs2hip_conv2d_s2_bwd_weight(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W,
                                int Cin, int Cout, void* stream);
int fs2hip_gru_gate_fwd(const float* gi, long long gi_stride, const float* gh, const float* hprev, float* hnew,
                        float* gates, int B, int U, void* stream);
int fs2hip_gru_gate_bwd(const float* dh, const float* gates, const float* hprev, float* dgi, long long dgi_stride,
                        float* dgh, float* dhprev, int B, int U, void* stream);
int fs2hip_gst_attn_fwd(const float* q, const float* k, const float* v, float* p, float* ctx, int B, int NT,
                        int heads, void* stream);
int fs2hip_gst_attn_bwd(const float* dctx, const float* q, const float* k, const float* v, const float* p,
                        float* dq, float* dk_part, float* dv_part, int B, int NT, int heads, void* stream);
int fs2hip_act_apply(const float* x, float* out, long long n, int act, void* stream);

/* dst[0 .. nbytes) = byte, enqueued on the stream (what torch.zeros / Tensor.zero_() did inside a step: the loss slot
 * vector of fs2/model.py:387-389's terms, the GRU's initial state fs2/gst/model.py:140-147).  A launch-plan command like
 * every other entry point, which an ATen fill is not. */
int fs2hip_memset(void* dst, int byte, long long nbytes, void* stream);

/* The padding half of the reference's collate_method (fs2/dataset.py:257-293: every ragged column written into the
 * top-left corner of a zero tensor) on the device, for a batch that is padded to a length bucket's geometry instead of
 * to its own maxima: up to FS2_PAD_MAX_MEMBERS tensors in ONE launch.  A member is a dense tensor [B][src0][src1][row
 * bytes] copied into the dense [B][dst0][dst1][row bytes]; every destination byte outside the source box becomes 0.
 * An axis that is not padded has equal extents (a one-axis member: src1 == dst1 == 1); all extents equal is a plain
 * copy, and src == dst with all extents equal is skipped.  Byte-wise: int32 / int64 token and duration tensors and fp32
 * features alike.  The member table is passed by value in the kernel argument (nothing is uploaded; a launch plan keeps
 * a host copy of it).  FS2HIP_EINVAL: n < 1 or n > FS2_PAD_MAX_MEMBERS, a null pointer, a non-positive extent, a
 * destination extent smaller than the source's, overlapping source and destination. */
#define FS2_PAD_MAX_MEMBERS 16
typedef struct {
  const void* src;
  void* dst;
  int B;
  int src0, src1; /* source extents of the (up to) two padded axes */
  int dst0, dst1; /* destination extents */
  int pad_;
  long long row_bytes; /* bytes of the contiguous inner row behind the padded axes */
} Fs2PadMember;
int fs2hip_pad_batch(const Fs2PadMember* members, int n, void* stream);

/* The way out of the GPU for a batch of predicted spectrograms (fs2/prediction_writing_callback.py:257-262 stores
 * [K bands, T frames] per utterance): y [B][Tm][C] fp32, lens [B] (clamped to 0..Tm here).  For every utterance b the
 * [C][len_b] transpose of y[b, :len_b, :] is written contiguously at packed + offsets[b]; offsets [B + 1] is produced
 * here from lens (a one-workgroup prologue launch): offsets[b] = C * (len_0 + ... + len_{b-1}), offsets[B] = the total.
 * Rows at and beyond len_b are never read; a length of 0 contributes nothing.  packed holds B * Tm * C floats (the worst
 * case): nothing outside packed[0 .. offsets[B]) and offsets[0 .. B] is written whatever lens holds.  Any C, Tm >= 1;
 * no alignment is required beyond the element types'. */
int fs2hip_pack_spec(const float* y, const int* lens, float* packed, long long* offsets, int B, int Tm, int C,
                     void* stream);

/* Exact-length inference: x is a dense [B][T][row_bytes] activation of any element type, lens [B] in device memory
 * (clamped to 0..T here).  Every row t >= lens[b] of utterance b becomes all-zero bytes -- 0.0 in fp32 and bf16 alike --
 * by plain stores: the tail is never read (it may hold NaN or Inf), rows below the length are neither read nor written,
 * and the work is proportional to the padding.  16-byte stores when row_bytes and x are multiples of 16, else 4-byte,
 * 2-byte (an odd bf16 column count) or single-byte stores by the same rule.  In place, on the stream, no host
 * synchronisation.  FS2HIP_EINVAL: a null pointer, a non-positive extent, B > 65535. */
int fs2hip_zero_tail_rows(void* x, long long row_bytes, const int* lens, int B, int T, void* stream);

/* Per-utterance loss scores of a teacher-forced batch (fs2/prediction_writing_callback.py:138-211 runs the model at batch
 * size 1 and calls fs2/loss.py:19-126 on every utterance): scores [B][FS2_SCORE_COLUMNS] fp32, dense, every element
 * written.  Columns: pitch, energy, duration, spec, postnet, attn_ctc, attn_bin, total.  Row b holds what the loss gives
 * for the batch of ONE made of utterance b cut to its own lengths -- its means run over the utterance's own len_b * C
 * elements, not over the padded B * T * C box fs2hip_masked_loss divides by.
 *   members[0 .. n): the mean terms, one per column 0 .. 6, the table passed by value in the kernel argument (a launch plan
 *     keeps a host copy, as of Fs2PadMember).  pred [B][T][C] fp32; the target is tgt [B][T][C] fp32, or, when tgt_int is
 *     non-null, log(tgt_int + 1) of an int32 tensor of that shape (durations, fs2/loss.py:81); lens [B] int32 in device
 *     memory, len_b = clamp(lens[b], 0, T).  scores[b][column] = weight * sum_{t < len_b, c} f(pred - tgt) / (len_b * C),
 *     f the square (kind 0) or the absolute value (kind 1); 0 when len_b is 0.  Rows at and beyond len_b are never read
 *     (they may hold NaN).
 *   soft [B][Tm][Ts], hard_idx [B][Tm] (both or neither), mel_lens [B]: attn_bin = -bin_weight * sum_{t < len_b,
 *     0 <= hard_idx < Ts} log(max(soft[b][t][hard_idx[b][t]], 1e-12)) / (number of such t), 0 when there is none
 *     (fs2/attn/attention_loss.py:65-73 on the utterance's own box).
 *   nll [B] or NULL: attn_ctc = ctc_weight * nll[b], nll being what fs2hip_attn_ctc_loss leaves in nll_ws -- already
 *     divided by the target length and zeroed where infinite: nn.CTCLoss(zero_infinity=True), mean reduction, batch of one.
 *   total = the columns 0 .. 6 added in that order in fp32 (fs2hip_sum_slots' order); a column without a term is 0.
 * Two launches, no atomics, no workspace.  An utterance's elements are added in an order that depends on len_b * C only --
 * not on B, T, the utterance's place in the batch or the alignment of its base address (16-byte loads are used where the
 * base allows them, the additions follow the logical element index either way): a row of a batch is bit-equal to the same
 * data scored with B = 1, T = len_b.
 * FS2HIP_EINVAL: scores NULL, B <= 0, n < 0 or n > FS2_SCORE_MAX_MEMBERS, a member without pred, lens or a target, with a
 * non-positive T or C, a kind other than 0 / 1, a column outside 0 .. 6 or one that another member, the binarisation term
 * (6) or nll (5) also fills; soft without hard_idx or mel_lens or with non-positive Tm / Ts. */
#define FS2_SCORE_MAX_MEMBERS 8
#define FS2_SCORE_COLUMNS 8
typedef struct {
  const float* pred;
  const float* tgt;
  const int* tgt_int; /* non-null: the target is log(tgt_int + 1) and tgt is ignored */
  const int* lens;
  int T, C;
  int kind; /* 0 = squared error, 1 = absolute error */
  float weight;
  int column;
  int pad_;
} Fs2ScoreMember;
int fs2hip_utterance_losses(const Fs2ScoreMember* members, int n, const float* soft, const int* hard_idx,
                            const int* mel_lens, int Tm, int Ts, float bin_weight, const float* nll, float ctc_weight,
                            float* scores, int B, void* stream);

/* fs2hip_attn_softmax with the log_softmax taken over the utterance's own keys (j < key_lens[b], when 1 <= key_lens[b] < T2)
 * instead of all T2: row (b, t) of logprob is then what the utterance gives when it is run alone, where T2 is its key
 * count -- in a padded batch the padded keys' logits are finite and enter the plain form's normaliser, which shifts every
 * row of logprob by a constant that the CTC loss (its blank logit is a fixed -1) does not forgive.  Exact-length inference
 * (FastSpeech2.forward(exact_lengths=True)) uses this form.  soft is the same masked softmax (it does not see the shift);
 * logprob at keys >= key_lens[b] holds the same expression and is not meant to be read.  -22 also for a null pointer. */
int fs2hip_attn_softmax_own_keys(const float* logits, const float* prior, const int* key_lens, float* logprob,
                                 float* soft, int B, int T1, int T2, void* stream);

/* The aligner's attention prior computed from the lengths (the matrix the data pipeline otherwise loads from
 * attn/<name>-attn-prior.pt, collates and copies to the device): prior [B][Tm][Ts] fp32, dense, EVERY element written and
 * none read (the caller need not clear it).  Per utterance M = clamp(mel_lens[b], 0, Tm), P = clamp(src_lens[b], 0, Ts),
 * n = P - 1; for frame i < M and key k < P, with a = scaling * (i + 1) and b' = scaling * (M - i):
 *     prior[b][i][k] = C(n, k) * Beta(k + a, n - k + b') / Beta(a, b')          (= scipy betabinom(n, a, b').pmf(k))
 * and exactly 0.f where i >= M or k >= P (what zero padding to the batch's or a bucket's geometry gives); the P = 1 row
 * is exactly 1.  Evaluated in fp64 in log space -- lgamma(n+1) - lgamma(k+1) - lgamma(n-k+1) + lgamma(k+a) + lgamma(n-k+b')
 * - lgamma(n+a+b') - (lgamma(a) + lgamma(b') - lgamma(a+b')), one exp -- and rounded to fp32 once, at the store: the terms
 * reach about 7 000 at 1291 x 200, where one fp32 ulp is 5e-4.  -22: a null pointer, a non-positive extent, scaling <= 0. */
int fs2hip_attn_prior(const int* mel_lens, const int* src_lens, float* prior, int B, int Tm, int Ts, float scaling,
                      void* stream);

/* The way out of the GPU for a synthesized batch's per-token and per-frame quantities -- the rounded durations and the
 * pitch and energy predictions the reference leaves in its padded output dict (fs2/variance_adaptor.py:399-411) and its
 * TextGrid writer reads one utterance at a time (fs2/prediction_writing_callback.py:331-347): up to FS2_PACK_MAX_MEMBERS
 * dense [B][T] tensors of 4-byte elements, each cut to every utterance's own length and packed back to back, in ONE call.
 * For member m and utterance b, with len = clamp(lens[b], 0, T):
 *     dst[offsets[b] .. offsets[b] + len) = src[b * T .. b * T + len)
 * offsets [B + 1] is produced here from lens (one prologue launch, a workgroup per member): offsets[b] = len_0 + ... +
 * len_{b-1} in elements, offsets[B] = the member's total.  Members may differ in T and in lens (token-level members take
 * src_lens, frame-level members tgt_lens).  Copied byte-wise: int32 and fp32 alike.  Elements of src at and beyond len
 * are never read; nothing at or beyond dst[offsets[B]] and nothing but offsets[0 .. B] is written whatever lens holds, so
 * dst must hold the member's total (B * T elements is the worst case).  dst needs 4-byte alignment only.  The member
 * table is passed by value in the kernel argument (nothing is uploaded; a launch plan keeps a host copy, as of
 * Fs2PadMember).  Two launches, no host read, no atomics, no workspace.
 * FS2HIP_EINVAL, before any launch: members NULL, n < 1 or n > FS2_PACK_MAX_MEMBERS, B <= 0, a member with a null field
 * or T <= 0. */
#define FS2_PACK_MAX_MEMBERS 8
typedef struct {
  const void* src;    /* [B][T], 4-byte elements (int32 or fp32: copied byte-wise) */
  const int* lens;    /* [B] in GPU memory; clamped to 0..T on the device */
  void* dst;          /* packed rows of this member, back to back */
  long long* offsets; /* [B + 1] element offsets into dst, total last; written by the call */
  int T;
  int pad_;
} Fs2PackMember;
int fs2hip_pack_rows(const Fs2PackMember* members, int n, int B, void* stream);

/* Length-aware style encoding (inference): the reference encoder ignores lengths (fs2/gst/model.py:192), so a padded
 * reference gives another style vector than the same reference alone.
 *   gru_last_state  the whole nn.GRU recurrence (gate order r, z, n) from h0 = 0 in ONE launch, with a step count per
 *                   utterance: gi [B][T][3U] (input projections incl. b_ih), w_hh [3U][U], b_hh [3U], steps [B] int32
 *                   in device memory; h_out [B][U] = the state after clamp(steps[b], 0, T) steps.  A count of 0 writes
 *                   zeros; rows of gi at and beyond an utterance's count are never read (they may hold NaN).  fp32; the
 *                   recurrent sums add k ascending, so a row's result depends on that row's gi alone (bit-equal whatever
 *                   the batch).  U must be 128, w_hh 16-byte aligned: FS2HIP_EINVAL otherwise, as for a null pointer
 *                   or a non-positive extent.
 *   conv_s2_lens    table [n + 1][B] int32: table[0] = lens, table[l + 1] = (table[l] - 1) / 2 + 1 where table[l] > 0,
 *                   else 0 -- the rows an utterance keeps after l stride-2 convolutions.  0 <= n <= 8. */
int fs2hip_gru_last_state(const float* gi, const float* w_hh, const float* b_hh, const int* steps, float* h_out, int B,
                          int T, int U, void* stream);
int fs2hip_conv_s2_lens(const int* lens, int* table, int B, int n, void* stream);

/* Length-aware style encoding (training): every utterance's style from its own frames, with a backward pass.  All fp32,
 * lengths read from device memory, no host synchronisation, no float atomics, deterministic.  FS2HIP_EINVAL, before any
 * launch: a null pointer, a non-positive extent, U != 128, a misaligned tensor.
 *   gru_fwd_states  gru_last_state kept for training: the same recurrence in the same arithmetic order (h_out is
 *                   bit-equal), which also writes hs [B][T+1][U] (hs[b][0] = 0, hs[b][t+1] = the state after step t) and
 *                   gates [B][T][4U] = (r, z, n, gh_n) per step.  Rows of gi at and beyond clamp(steps[b], 0, T) are never
 *                   read; the rows of hs and gates beyond it are written as zeros.
 *   gru_bwd_states  the whole backward through time in ONE launch, a workgroup per utterance: from dh_last [B][U] it
 *                   writes dgi [B][T][3U] (gradient of gi), dgh [B][T+1][3U] (gradient of w_hh h_{t-1} + b_hh; row t
 *                   pairs with hs[b][t], so dgh^T hs over all B * (T + 1) rows is the gradient of w_hh and dgh's column
 *                   sums that of b_hh) and dh0 [B][U] (gradient of the initial state; dh_last where there is no step).
 *                   Rows at and beyond an utterance's step count, row T of dgh included, are exact zeros.  The sums add
 *                   in a fixed order and read that utterance alone: bit-equal whatever the batch.
 * BatchNorm over the VALID positions of y [B][H][W][C] (channels last; C % 4 == 0, C <= 1024): utterance b keeps its first
 * clamp(lens[b], 0, H) rows of H, and rows beyond them are never read (they may hold NaN).
 *   bn_lens_parts   rows of the `partial` scratch [parts][2][C] both calls below take (0 for invalid extents)
 *   bn_stats_lens   per-channel mean and biased variance over the N = W * sum_b L[b] valid positions (pivot-shifted
 *                   stripes merged with Chan's formula in fp64, as colstats + bn_finalize), written as the stats [5][C]
 *                   of bn_finalize (scale, shift, mean, invstd, eps) for bn_act_fwd; the running buffers (both or neither
 *                   may be NULL) move with `momentum` and the unbiased variance N / (N - 1).  N = 0: mean 0, variance 0,
 *                   running buffers untouched.
 *   bn_act_bwd_lens backward of act(y * scale + shift) with those statistics: dgamma, dbeta, and dy [B][H][W][C] whose
 *                   sums and 1 / N run over the valid positions; rows of dy beyond the lengths are written as zeros, rows
 *                   of dout and y beyond them are never read.  coef: [2][C] scratch.  Up to 16 valid rows in all are
 *                   taken in fp64 (as bn_act_bwd's few-row form). */
int fs2hip_gru_fwd_states(const float* gi, const float* w_hh, const float* b_hh, const int* steps, float* hs, float* gates,
                          float* h_out, int B, int T, int U, void* stream);
int fs2hip_gru_bwd_states(const float* dh_last, const float* hs, const float* gates, const float* w_hh, const int* steps,
                          float* dgi, float* dgh, float* dh0, int B, int T, int U, void* stream);
int fs2hip_bn_lens_parts(int B, int H, int W);
int fs2hip_bn_stats_lens(const float* y, const int* lens, float* partial, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, float* stats, int B, int H,
                         int W, int C, void* stream);
int fs2hip_bn_act_bwd_lens(const float* dout, const float* y, const float* stats, const int* lens, float* partial,
                           float* coef, float* dgamma, float* dbeta, float* dy, int B, int H, int W, int C, int act,
                           void* stream);

/* Dynamic time warping between two batches of frame sequences of different lengths (csrc/dtw.hip): the distance
 * `fs2l synthesize --compare-to` reports between a free synthesis and the recorded mel.  Both calls are fp32, read the
 * lengths from device memory (clamped to 0 .. T here), and use no host synchronisation, no atomics and no workspace.
 *   frame_dist  a [B][T1][C], b [B][T2][C], cost [B][T1][T2].  With n = clamp(a_lens[u], 0, T1), r = clamp(b_lens[u], 0, T2):
 *                   cost[u][i][j] = sqrtf(sum_c (a[u][i][c] - b[u][j][c])^2)      for i < n, j < r
 *               in fp32 without contraction, c ascending from 0.f, the same for every element whatever the tiling.
 *               Nothing else of cost is written; rows of a and b at and beyond the lengths are never read (they may hold
 *               NaN).  C <= FS2_FRAME_DIST_MAX_C (the tiles' LDS), B <= 65535.
 *   dtw         per utterance, on cost's n x r box: D[0][0] = c[0][0], S[0][0] = 1, and otherwise
 *                   best = D[i-1][j-1]; if (D[i-1][j] < best) take (i-1, j); if (D[i][j-1] < best) take (i, j-1)
 *                   D[i][j] = c[i][j] + best, S[i][j] = S[taken] + 1
 *               with strict <, in that order, a predecessor that does not exist counting as +inf.  total[u] = D[n-1][r-1],
 *               steps[u] = S[n-1][r-1] = the cells on the path a backtrack under the same rule finds; (0.f, 0) when n or r
 *               is 0.  Adds and compares only: bit-exact from cost, and a row does not depend on the rest of the batch.
 *               total and steps are written for every u; nothing outside the box is read.  One wavefront per utterance,
 *               64 columns at a time, ceil(r / 64) * (n + 63) dependent steps at most.  T1 <= FS2_DTW_MAX_T1 (8 bytes of LDS
 *               per row beside the 16 KiB cost ring).
 *   dtw_dirs    dtw that also keeps, for every cell of the box, the predecessor it took: dirs [B][T1][T2], ONE BYTE per cell
 *               (no packed form), 0 = diagonal (i-1, j-1), 1 = up (i-1, j), 2 = left (i, j-1); cell (0, 0) gets 0.  total
 *               and steps are bit-equal to dtw's on the same matrix.  No byte of dirs outside the box is written; an empty
 *               box writes total = 0, steps = 0 and no direction.  The codes leave through a second LDS ring of 64 x 64
 *               bytes (a row of 64 codes per store), which the 64 KiB of dynamic LDS has to hold as well:
 *               T1 <= FS2_DTW_PATH_MAX_T1 = (65536 - 16384 - 4096) / 8.
 *   dtw_path    the backtrack: from (n-1, r-1) the walk follows dirs to (0, 0) and writes, for every row i < n of the box,
 *                   ref_first[u][i], ref_last[u][i]   the smallest and largest column j of the path's cells in row i
 *                   frame_cost[u][i]                  cost[i][ref_last] + cost[i][ref_last - 1] + ... + cost[i][ref_first]
 *               (all [B][T1]; the fp32 sum starts from the cell at ref_last and adds the others in the order the walk meets
 *               them, j descending, without contraction: bit-defined).  Rows i >= n are never written, an empty box writes
 *               nothing, nothing outside the box is read.  In column 0 the walk only goes up and in row 0 only left
 *               whatever dirs says, and any code but 1 and 2 counts as diagonal, so no content of dirs leads outside the
 *               box.  One wavefront per utterance, at most n + r - 1 dependent steps, read from LDS tiles of 32 x 64 cells.
 * FS2HIP_EINVAL, before any launch: a null pointer, a non-positive extent, an extent beyond the limits above. */
#define FS2_FRAME_DIST_MAX_C 204
#define FS2_DTW_MAX_T1 6144
#define FS2_DTW_PATH_MAX_T1 5632
int fs2hip_frame_dist(const float* a, const int* a_lens, const float* b, const int* b_lens, float* cost, int B, int T1,
                      int T2, int C, void* stream);
int fs2hip_dtw(const float* cost, const int* lens1, const int* lens2, float* total, int* steps, int B, int T1, int T2,
               void* stream);
int fs2hip_dtw_dirs(const float* cost, const int* lens1, const int* lens2, float* total, int* steps, unsigned char* dirs,
                    int B, int T1, int T2, void* stream);
int fs2hip_dtw_path(const float* cost, const unsigned char* dirs, const int* lens1, const int* lens2, int* ref_first,
                    int* ref_last, float* frame_cost, int B, int T1, int T2, void* stream);

/* Cepstral coefficients of frame sequences (csrc/cepstra.hip): the features `fs2l synthesize --compare-to DIR --cepstra K`
 * and `fs2l train --val-synthesis --val-cepstra K` take the second DTW distance on (MCD-DTW's: the low DCT coefficients of
 * a log-mel frame, the energy term dropped).  fp32, the lengths are read from device memory (clamped to 0 .. T here), no
 * host synchronisation, no atomics and no workspace.
 *   cepstra     x [B][T][C], table [K][C], out [B][T][K].  With n = clamp(lens[b], 0, T):
 *                   out[b][t][k] = (((0.f + x[b][t][0] * table[k][0]) + x[b][t][1] * table[k][1]) + ...)   for t < n, k < K
 *               in fp32 without contraction, m ascending, the same for every element whatever the tiling: bit-defined.
 *               Rows t >= n of x are never read (they may hold NaN) and rows t >= n of out are never written; lens[b] = 0
 *               writes nothing.  The table is the caller's (hip.dct_table: orthonormal DCT-II, rows 1 .. K,
 *               table[k][m] = sqrt(2 / C) * cos(pi * (k + 1) * (m + 0.5) / C), float64 rounded to fp32).  A workgroup
 *               stages 64 rows in LDS (odd row stride, a lane per row), its four wavefronts split the K coefficients and
 *               read the table by uniform loads, and the 64 x K block of results leaves through the same LDS tile in one
 *               contiguous piece.  1 <= C <= FS2_FRAME_DIST_MAX_C, 1 <= K <= min(C - 1, FS2_CEPSTRA_MAX_K).
 * FS2HIP_EINVAL, before any launch: a null pointer, a non-positive extent, an extent beyond the limits above. */
#define FS2_CEPSTRA_MAX_K 64
int fs2hip_cepstra(const float* x, const int* lens, const float* table, float* out, int B, int T, int C, int K,
                   void* stream);

/* ------------------------------------------------------------------------------------
 * Launch plans: a training step's whole launch sequence enqueued by ONE call.
 *
 * The reference's step is Python all the way down (Lightning -> nn.Module.forward -> ATen dispatch,
 * fs2/model.py:153-268, :384-390); this build's eager step is Python down to the entry points above (~590 launches,
 * ~18 us of interpreter time each: the host needs 10 ms to enqueue an 11 ms bf16 step).  A plan is that sequence
 * recorded once per batch geometry -- every entry-point call with its arguments, on which of the two streams it
 * ran, and the fork / join events between them -- and replayed by fs2hip_plan_replay: the host cost of a step
 * becomes the launches themselves.  The recorded step's temporaries live in a memory pool of the plan's own (the
 * caller's business: fastspeech2_lightning_amd/plan.py), so the recorded addresses stay valid; inputs are copied into
 * the recorded input buffers; dropout masks, the learning-rate schedule and BatchNorm statistics advance through
 * device memory exactly as in the eager step, which is why a replay is bit-identical to it (tests/test_plan_gpu.py).
 *
 * op >= 0: index of an entry point (fs2hip_plan_op_id(name); the table is generated from this header by
 *          tools/gen_plan_thunks.py -> csrc/plan_thunks.inc); a[i] = its i-th argument, the stream excluded:
 *          pointers and integers as they are (int sign-extended), a float as its bit pattern in the low 32 bits;
 *          struct arguments (Fs2GemmArgs, job arrays) point to HOST copies the plan's owner keeps alive.
 * FS2_PLAN_SYNC: record events[a[0]] on stream a[1], make stream a[2] wait for it (stream indices into the replay call's
 *          stream table: 0 = the main stream, 1.. = the step's side streams).
 * ------------------------------------------------------------------------------------ */
#define FS2_PLAN_SLOTS 20
#define FS2_PLAN_SYNC (-1)
typedef struct {
  int op;      /* entry-point id or FS2_PLAN_SYNC */
  int stream;  /* index into the stream table of fs2hip_plan_replay: 0 main, 1.. side streams */
  unsigned long long a[FS2_PLAN_SLOTS];
} Fs2PlanCmd;

int fs2hip_plan_op_count(void);
/* id of an entry point by name, -1 when it is not a plan op (no stream parameter, unknown) */
int fs2hip_plan_op_id(const char* name);
/* n events for FS2_PLAN_SYNC commands (created without timing) into out[0..n); destroy frees them */
int fs2hip_plan_events_create(void** out, int n);
int fs2hip_plan_events_destroy(void* const* events, int n);
/* enqueues cmds[first .. last); on failure returns the failing command's code and writes its index to *failed_at */
int fs2hip_plan_replay(const Fs2PlanCmd* cmds, int first, int last, void* const* streams, int n_streams,
                       void* const* events, int n_events, int* failed_at);

#ifdef __cplusplus
}
#endif
#endif /* FS2HIP_H */
