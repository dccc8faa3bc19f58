"""Kernel parity of the variance-adaptor gather kernels and the optimizer kernels of ``csrc/misc.hip``: positional table,
masked positional add, row-vector add, axpby (+ the dropout mask's host definition), text embedding forward / backward,
bucketize + embedding (both control forms), the LengthRegulator and the fused Noam / global-norm clip / AdamW step --
against the float64 references of ``tests/adaptor_references.py`` at the sizes where their grid-stride loops, lane loops
and scalar tails take every path, and the refusals.

Exact outputs (gathers, integer results, one fp32 add) are compared with ``torch.equal``; outputs are allocated
poisoned (NaN, or -77 for the integer ones), so an element a kernel skips fails its comparison.

Error measure of the float quantities.  Sums of many terms (embedding gradient, LengthRegulator backward): per element,
|got - ref64| over the sum of the magnitudes of the element's terms (a sum itself may cancel), then the worst element.
Optimizer state ``m``, ``v`` and the displacement ``p - p0`` after the last step, and ``axpby``: max |got - ref64| over
max |ref64|.  ``grad_norm`` and ``clip_coef``: relative.  The yardstick is PyTorch's own fp32 CPU computation of the same
thing on the same inputs (``F.embedding`` backward, autograd of ``repeat_interleave``, ``torch.optim.AdamW`` +
``clip_grad_norm_``, the plain expression), measured the same way against float64; a kernel passes with
``err <= MARGIN[quantity] * torch_err + FLOOR``, FLOOR = 4 * 2^-23.  The kernels and PyTorch sum in different orders and
neither is the better one, hence a margin.

Measured on an MI355X over all cases: the worst kernel error, the worst PyTorch-fp32 error, and the worst ratio
kernel / PyTorch among the checks where the kernel is off by more than one ulp (2^-23) of the scale:

  quantity                                  kernel    PyTorch   worst ratio
  axpby (a*x + b*y, a*x)                    6.1e-08   8.4e-08   -
  embedding dW (a row sums 1 642 terms)     1.4e-07   1.6e-07   0.90
  regulator dx (a token sums 600 frames)    2.1e-07   2.1e-07   1.00
  grad_norm     n <= 1000                   7.4e-08   9.3e-08   -
  grad_norm     n = 8192 * 256 + 3          4.7e-08   6.9e-06   -
  clip_coef     n <= 1000                   6.5e-08   7.7e-08   -
  clip_coef     n = 8192 * 256 + 3          4.5e-08   6.8e-06   -
  m             n <= 1000                   1.4e-07   1.2e-07   1.36
  m             n = 8192 * 256 + 3          1.5e-07   5.2e-06   0.03
  v             n <= 1000                   1.5e-07   1.6e-07   1.00
  v             n = 8192 * 256 + 3          3.2e-07   1.2e-05   0.03
  displacement  n <= 1000                   1.7e-04   2.0e-04   1.00
  displacement  n = 8192 * 256 + 3          3.0e-04   3.0e-04   1.00
  positional table, worst absolute error    7.0e-08 at T = 2048 (its bound: 2e-7 + 2e-6 |ref|)

Chosen from them: FLOOR = 4 * 2^-23 = 4.8e-07 and MARGIN = 2.0 (embedding dW, regulator dx, v, displacement), 2.5 (m),
1.0 (grad_norm, clip_coef, axpby: the kernel is never off by more than one ulp there) -- each at most about twice the
quantity's worst ratio.  PyTorch's large-n figures for grad_norm, clip_coef, m and v carry its fp32 norm of two million
elements; the kernel finishes that sum in double.  One margin for both sizes would leave the large-n bound 50 to 150
times the kernel's error, so n = 8192 * 256 + 3 has margins of its own, from its own worst ratios (counting the checks
below one ulp too: grad_norm 0.10, clip_coef 0.008, m and v 0.03): 0.2, 0.02, 0.06, 0.06, and 2.0 for the
displacement.  The displacement is 1e-2 on parameters of magnitude up to 5, so the
twelve fp32 roundings of p itself (ulp 4.8e-07 each) are 3e-4 of it, in the kernel and in PyTorch alike: that is the
resolution of this check, a 0.1 % error of the step.

Which test launches which kernel:

  fs2hip_posenc_table          posenc_table_kernel                  test_posenc_table
  fs2hip_add_posenc            add_posenc_kernel (strided: 5x821x1024)  test_add_posenc
  fs2hip_add_rowvec            add_rowvec_kernel (strided: 2x1025x1024) test_add_rowvec
  fs2hip_axpby                 axpby_kernel (strided: 8192*256 + 5)  test_axpby_against_float64, test_axpby_mask_is_the_host_rule
  fs2hip_embedding_fwd         embedding_fwd_kernel                 test_embedding_forward
  fs2hip_onehot + weight GEMM  onehot_kernel (strided: 25003 x 84 only)  test_embedding_backward
  fs2hip_bucket_embed_add      bucket_embed_add_kernel              test_bucket_embed_add
  fs2hip_bucket_embed_add_ctl  bucket_embed_add_ctl_kernel          test_bucket_embed_add_tensor_control
  fs2hip_length_regulate_fwd   lr_cumsum_kernel, lr_gather_kernel   test_length_regulator_forward
  fs2hip_duration_cumsum       lr_cumsum_kernel                     test_length_regulator_forward
  fs2hip_length_regulate_bwd   lr_bwd_kernel                        test_length_regulator_backward
  fs2hip_step_advance          step_advance_kernel                  test_optimizer
  fs2hip_grad_clip_coef        sumsq_kernel (strided, 3-element tail: 8192*256 + 3), clip_finish_kernel   test_optimizer
  fs2hip_adamw_step            adamw_kernel (strided: 8192*256 + 3)  test_optimizer
  every entry point above      (no launch)                          test_refusals_*
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import adaptor_references as R
from tests import layernorm_references as LR

pytestmark = pytest.mark.gpu

DEN_FLOOR = 1e-12
FLOOR = 4 * 2.0 ** -23
#: per quantity, at most about twice the worst ratio measured (module docstring)
MARGIN = {"embedding dW": 2.0, "regulator dx": 2.0, "m": 2.5, "v": 2.0, "displacement": 2.0, "grad_norm": 1.0,
          "clip_coef": 1.0, "axpby": 1.0,
          # n = 8192 * 256 + 3: PyTorch's figures carry its fp32 norm of two million elements, the kernel's do not
          "m large": 0.06, "v large": 0.06, "displacement large": 2.0, "grad_norm large": 0.2, "clip_coef large": 0.02}
EINVAL = -22
POISON_INT = -77  # no bucket, cumulative duration, length or source token is negative below -1


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    """Every ``torch.empty`` / ``torch.empty_like`` on the GPU comes back as NaN (floating types) or -77 (integer types:
    ``idx``, ``cum``, ``lens``, ``src_idx``) while a test of this file runs (the wrappers allocate their results that way):
    an element a kernel skips is a NaN or a -77, not whatever an earlier, identical call left in the block the allocator
    hands out again."""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.numel():
            if t.is_floating_point():
                t.fill_(float("nan"))
            elif t.dtype in (torch.int32, torch.int64):
                t.fill_(POISON_INT)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: poisoned(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poisoned(real_empty_like(*a, **k)))


# ---------------------------------------------------------------------------------------------------------------------
# measure
# ---------------------------------------------------------------------------------------------------------------------
def elem_err(got, ref64, scale64):
    """Worst element of |got - ref64| / scale, every element with its own scale."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    return float(((got - ref64).abs() / scale64.clamp_min(DEN_FLOOR)).max())


def max_err(got, ref64):
    """max |got - ref64| over max |ref64|."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    return float((got - ref64).abs().max()) / max(float(ref64.abs().max()), DEN_FLOOR)


def rel_err(got, ref):
    got = float(got)
    assert math.isfinite(got)
    return abs(got - ref) / max(abs(ref), DEN_FLOOR)


def within(quantity, tag, err, yard):
    """The kernel's error against the yardstick's; prints the figures first (``pytest -s`` keeps them)."""
    print(f"ADFIG {quantity} | {tag} | kernel {err:.3e} torch {yard:.3e} ratio {err / max(yard, 1e-300):.2f}")
    assert err <= MARGIN[quantity] * yard + FLOOR, \
        f"{tag} {quantity}: kernel error {err:.3e}, PyTorch fp32 error {yard:.3e}, margin {MARGIN[quantity]}"


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# positional table, elementwise adds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", [(2048, 384), (257, 6), (1, 2)])
def test_posenc_table(H, T, D):
    """sin / cos of the fp32 angle t * inv_freq[c], angles up to thousands of radians, against float64."""
    inv = R.inv_freq(D)
    tab = H.posenc_table(inv.cuda(), T, D)
    assert tab.shape == (T, D)
    want = R.posenc_table64(inv, T)
    print(f"ADFIG posenc table | T={T} D={D} | worst abs error {float((tab.cpu().double() - want).abs().max()):.3e}")
    np.testing.assert_allclose(tab.cpu().double().numpy(), want.numpy(), rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("B,T,D,lens", [(5, 821, 1024, [0, 1, 821, 824, 400]), (3, 9, 16, [1, 0, 12]),
                                         (4, 9, 16, [1, 0, 9, 12])])
def test_add_posenc(H, B, T, D, lens):
    """Valid frames are x + table[t] (one fp32 add), padded frames x bit for bit; a table longer than T; the first shape is
    just past the 4096 x 256 float4 of one pass of the grid."""
    g = R.gen(B + T + D)
    x, table = torch.randn(B, T, D, generator=g), torch.randn(T + 5, D, generator=g)
    lens = torch.tensor(lens, dtype=torch.int32)
    if T > 100:
        assert B * T * D // 4 > 4096 * 256
    got = H.add_posenc(x.cuda(), table.cuda(), lens.cuda(), B, T).cpu()
    assert torch.equal(got, R.add_posenc(x, table, lens))
    pad = torch.arange(T)[None, :] >= lens[:, None]
    assert int(pad.sum()) > 0 and same_bits(got[pad], x[pad])


@pytest.mark.parametrize("B,T,D", [(2, 1025, 1024), (3, 5, 6)])
def test_add_rowvec(H, B, T, D):
    g = R.gen(B * T + D)
    x, e = torch.randn(B, T, D, generator=g), torch.randn(B, D, generator=g)
    if T > 100:
        assert B * T * D > 8192 * 256
    assert torch.equal(H.add_rowvec(x.cuda(), e.cuda(), B, T).cpu(), R.add32(x, e[:, None, :]))


AXPBY_SIZES = [8192 * 256 + 5, 1]


@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby_against_float64(H, n):
    g = R.gen(n % 1000)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = 0.37, -1.9
    ref = R.f32(a) * x.double() + R.f32(b) * y.double()
    within("axpby", f"n={n} a*x+b*y", max_err(H.axpby(x.cuda(), y.cuda(), a, b), ref), max_err(a * x + b * y, ref))
    ref = R.f32(a) * x.double()
    within("axpby", f"n={n} a*x", max_err(H.axpby(x.cuda(), None, a, 0.0), ref), max_err(a * x, ref))


@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby_mask_is_the_host_rule(H, n):
    """``Drop(0.25, seed, step)`` on a vector of ones: the factors are those of the host definition element for element,
    past the grid's first pass and through the last 5 elements, at two steps.  (This kernel is the mask oracle of the
    other dropout tests.)"""
    p, seed = 0.25, (1 << 41) + 0x5EED
    masks = []
    for step in (3, 11):
        st = torch.full((1,), step, dtype=torch.int64, device="cuda")
        got = H.axpby(torch.ones(n, device="cuda"), None, 1.0, 0.0, H.Drop(p, seed, st)).cpu()
        want = LR.drop_factors(p, seed, step, n)
        assert torch.equal(got, want)
        assert torch.equal(got[-5:], want[-5:])
        masks.append(want)
    if n > 1:
        assert 0.2 * n < int((masks[0] == 0).sum()) < 0.3 * n and not torch.equal(masks[0], masks[1])


# ---------------------------------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V,D", [(4099, 83, 384), (1, 2, 4)])
def test_embedding_forward(H, M, V, D):
    """Rows equal W[idx] bit for bit; indices -1, V and V + 100 read rows 0 and V - 1 (the clamp the kernel documents)."""
    g = R.gen(M + V)
    W = torch.randn(V, D, generator=g)
    idx = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    if M > 8:
        idx[5], idx[6], idx[7], idx[M - 1] = -1, V, V + 100, -1
    else:
        idx[0] = 1
    got = H.embedding_fwd(idx.cuda(), W.cuda()).cpu()
    assert got.shape == (M, D) and same_bits(got, W[idx.long().clamp(0, V - 1)])
    if M > 8:
        assert same_bits(got[5], W[0]) and same_bits(got[6], W[V - 1]) and same_bits(got[7], W[V - 1])


@pytest.mark.parametrize("M,V,D,padding_idx", [(4099, 83, 384, 0), (4099, 83, 384, -1), (37, 84, 8, 0), (37, 84, 8, -1),
                                               (25003, 84, 8, 0)])
def test_embedding_backward(H, M, V, D, padding_idx):
    """The one-hot GEMM against a float64 index_add; one index owns over a third of the rows (a sum of more than a thousand
    terms at M = 4099); rows never indexed and the padding row are exactly 0.  V = 84 needs no pad column.  The one-hot
    matrix of M = 25003 is past the 8192 x 256 elements of one pass of ``onehot_kernel``'s grid; the others are not."""
    assert H.get_precision() == "32-true"
    if M > 20000:
        assert M * ((V + 3) // 4 * 4) > 8192 * 256
    idx, never = R.skewed_indices(M, V)
    dy = torch.randn(M, D, generator=R.gen(M + D))
    dW = torch.empty(V, D, device="cuda")
    assert bool(torch.isnan(dW).all())
    H.embedding_bwd(idx.cuda(), dy.cuda(), dW, padding_idx=padding_idx)
    ref, scale = R.embedding_bwd64(idx, dy, V, padding_idx)
    W32 = torch.zeros(V, D, requires_grad=True)
    F.embedding(idx.long(), W32, padding_idx=padding_idx if padding_idx >= 0 else None).backward(dy)
    within("embedding dW", f"M={M} V={V} D={D} pad={padding_idx}", elem_err(dW, ref, scale),
           elem_err(W32.grad, ref, scale))
    assert bool((dW.cpu()[never] == 0).all())
    if padding_idx >= 0:
        assert int((idx == padding_idx).sum()) > 0 and bool((dW.cpu()[padding_idx] == 0).all())
    else:
        assert bool((dW.cpu()[0] != 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# bucketize + embedding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("D", [4, 384])
@pytest.mark.parametrize("NB", [1, 2, 255, 256])
def test_bucket_embed_add(H, NB, D, control):
    """Every edge and its fp32 neighbours, +-inf, NaN, points beyond both ends, quotients edge / control: ``idx`` is
    torch.bucketize's (NaN takes bucket NB), ``out`` exactly x + W[idx]."""
    bins = R.bucket_bins(NB)
    val = R.bucket_values(bins, control)
    M = val.numel()
    g = R.gen(NB + D)
    W, x = torch.randn(NB + 1, D, generator=g), torch.randn(M, D, generator=g)
    want_out, want_idx, _ = R.bucket_embed_add(val, control, bins, W, x)
    out, idx = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), control=control)
    nan = torch.isnan(val)
    assert int(nan.sum()) >= 2 and bool((want_idx[nan] == NB).all())
    assert idx.cpu()[nan].tolist() == [NB] * int(nan.sum()), "a NaN value takes the last bucket, as torch.bucketize"
    assert torch.equal(idx.cpu().long(), want_idx)
    assert torch.equal(out.cpu(), want_out)


@pytest.mark.parametrize("form", ["token", "utterance"])
def test_bucket_embed_add_tensor_control(H, form):
    """The device-control kernel's own search on the +-inf and NaN rows: a [B, Ts] control picked through ``ctl_idx`` with
    -1 and indices >= Ts (control exactly 1 there), and a per-utterance control."""
    B, T, Ts, D = 3, 41, 7, 8
    bins = R.bucket_bins(255)
    NB = bins.numel()
    g = R.gen(77)
    val = -4 + 8 * torch.rand(B, T, generator=g)
    val[:, 0], val[:, 1], val[:, 2], val[:, 3] = float("inf"), float("-inf"), float("nan"), float("nan")
    val[:, 4:24] = bins[torch.randint(0, NB, (B, 20), generator=g)]
    W, x = torch.randn(NB + 1, D, generator=g), torch.randn(B, T, D, generator=g)
    if form == "token":
        control = 0.5 + torch.rand(B, Ts, generator=g)
        ctl_idx = torch.randint(0, Ts, (B, T), generator=g, dtype=torch.int32)
        ctl_idx[:, 2], ctl_idx[0, 0], ctl_idx[1, 1], ctl_idx[1, 10], ctl_idx[2, 20] = -1, Ts, -1, Ts + 5, -1
        c = R.control_of_rows(control, ctl_idx)
        assert int((c == 1).sum()) >= 7
        got = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), control=control.cuda(),
                                 ctl_idx=ctl_idx.cuda(), scaled=True)
    else:
        control = 0.5 + torch.rand(B, generator=g)
        c = control[:, None].expand(B, T)
        got = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), control=control.cuda(), scaled=True)
    want_out, want_idx, want_scaled = R.bucket_embed_add(val, c, bins, W, x)
    out, idx, scaled = (t.cpu() for t in got)
    nan = torch.isnan(val)
    assert bool((idx[nan] == NB).all()), "a NaN value takes the last bucket, as torch.bucketize"
    assert bool((idx[:, 0] == NB).all()) and bool((idx[:, 1] == 0).all())
    assert torch.equal(idx.long(), want_idx) and torch.equal(out, want_out)
    assert torch.equal(torch.isnan(scaled), nan) and torch.equal(scaled[~nan], want_scaled[~nan])


# ---------------------------------------------------------------------------------------------------------------------
# length regulator
# ---------------------------------------------------------------------------------------------------------------------
class LRCase:
    def __init__(self, B, Ts, Tm, D):
        self.shape, self.tag = (B, Ts, Tm, D), f"B={B} Ts={Ts} Tm={Tm} D={D}"
        g = R.gen(B + Ts + Tm + D)
        self.dur = R.lr_durations(B, Ts, Tm)
        self.x, self.table = torch.randn(B, Ts, D, generator=g), torch.randn(Tm + 3, D, generator=g)
        self.dy = torch.randn(B, Tm, D, generator=g)
        self.plain = R.length_regulate(self.x, self.dur, Tm)
        self.tabled = R.length_regulate(self.x, self.dur, Tm, self.table)


@pytest.fixture(scope="module", params=R.LR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def lrcase(request):
    return LRCase(*request.param)


@pytest.mark.parametrize("with_table", [False, True])
def test_length_regulator_forward(H, lrcase, with_table):
    """``out``, ``cum``, ``lens`` and ``src_idx`` are exact, frames past the total exactly 0, and ``duration_cumsum``
    gives the same ``cum`` and ``lens``."""
    c = lrcase
    B, Ts, Tm, D = c.shape
    want_out, want_cum, want_lens, want_src = c.tabled if with_table else c.plain
    out, cum, lens, src = H.length_regulate_fwd(c.x.cuda(), c.dur.cuda(), Tm, table=c.table.cuda() if with_table else None,
                                                want_src_idx=True)
    assert torch.equal(cum.cpu(), want_cum) and torch.equal(lens.cpu(), want_lens)
    assert torch.equal(src.cpu(), want_src)
    assert torch.equal(out.cpu(), want_out)
    past = want_src < 0
    assert same_bits(out.cpu()[past], torch.zeros(int(past.sum()), D))
    out3 = H.length_regulate_fwd(c.x.cuda(), c.dur.cuda(), Tm, table=c.table.cuda() if with_table else None)
    assert len(out3) == 3 and torch.equal(out3[0], out)
    cum2, lens2 = H.duration_cumsum(c.dur.cuda(), Tm)
    assert torch.equal(cum2.cpu(), want_cum) and torch.equal(lens2.cpu(), want_lens)


def test_length_regulator_backward(H, lrcase):
    """Segment sums of dy against float64 (the longest token sums 600 frames in sequence); gradients of zero-duration
    tokens and of tokens wholly past Tm are exactly 0."""
    c = lrcase
    B, Ts, Tm, D = c.shape
    _, cum, _, src = c.plain
    dx = H.length_regulate_bwd(c.dy.cuda(), cum.cuda())
    ref, scale = R.length_regulate_bwd64(c.dy, src, Ts)
    xr = c.x.clone().requires_grad_(True)
    pos = c.dur.long().clamp(min=0)
    outs = [torch.repeat_interleave(xr[b], pos[b], dim=0)[:Tm] for b in range(B)]
    torch.autograd.backward(outs, [c.dy[b, : o.shape[0]] for b, o in enumerate(outs)])
    within("regulator dx", c.tag, elem_err(dx, ref, scale), elem_err(xr.grad, ref, scale))
    start = cum.long() - pos
    silent = (pos == 0) | (start >= Tm)
    if B > 1:
        assert int(silent.sum()) > 0 and int((start >= Tm).sum()) > 0
    assert same_bits(dx.cpu()[silent], torch.zeros(int(silent.sum()), D))


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------
def one_ulp(got, want64):
    """``got`` (fp32) within one fp32 ulp of the float64 value rounded to fp32."""
    want = np.float32(want64)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("n,config", [(n, c) for n in R.OPT_SIZES for c in range(len(R.OPT_CONFIGS))
                                      if not (n > 1 << 20 and c == 2)],
                         ids=lambda v: str(v))
def test_optimizer(H, n, config):
    """Twelve steps of step_advance + grad_clip_coef + adamw_step over a rising, peaking and decaying rate, against the
    float64 restatement: the state record after every step, ``m``, ``v`` and the displacement p - p0 after the last."""
    max_norm, grad_scale = R.OPT_CONFIGS[config]
    o, tag = R.OPT, f"n={n} max_norm={max_norm} grad_scale={grad_scale}"
    size = " large" if n > 1 << 20 else ""
    p0 = R.opt_params(n)
    ref = R.Optimizer64(p0, max_norm=max_norm, grad_scale=grad_scale, **o)
    pt = p0.clone().requires_grad_(True)  # the yardstick: PyTorch in fp32 on the CPU, the same fp32 hyperparameters
    opt = torch.optim.AdamW([pt], ref.base_lr, betas=(ref.b1, ref.b2), eps=ref.eps, weight_decay=ref.wd)
    p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    st = H.new_step_state("cuda")
    for k in range(1, R.OPT_STEPS + 1):
        g = R.opt_grad(n, k)
        rec = ref.step(g)
        for grp in opt.param_groups:
            grp["lr"] = R.noam_lr(ref.base_lr, o["warmup"], k)
        pt.grad = g * grad_scale
        norm32, coef32 = float(pt.grad.norm()), grad_scale
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([pt], max_norm)
            norm32, coef32 = float(total), float(torch.clamp(max_norm / (total + 1e-6), max=1.0)) * grad_scale
        opt.step()
        gd = g.cuda()
        H.step_advance(st, o["base_lr"], o["warmup"], *o["betas"])
        H.grad_clip_coef(gd, max_norm, grad_scale, st)
        H.adamw_step(p, gd, m, v, st, *o["betas"], o["eps"], o["weight_decay"])
        word = st.cpu()
        f = word.view(torch.float32)
        assert int(word[0]) == k == rec["step"]
        for name, i in (("lr", 2), ("bc1", 3), ("bc2", 4)):
            assert one_ulp(f[i], rec[name]), f"{tag} step {k} {name}: {float(f[i])!r} against {rec[name]!r}"
        within("grad_norm" + size, f"{tag} step {k}", rel_err(f[6], rec["grad_norm"]), rel_err(norm32, rec["grad_norm"]))
        within("clip_coef" + size, f"{tag} step {k}", rel_err(f[5], rec["clip_coef"]), rel_err(coef32, rec["clip_coef"]))
        if R.opt_grad_kind(k) == "zero":
            assert float(f[6]) == 0.0
            for t in (p, m, v):
                assert bool(torch.isfinite(t).all()), f"{tag}: non-finite after the zero-gradient step"
    state = opt.state[pt]
    p0d = p0.double()
    within("m" + size, tag, max_err(m, ref.m), max_err(state["exp_avg"], ref.m))
    within("v" + size, tag, max_err(v, ref.v), max_err(state["exp_avg_sq"], ref.v))
    within("displacement" + size, tag, max_err(p.cpu().double() - p0d, ref.p - p0d), max_err(pt.detach().double() - p0d, ref.p - p0d))


def test_optimizer_refuses_a_misaligned_gradient(H):
    g = torch.randn(1028, generator=R.gen(1)).cuda()
    st = H.new_step_state("cuda")
    before = st.clone()
    assert g.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match="invalid arguments"):
        H.grad_clip_coef(g[1:], 1.0, 1.0, st)
    torch.cuda.synchronize()
    assert torch.equal(st, before)
    H.grad_clip_coef(g[4:], 1.0, 1.0, st)
    assert rel_err(st.cpu().view(torch.float32)[6], float(g[4:].double().norm())) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# refusals: FS2HIP_EINVAL before any launch, outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_wrappers(H):
    """A width that is no multiple of 4 (an odd one for the table) raises through every wrapper."""
    dev = "cuda"
    x6, lens, idx = torch.zeros(2, 3, 6, device=dev), torch.ones(2, dtype=torch.int32, device=dev), \
        torch.zeros(2, 3, dtype=torch.int32, device=dev)
    bad = "invalid arguments"
    with pytest.raises(RuntimeError, match=bad):
        H.posenc_table(torch.ones(3, device=dev), 4, 7)
    with pytest.raises(RuntimeError, match=bad):
        H.add_posenc(x6, torch.zeros(3, 6, device=dev), lens, 2, 3)
    with pytest.raises(RuntimeError, match=bad):
        H.embedding_fwd(idx, torch.zeros(5, 6, device=dev))
    val, bins, W = torch.zeros(2, 3, device=dev), torch.zeros(3, device=dev), torch.zeros(4, 6, device=dev)
    with pytest.raises(RuntimeError, match=bad):
        H.bucket_embed_add(val, bins, W, x6)
    with pytest.raises(RuntimeError, match=bad):
        H.bucket_embed_add(val, bins, W, x6, control=torch.ones(2, device=dev))
    with pytest.raises(RuntimeError, match=bad):
        H.length_regulate_fwd(x6, idx, 5)
    with pytest.raises(RuntimeError, match=bad):
        H.length_regulate_bwd(torch.zeros(2, 5, 6, device=dev), idx)
    with pytest.raises(RuntimeError, match=bad):  # no rows at all
        H.embedding_fwd(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(5, 8, device=dev))


def test_non_positive_sizes_raise_through_the_wrappers(H):
    """No utterances, no frames, no tokens, no rows, no edges, no elements: every wrapper raises, either on its own shape
    check or on the entry point's refusal."""
    dev = "cuda"
    f = lambda *shape: torch.zeros(*shape, device=dev)
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    st = H.new_step_state(dev)
    calls = {
        "posenc_table T = 0": lambda: H.posenc_table(f(3), 0, 6),
        "posenc_table D = 0": lambda: H.posenc_table(f(0), 4, 0),
        "add_posenc B = 0": lambda: H.add_posenc(f(0, 3, 8), f(3, 8), i(0), 0, 3),
        "add_posenc T = 0": lambda: H.add_posenc(f(2, 0, 8), f(3, 8), i(2), 2, 0),
        "add_rowvec B = 0": lambda: H.add_rowvec(f(0, 3, 8), f(0, 8), 0, 3),
        "add_rowvec T = 0": lambda: H.add_rowvec(f(2, 0, 8), f(2, 8), 2, 0),
        "axpby n = 0": lambda: H.axpby(f(0), f(0)),
        "embedding_fwd M = 0": lambda: H.embedding_fwd(i(0), f(5, 8)),
        "embedding_fwd V = 0": lambda: H.embedding_fwd(i(2, 3), f(0, 8)),
        "embedding_bwd M = 0": lambda: H.embedding_bwd(i(0), f(0, 8), f(5, 8)),
        "bucket_embed_add M = 0": lambda: H.bucket_embed_add(f(0), f(3), f(4, 8), f(0, 8)),
        "bucket_embed_add NB = 0": lambda: H.bucket_embed_add(f(2, 3), f(0), f(1, 8), f(2, 3, 8)),
        "bucket_embed_add, tensor control, B = 0": lambda: H.bucket_embed_add(f(0, 3), f(3), f(4, 8), f(0, 3, 8),
                                                                              control=f(1) + 1),
        "bucket_embed_add, tensor control, NB = 0": lambda: H.bucket_embed_add(f(2, 3), f(0), f(1, 8), f(2, 3, 8),
                                                                               control=f(2) + 1),
        "length_regulate_fwd B = 0": lambda: H.length_regulate_fwd(f(0, 3, 8), i(0, 3), 5),
        "length_regulate_fwd Ts = 0": lambda: H.length_regulate_fwd(f(2, 0, 8), i(2, 0), 5),
        "length_regulate_fwd Tm = 0": lambda: H.length_regulate_fwd(f(2, 3, 8), i(2, 3), 0),
        "length_regulate_fwd Tm < 0": lambda: H.length_regulate_fwd(f(2, 3, 8), i(2, 3), -4),
        "length_regulate_bwd B = 0": lambda: H.length_regulate_bwd(f(0, 5, 8), i(0, 3)),
        "length_regulate_bwd Tm = 0": lambda: H.length_regulate_bwd(f(2, 0, 8), i(2, 3)),
        "length_regulate_bwd Ts = 0": lambda: H.length_regulate_bwd(f(2, 5, 8), i(2, 0)),
        "duration_cumsum B = 0": lambda: H.duration_cumsum(i(0, 3), 5),
        "duration_cumsum Ts = 0": lambda: H.duration_cumsum(i(2, 0), 5),
        "grad_clip_coef n = 0": lambda: H.grad_clip_coef(f(0), 1.0, 1.0, st),
        "adamw_step n = 0": lambda: H.adamw_step(f(0), f(0), f(0), f(0), st, 0.9, 0.98, 1e-8, 0.01),
    }
    before = st.clone()
    for what, call in calls.items():
        with pytest.raises((RuntimeError, ValueError), match="fs2hip"):
            call()
            pytest.fail(f"{what}: accepted")
    torch.cuda.synchronize()
    assert torch.equal(st, before)


def test_refusals_leave_the_outputs_untouched(H):
    """Widths that are no multiple of 4, an odd table width and non-positive sizes, straight at the entry points: each
    returns FS2HIP_EINVAL and writes nothing.  (Every buffer would hold the largest shape named here.)"""
    L, s = H.lib(), H._stream()
    n = 4096
    fin, iin = torch.ones(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    fo = [torch.full((n,), float("nan"), device="cuda") for _ in range(4)]
    io = [torch.full((n,), POISON_INT, dtype=torch.int32, device="cuda") for _ in range(3)]
    st = H.new_step_state("cuda")
    st0 = st.clone()
    F_, I_, S_ = fin.data_ptr(), iin.data_ptr(), st.data_ptr()
    O0, O1, O2, O3 = (t.data_ptr() for t in fo)
    J0, J1, J2 = (t.data_ptr() for t in io)
    calls = []

    def each(name, fn, good, bads):
        """``good``: a valid size tuple; every entry of ``bads`` replaces some of its members."""
        for what, repl in bads:
            args = list(good)
            for pos, val in repl.items():
                args[pos] = val
            calls.append((f"{name}: {what}", fn, args))

    each("posenc_table", lambda T, D: L.fs2hip_posenc_table(F_, O0, T, D, s), (4, 6),
         [("odd D", {1: 7}), ("T = 0", {0: 0}), ("T < 0", {0: -1}), ("D = 0", {1: 0})])
    each("add_posenc", lambda B, T, D: L.fs2hip_add_posenc(F_, F_, I_, O0, B, T, D, s), (2, 3, 8),
         [("D = 6", {2: 6}), ("B = 0", {0: 0}), ("T = 0", {1: 0}), ("D = 0", {2: 0}), ("T < 0", {1: -3})])
    each("embedding_fwd", lambda M, V, D: L.fs2hip_embedding_fwd(I_, F_, O0, M, V, D, s), (4, 5, 8),
         [("D = 6", {2: 6}), ("M = 0", {0: 0}), ("V = 0", {1: 0}), ("D = 0", {2: 0}), ("M < 0", {0: -4})])
    each("onehot", lambda M, Vp: L.fs2hip_onehot(I_, O0, M, Vp, -1, s), (4, 8),
         [("Vp = 6", {1: 6}), ("M = 0", {0: 0}), ("Vp = 0", {1: 0})])
    each("bucket_embed_add", lambda M, NB, D: L.fs2hip_bucket_embed_add(F_, 1.0, F_, NB, F_, F_, O0, J0, M, D, s),
         (4, 3, 8), [("D = 6", {2: 6}), ("M = 0", {0: 0}), ("NB = 0", {1: 0}), ("D = 0", {2: 0})])
    each("bucket_embed_add_ctl",
         lambda M, NB, D, div, ctl, cidx, cT: L.fs2hip_bucket_embed_add_ctl(F_, ctl, div, cidx, cT, F_, NB, F_, F_, O0, J0,
                                                                            O1, M, D, s),
         (4, 3, 8, 2, F_, None, 0),
         [("D = 6", {2: 6}), ("M = 0", {0: 0}), ("NB = 0", {1: 0}), ("D = 0", {2: 0}), ("ctl_div = 0", {3: 0}),
          ("M % ctl_div", {3: 3}), ("no control", {4: None}), ("ctl_idx without ctl_T", {5: I_, 6: 0})])
    each("length_regulate_fwd",
         lambda B, Ts, Tm, D: L.fs2hip_length_regulate_fwd(F_, I_, None, O0, J0, J1, J2, B, Ts, Tm, D, s), (2, 3, 5, 8),
         [("D = 6", {3: 6}), ("B = 0", {0: 0}), ("Ts = 0", {1: 0}), ("Tm = 0", {2: 0}), ("D = 0", {3: 0})])
    each("length_regulate_bwd", lambda B, Ts, Tm, D: L.fs2hip_length_regulate_bwd(F_, I_, O0, B, Ts, Tm, D, s),
         (2, 3, 5, 8), [("D = 6", {3: 6}), ("B = 0", {0: 0}), ("Ts = 0", {1: 0}), ("Tm = 0", {2: 0}), ("D = 0", {3: 0})])
    each("duration_cumsum",
         lambda B, Ts, expect: L.fs2hip_duration_cumsum(I_, J0, J1, expect, None, None, B, Ts, 5, s), (2, 3, None),
         [("B = 0", {0: 0}), ("Ts = 0", {1: 0}), ("expect without mismatch", {2: I_})])
    each("grad_clip_coef", lambda n_, ptr: L.fs2hip_grad_clip_coef(ptr, n_, 1.0, 1.0, O0, S_, s), (8, F_),
         [("n = 0", {0: 0}), ("n < 0", {0: -8}), ("gradient 4 bytes off", {1: F_ + 4})])
    each("adamw_step", lambda n_: L.fs2hip_adamw_step(O0, F_, O1, O2, n_, S_, 0.9, 0.98, 1e-8, 0.01, s), (8,),
         [("n = 0", {0: 0}), ("n < 0", {0: -8})])
    each("axpby", lambda n_: L.fs2hip_axpby(F_, None, O0, n_, 1.0, 1.0, 0.0, 0, None, s), (8,),
         [("n = 0", {0: 0}), ("n < 0", {0: -8})])
    each("add_rowvec", lambda B, T, D: L.fs2hip_add_rowvec(F_, F_, O0, B, T, D, s), (2, 3, 6),
         [("B = 0", {0: 0}), ("T = 0", {1: 0}), ("D = 0", {2: 0})])
    assert F_ % 16 == 0 and len(calls) > 50
    for what, fn, args in calls:
        assert fn(*args) == EINVAL, what
    torch.cuda.synchronize()
    for t in fo:
        assert bool(torch.isnan(t).all()), "a refused call wrote a float output"
    for t in io:
        assert bool((t == POISON_INT).all()), "a refused call wrote an integer output"
    assert torch.equal(st, st0)
