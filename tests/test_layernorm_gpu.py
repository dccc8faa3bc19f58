"""Kernel parity of the LayerNorm family (``csrc/norm.hip``): every entry point and template form, fp32 against a
float64 evaluation of the formula, the bf16-storage forms against the fp32 kernels on the same values, the fused dropout
against the mask's definition restated on the host (``tests/layernorm_references.py``), and the refusals.

Error measure (fp32 kernels).  Per row: max |got - ref64| over max |ref64| of THAT row (denominator floored at 1e-12),
then the worst row -- per row because the all-zero and constant rows of the ``relu`` data have rstd = eps^-0.5 = 316 and
would set a whole-tensor maximum that hides every other row.  Sums over rows (dgamma, dbeta, colsum(dz)) use the same
measure with a per-column scale, the sum of the magnitudes of the column's terms (a column sum itself may cancel to
nothing).  The yardstick is PyTorch's own fp32 CPU LayerNorm / autograd / column sum on the same inputs, measured the
same way against float64; a kernel passes with ``err <= MARGIN[kind] * torch_err + FLOOR``, nothing else.
A 64-lane butterfly and a sequential loop sum in different orders and neither is the better one, hence a margin;
FLOOR = 4 * 2^-23 (four fp32 ulps of the row scale) covers the cases where the yardstick happens to be exact.  The
backward's float64 reference takes the kernel's own saved mean / rstd (upcast), as the kernel does; the statistics are
checked on their own.  For ``fs2hip_layernorm_bwd_pred`` rows that keep fewer than two elements take the scale of the row
before relu' zeroes it (see the test); every other row is measured against its own kept elements.

Measured on an MI355X over all eleven shapes: the worst kernel error, the worst PyTorch-fp32 error, and the worst ratio
kernel / PyTorch among the checks where the kernel is off by more than one ulp (2^-23) of the scale:

  data kind   quantity                         kernel    PyTorch   worst ratio
  randn       y, y * mask                      2.2e-07   2.8e-07   1.08
  randn       mean, rstd                       1.5e-07   1.7e-07   1.00
  randn       dx, dx + add, predictor dx       2.4e-07   7.8e-07   1.07
  randn       dgamma, dbeta, colsum(dz)        1.4e-07   1.9e-07   0.83
  offset      y, y * mask                      4.6e-05   6.8e-05   4.08  (M = 5; 3.1 at M = 7; below 1 from M = 9 on)
  offset      mean, rstd                       1.8e-07   2.7e-05   0.93
  offset      dx, dx + add, predictor dx       2.2e-07   1.8e-04   0.04  (PyTorch's figure carries its statistics' error)
  offset      dgamma, dbeta, colsum(dz)        1.6e-07   8.5e-04   0.00
  relu        y, y * mask                      3.1e-07   3.5e-07   1.38
  relu        mean, rstd                       2.0e-07   2.0e-07   1.02
  relu        dx, dx + add, predictor dx       4.5e-07   4.5e-07   1.23
  relu        dgamma, dbeta, colsum(dz)        1.6e-07   3.1e-06   1.26
  tiny        y, y * mask                      1.1e-07   1.2e-07   -
  tiny        mean, rstd                       9.9e-08   1.2e-07   -
  tiny        dx, dx + add, predictor dx       2.2e-07   2.9e-07   1.10
  tiny        dgamma, dbeta, colsum(dz)        1.6e-07   1.3e-06   1.33
  bf16 forms  colsum(dz), randn / relu         1.6e-07   2.1e-07   0.96 / 1.24

Chosen from them: FLOOR = 4 * 2^-23 = 4.8e-07 and MARGIN = 2.0 (randn), 2.5 (relu, tiny), 6.0 (offset) -- each at most
about twice the kind's worst ratio.  Every kernel error above is below FLOOR except y of the ``offset`` rows, which is
one rounding of a mean near 1000 (ulp 6.1e-05) and is held by the 6.0 margin alone.  Measured against their own kept
element, single-positive-element ReLU rows at C = 64 read 3.8e-02 (kernel) against 4.2e-03 .. 1.9e-02 (PyTorch) in the
predictor backward: an analytically zero gradient, noise against noise.

Which test launches which (entry point, template form); every one at NCH = 1, 2 and 4 (C <= 256, <= 512, <= 1024):

  fs2hip_layernorm_fwd       ln_fwd<N, YB=0, DROP=0>              test_forward_fp32
  fs2hip_layernorm_fwd_drop  ln_fwd<N, 0, DROP=1>                 test_forward_dropout_fp32
  fs2hip_layernorm_fwd_b     ln_fwd<N, YB=1>                      test_bf16_forward, test_bf16_rounds_to_nearest_even
  fs2hip_layernorm_bwd       ln_bwd<N, DZ=0>                      test_backward_fp32
  fs2hip_layernorm_bwd_dz    ln_bwd<N, DZ=1>                      test_backward_second_output_fp32
  fs2hip_layernorm_bwd_pred  ln_bwd<N, PRED=1, XOB=0>             test_backward_predictor_fp32
  fs2hip_layernorm_bwd_pred  ln_bwd<N, PRED=1, XOB=1>             test_bf16_predictor
  fs2hip_layernorm_bwd_x     ln_bwd<N, DZ=0, DYB=1>               test_bf16_dy_backward
  fs2hip_layernorm_bwd_x     ln_bwd<N, DZ=1, DYB=0|1, ZB=0|1>     test_bf16_second_output (flags 1, 2, 3)
  fs2hip_layernorm_bwd_x     ln_bwd<N, DZ=0|1, DYB=0, ZB=0>       test_bwd_x_fp32_forms_are_the_fp32_entry_points
  rows per workgroup 8 / 16 / 32                                  M = 4096 / 4097, 16384 / 16385 of the fp32 tests,
                                                                  test_backward_row_count_thresholds
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import layernorm_references as R

pytestmark = pytest.mark.gpu

EPS = 1e-5
DEN_FLOOR = 1e-12
FLOOR = 4 * 2.0 ** -23
#: per data kind, at most about twice the worst ratio measured (module docstring)
MARGIN = {"randn": 2.0, "offset": 6.0, "relu": 2.5, "tiny": 2.5}


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    hip.lib()
    return hip


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    """Every floating ``torch.empty`` / ``torch.empty_like`` on the GPU comes back as NaN while a test of this file runs
    (the wrappers allocate their results that way): an element a kernel skips is a NaN, not whatever an earlier,
    identical call left in the block the allocator hands out again."""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.is_floating_point() and t.numel():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: poisoned(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poisoned(real_empty_like(*a, **k)))


# ---------------------------------------------------------------------------------------------------------------------
# measure
# ---------------------------------------------------------------------------------------------------------------------
def row_err(got, ref64, den=None):
    """Worst row of max |got - ref64| / max |ref64| per row (``den``: the per-row scales, where they are not all the
    reference's own row maxima)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    den = (ref64.abs().amax(-1) if den is None else den).clamp_min(DEN_FLOOR)
    return float(((got - ref64).abs().amax(-1) / den).max())


def vec_err(got, ref64, scale64):
    """Per element of a vector (statistics: one per row; column sums: one per column), each with its own scale."""
    got = got.detach().cpu().double().reshape(-1)
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    return float(((got - ref64).abs() / scale64.clamp_min(DEN_FLOOR)).max())


def within(what, c, err, yard, tag=None):
    """The kernel's error against the yardstick's; prints the figures first (``pytest -s`` keeps them)."""
    tag = tag or c.tag
    print(f"LNFIG {tag} {what} kernel {err:.3e} torch {yard:.3e} ratio {err / max(yard, 1e-300):.2f}")
    assert err <= MARGIN[c.kind] * yard + FLOOR, \
        f"{tag} {what}: kernel error {err:.3e}, PyTorch fp32 error {yard:.3e}, margin {MARGIN[c.kind]}"


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 4),          # one active lane
          (5, 252),        # 63 lanes
          (9, 260),        # one lane in the second chunk
          (33, 516),       # three chunks on the NCH = 4 instance
          (7, 768),
          (13, 1024),      # widest row
          (4096, 64),      # last 8-row case
          (4097, 64),      # first 16-row case; the last workgroup holds one row
          (16384, 64),     # last 16-row case
          (16385, 64),     # first 32-row case
          (16385, 256)]    # 32-row case at the model's width
KINDS = ["randn", "offset", "relu", "tiny"]
BF16_SHAPES = [(5, 252), (9, 260), (7, 768), (13, 1024), (4097, 64), (16385, 256)]
ROWS_PER_WG = {4096: 8, 4097: 16, 16384: 16, 16385: 32}


def make_x(kind, M, C, g):
    if kind == "randn":
        return torch.randn(M, C, generator=g)
    if kind == "offset":  # the residual stream: a per-row offset of 10 .. 1000 either way, unit spread
        mag = 10.0 ** (1 + 2 * torch.rand(M, generator=g))
        mag[M // 2] = 1000.0
        sign = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
        return torch.randn(M, C, generator=g) + (sign * mag)[:, None]
    if kind == "relu":    # what the variance predictors normalise: ReLU outputs, dead rows, a saturated row
        x = torch.relu(torch.randn(M, C, generator=g) - 1.5)
        for r in {0, M // 2, M - 1}:
            x[r] = 0.0
        if M >= 5:
            # 1.5 * k is exact in fp32 for every k <= 1024: the row's mean is exactly 1.5 and its variance exactly 0 in any
            # summation order, so y = beta and rstd = eps^-0.5 are the same question for the kernel and the yardstick
            x[1] = 1.5
        return x
    if kind == "tiny":    # eps dominates the variance
        return 1e-3 * torch.randn(M, C, generator=g)
    raise ValueError(kind)


def torch_bwd(x, gamma, beta, dy):
    """PyTorch's fp32 CPU LayerNorm backward (autograd): dx, dgamma, dbeta."""
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    F.layer_norm(xr, (x.shape[-1],), gr, br, EPS).backward(dy)
    return xr.grad, gr.grad, br.grad


class Case:
    def __init__(self, M, C, kind):
        self.M, self.C, self.kind, self.tag = M, C, kind, f"{kind} M={M} C={C}"
        g = torch.Generator().manual_seed(100003 * KINDS.index(kind) + 1031 * C + M)
        self.x = make_x(kind, M, C, g)
        self.gamma, self.beta = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
        self.dy, self.add = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
        self.y64, self.mean64, self.rstd64 = R.ln_fwd64(self.x, self.gamma, self.beta, EPS)
        y32, mean32, rstd32 = torch.native_layer_norm(self.x, (C,), self.gamma, self.beta, EPS)
        self.y32, self.mean32, self.rstd32 = y32, mean32.reshape(-1), rstd32.reshape(-1)
        self.xmax = self.x.double().abs().amax(-1)
        self.d = {k: getattr(self, k).cuda() for k in ("x", "gamma", "beta", "dy", "add")}
        self._stats = None

    def stats(self, H):
        """The kernel's own saved statistics (device fp32) and their upcast copies for ``ln_bwd64``."""
        if self._stats is None:
            _, mean, rstd = H.layernorm_fwd(self.d["x"], self.d["gamma"], self.d["beta"], EPS)
            self._stats = (mean, rstd, mean.cpu().double(), rstd.cpu().double())
        return self._stats

    def yard_bwd(self, dy):
        """Errors of PyTorch's fp32 backward against float64 with exact statistics: (dx, dgamma, dbeta) and the column
        scales of dgamma / dbeta."""
        dx32, dg32, db32 = torch_bwd(self.x, self.gamma, self.beta, dy)
        dx64, dg64, db64 = R.ln_bwd64(dy, self.x, self.gamma, self.mean64, self.rstd64)
        xh = (self.x.double() - self.mean64[:, None]) * self.rstd64[:, None]
        sg, sb = (dy.double() * xh).abs().sum(0), dy.double().abs().sum(0)
        return row_err(dx32, dx64), vec_err(dg32, dg64, sg), vec_err(db32, db64, sb), dx32


@pytest.fixture(scope="module", params=[(M, C, k) for (M, C) in SHAPES for k in KINDS],
                ids=lambda p: f"{p[0]}x{p[1]}-{p[2]}")
def case(request):
    return Case(*request.param)


def check_param_sums(c, what, dgamma, dbeta, dy, mean_d, rstd_d, yard_g, yard_b):
    """dgamma / dbeta of the kernel against float64 sums taken with the kernel's statistics."""
    xh = (c.x.double() - mean_d[:, None]) * rstd_d[:, None]
    d = dy.double()
    within(what + " dgamma", c, vec_err(dgamma, (d * xh).sum(0), (d * xh).abs().sum(0)), yard_g)
    within(what + " dbeta", c, vec_err(dbeta, d.sum(0), d.abs().sum(0)), yard_b)


def nan_vecs(C, n):
    return [torch.full((C,), float("nan"), device="cuda") for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the mask's definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [None, 0, 7])
@pytest.mark.parametrize("seed", [31337, (1 << 40) + 0x9E3779B9])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_is_the_stated_rule(H, p, seed, step):
    """``fs2hip_axpby`` over ones with a Drop record gives exactly the factors of the rule in ``csrc/common.h`` (and
    ``include/fs2hip.h``), restated in NumPy: stored seeds reproduce their masks."""
    n = 4 * 1024 + 4
    st = None if step is None else torch.full((1,), step, dtype=torch.int64, device="cuda")
    got = H.axpby(torch.ones(n, device="cuda"), None, 1.0, 0.0, H.Drop(p, seed, st))
    want = R.drop_factors(p, seed, step, n)
    assert 0 < int((want == 0).sum()) < n
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fp32 kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sorted(ROWS_PER_WG) + [16385 + 1024])
def test_backward_row_count_thresholds(H, M):
    """The row counts of the fp32 cases really select the 8-, 16- and 32-row branches of the backward."""
    if os.environ.get("FS2_LN_BWD_ROWS"):
        pytest.skip("FS2_LN_BWD_ROWS forces one row count for every M: the thresholds are not in force")
    rows = ROWS_PER_WG.get(M, 32)
    assert H.lib().fs2hip_layernorm_bwd_blocks(M) == -(-M // rows)


def test_forward_fp32(H, case):
    c = case
    y, mean, rstd = H.layernorm_fwd(c.d["x"], c.d["gamma"], c.d["beta"], EPS)
    within("y", c, row_err(y, c.y64), row_err(c.y32, c.y64))
    within("mean", c, vec_err(mean, c.mean64, c.xmax), vec_err(c.mean32, c.mean64, c.xmax))
    within("rstd", c, vec_err(rstd, c.rstd64, c.rstd64), vec_err(c.rstd32, c.rstd64, c.rstd64))


def test_forward_dropout_fp32(H, case):
    """``fs2hip_layernorm_fwd_drop``: y = LayerNorm(x) * mask with the mask of the rule (element index row * C + c), the
    zeros exactly where the rule drops, the statistics those of the plain forward."""
    c = case
    p, seed, step = 0.3, (1 << 33) + 0x1234, 5
    st = torch.full((1,), step, dtype=torch.int64, device="cuda")
    f = R.drop_factors(p, seed, step, c.M * c.C).view(c.M, c.C)
    y0, mean0, rstd0 = H.layernorm_fwd(c.d["x"], c.d["gamma"], c.d["beta"], EPS)
    y, mean, rstd = H.layernorm_fwd_drop(c.d["x"], c.d["gamma"], c.d["beta"], H.Drop(p, seed, st), EPS)
    assert torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    assert torch.equal(y.cpu() == 0, (f == 0) | (y0.cpu() == 0))
    ym64 = c.y64 * f.double()
    within("y*mask", c, row_err(y, ym64), row_err(c.y32 * f, ym64))


def test_backward_fp32(H, case):
    """``fs2hip_layernorm_bwd``: immediate and deferred second stage, with and without the residual gradient."""
    c, d = case, case.d
    mean, rstd, mean_d, rstd_d = c.stats(H)
    yard_x, yard_g, yard_b, dx32 = c.yard_bwd(c.dy)
    dx64, _, _ = R.ln_bwd64(c.dy, c.x, c.gamma, mean_d, rstd_d)
    dg, db = nan_vecs(c.C, 2)
    dx = H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg, db)
    within("dx", c, row_err(dx, dx64), yard_x)
    check_param_sums(c, "bwd", dg, db, c.dy, mean_d, rstd_d, yard_g, yard_b)
    # the residual gradient joins after the LayerNorm arithmetic: the yardstick is PyTorch's dx + add in fp32
    dg2, db2 = nan_vecs(c.C, 2)
    dxa = H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg2, db2, dx_add=d["add"], defer=True)
    H.flush_grad_reductions()
    ref_a = dx64 + c.add.double()
    exact_a = R.ln_bwd64(c.dy, c.x, c.gamma, c.mean64, c.rstd64)[0] + c.add.double()
    within("dx+add", c, row_err(dxa, ref_a), row_err(dx32 + c.add, exact_a))
    # the same partial sums finished by the batched second stage: the same order, the same bits
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    dg3, db3 = nan_vecs(c.C, 2)
    assert torch.equal(H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg3, db3, dx_add=d["add"]), dxa)
    assert torch.equal(dg3, dg) and torch.equal(db3, db)
    dg4, db4 = nan_vecs(c.C, 2)
    dx4 = H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg4, db4, defer=True)
    H.flush_grad_reductions()
    assert torch.equal(dx4, dx) and torch.equal(dg4, dg) and torch.equal(db4, db)


def test_backward_second_output_fp32(H, case):
    """``fs2hip_layernorm_bwd_dz``: dx is the plain backward's; dz = dz_scale * mask * dx bit for bit on the kernel's own
    dx with the mask of the rule; colsum(dz) against a float64 sum of the dz the kernel wrote."""
    c, d = case, case.d
    mean, rstd, mean_d, rstd_d = c.stats(H)
    p, seed, step, scale = 0.3, 0xABCDEF, 3, 0.7
    st = torch.full((1,), step, dtype=torch.int64, device="cuda")
    f = R.drop_factors(p, seed, step, c.M * c.C).view(c.M, c.C)
    dg0, db0 = nan_vecs(c.C, 2)
    dx0 = H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg0, db0, dx_add=d["add"])
    dg, db, dzsum = nan_vecs(c.C, 3)
    dx, dz = H.layernorm_bwd(d["dy"], d["x"], d["gamma"], mean, rstd, dg, db, dx_add=d["add"], dz_scale=scale,
                             dz_drop=H.Drop(p, seed, st), dz_colsum=dzsum)
    H.flush_grad_reductions()
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    # the kernel's products in the kernel's order, in fp32: (dx * scale) * factor
    assert torch.equal(dz.cpu(), (dx.cpu() * torch.tensor(scale, dtype=torch.float32)) * f)
    z = dz.cpu()
    z64, zs = z.double().sum(0), z.double().abs().sum(0)
    within("colsum(dz)", c, vec_err(dzsum, z64, zs), vec_err(z.sum(0), z64, zs))


def test_backward_predictor_fp32(H, case):
    """``fs2hip_layernorm_bwd_pred``: dx = relu'(x) * LayerNormBackward(mask * dy), mask of the rule."""
    c, d = case, case.d
    mean, rstd, mean_d, rstd_d = c.stats(H)
    p, seed, step = 0.3, (1 << 35) + 99, 11
    st = torch.full((1,), step, dtype=torch.int64, device="cuda")
    f = R.drop_factors(p, seed, step, c.M * c.C).view(c.M, c.C)
    dym = f * c.dy                       # one fp32 product, as in the kernel
    pos = (c.x > 0)
    yard_x, yard_g, yard_b, dx32 = c.yard_bwd(dym)
    full_exact = R.ln_bwd64(dym, c.x, c.gamma, c.mean64, c.rstd64)[0]
    full64 = R.ln_bwd64(dym, c.x, c.gamma, mean_d, rstd_d)[0]
    exact, dx64 = full_exact * pos, full64 * pos
    dg, db = nan_vecs(c.C, 2)
    dx = H.layernorm_bwd_pred(d["dy"], d["x"], d["gamma"], mean, rstd, dg, db, H.Drop(p, seed, st))
    H.flush_grad_reductions()
    # The row scale is the issue's -- the largest kept element of the reference row -- except for rows that keep fewer
    # than two elements.  A ReLU row with a single positive element a normalises to the same vector for every a, so
    # the one gradient relu' keeps is analytically 0 up to eps / var: measured against itself such a row compares
    # rounding noise with rounding noise (4e-2 for the kernel, 2e-2 for PyTorch at C = 64).  Those rows take the scale
    # of the row BEFORE relu' zeroes it, which is what the kernel's rounding errors are proportional to.
    few = pos.sum(-1) < 2
    den = torch.where(few, full64.abs().amax(-1), dx64.abs().amax(-1))
    den_exact = torch.where(few, full_exact.abs().amax(-1), exact.abs().amax(-1))
    within("pred dx", c, row_err(dx, dx64, den), row_err(dx32 * pos, exact, den_exact))
    check_param_sums(c, "pred", dg, db, dym, mean_d, rstd_d, yard_g, yard_b)
    assert bool((dx.cpu()[~pos] == 0).all())
    if c.kind == "relu":  # dead rows: relu' = 0 everywhere, whatever rstd = 316 multiplies
        dead = (c.x == 0).all(-1)
        assert int(dead.sum()) >= 1 and bool((dx.cpu()[dead] == 0).all())
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. bf16 variants against the fp32 kernels on the same values (anchored to float64 at the same shapes above)
# ---------------------------------------------------------------------------------------------------------------------
class BCase:
    def __init__(self, H, M, C, kind):
        self.M, self.C, self.kind, self.tag = M, C, kind, f"bf16 {kind} M={M} C={C}"
        g = torch.Generator().manual_seed(7919 * C + M + KINDS.index(kind))
        self.x = make_x(kind, M, C, g).cuda()
        self.gamma, self.beta = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), torch.randn(C, generator=g).cuda()
        self.dy, self.add = torch.randn(M, C, generator=g).cuda(), torch.randn(M, C, generator=g).cuda()
        self.dy_b = self.dy.bfloat16()
        _, self.mean, self.rstd = H.layernorm_fwd(self.x, self.gamma, self.beta, EPS)


@pytest.fixture(scope="module", params=[(M, C, k) for (M, C) in BF16_SHAPES for k in ("randn", "relu")],
                ids=lambda p: f"{p[0]}x{p[1]}-{p[2]}")
def bcase(request, H):
    return BCase(H, *request.param)


def test_bf16_forward(H, bcase):
    b = bcase
    y32, mean32, rstd32 = H.layernorm_fwd(b.x, b.gamma, b.beta, EPS)
    yb, mean, rstd = H.layernorm_fwd(b.x, b.gamma, b.beta, EPS, out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, y32.bfloat16())
    assert torch.equal(mean, mean32) and torch.equal(rstd, rstd32)


def test_bf16_rounds_to_nearest_even(H):
    """gamma = 0 makes y = beta exactly; beta sits on bf16 ties (and one fp32 ulp either side), in both halves of a
    packed pair and both signs: the stored bits are those of round-to-nearest-even."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x3F800000, 0x3F828000,
            0x3F818000, 0x3F808000, 0xBF818000, 0xBF808000]
    want = [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0xBF82, 0x3F80, 0x3F82, 0x3F82, 0x3F80, 0xBF82, 0xBF80]
    C = len(bits)
    beta = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in bits], dtype=torch.int32).view(torch.float32)
    x = torch.randn(3, C, generator=torch.Generator().manual_seed(1)).cuda()
    gamma = torch.zeros(C, device="cuda")
    y32, _, _ = H.layernorm_fwd(x, gamma, beta.cuda(), EPS)
    assert torch.equal(y32.cpu(), beta.expand(3, C))
    yb, _, _ = H.layernorm_fwd(x, gamma, beta.cuda(), EPS, out_dtype=torch.bfloat16)
    got = yb.cpu().view(torch.int16).int() & 0xFFFF
    assert got.tolist() == [want] * 3


def test_bf16_dy_backward(H, bcase):
    """bf16 dy, no second output: what the fp32 kernel gives on the same values, bit for bit."""
    b = bcase
    dg32, db32, dg, db = nan_vecs(b.C, 4)
    dx32 = H.layernorm_bwd(b.dy_b.float(), b.x, b.gamma, b.mean, b.rstd, dg32, db32, dx_add=b.add, defer=True)
    dx = H.layernorm_bwd(b.dy_b, b.x, b.gamma, b.mean, b.rstd, dg, db, dx_add=b.add)
    H.flush_grad_reductions()
    assert dx.dtype == torch.float32 and torch.equal(dx, dx32)
    assert torch.equal(dg, dg32) and torch.equal(db, db32)
    dx_n = H.layernorm_bwd(b.dy_b, b.x, b.gamma, b.mean, b.rstd, dg, db)
    dx32_n = H.layernorm_bwd(b.dy_b.float(), b.x, b.gamma, b.mean, b.rstd, dg32, db32)
    H.flush_grad_reductions()
    assert torch.equal(dx_n, dx32_n) and torch.equal(dg, dg32) and torch.equal(db, db32)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bf16_second_output(H, bcase, p):
    """The second-output backward with bf16 on either side, all four (dy, dz) type combinations: dx, dgamma, dbeta and an
    fp32 dz are the fp32 path's bits on the same values, a bf16 dz is the fp32 dz rounded once, and colsum(dz) is the
    sum of the ROUNDED values the kernel wrote."""
    b = bcase
    scale = 0.7
    st = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    drop = H.Drop(p, 0x51F15EED, st) if p else H.NO_DROP
    for dyb in (False, True):
        dy32 = b.dy_b.float() if dyb else b.dy
        dg32, db32, zs32 = nan_vecs(b.C, 3)
        dx32, dz32 = H.layernorm_bwd(dy32, b.x, b.gamma, b.mean, b.rstd, dg32, db32, dx_add=b.add, dz_scale=scale,
                                     dz_drop=drop, dz_colsum=zs32)
        H.flush_grad_reductions()
        for zb in (False, True):
            what = f"{b.tag} p={p} dy {'bf16' if dyb else 'fp32'} dz {'bf16' if zb else 'fp32'}"
            dg, db, zs = nan_vecs(b.C, 3)
            dx, dz = H.layernorm_bwd(b.dy_b if dyb else b.dy, b.x, b.gamma, b.mean, b.rstd, dg, db, dx_add=b.add,
                                     dz_scale=scale, dz_drop=drop, dz_colsum=zs,
                                     dz_dtype=torch.bfloat16 if zb else torch.float32)
            H.flush_grad_reductions()
            assert torch.equal(dx, dx32), what
            assert torch.equal(dg, dg32) and torch.equal(db, db32), what
            assert dz.dtype == (torch.bfloat16 if zb else torch.float32), what
            assert torch.equal(dz, dz32.bfloat16() if zb else dz32), what
            # Against the values as WRITTEN.  |dz| ~ 1 here (scale 0.7, gamma ~ 1, unit dy), so one bf16 rounding moves an
            # element by up to 2^-9: a column sum of the unrounded values differs from this reference by about
            # 2^-9 * sqrt(M) * |dz| (0.1 at M = 4097, 0.2 at M = 16385) where the fp32 summation error of either
            # order is below 1e-3 -- a kernel that accumulated before rounding fails at every shape here.
            z = dz.float().cpu()
            z64, zabs = z.double().sum(0), z.double().abs().sum(0)
            within("colsum(dz)", b, vec_err(zs, z64, zabs), vec_err(z.sum(0), z64, zabs), tag=what)


def test_bwd_x_fp32_forms_are_the_fp32_entry_points(H, bcase):
    """``fs2hip_layernorm_bwd_x`` with flags = 0 (fp32 dy, fp32 dz or none): the forms no wrapper reaches."""
    b = bcase
    L, s, C = H.lib(), H._stream(), b.C
    nblk = L.fs2hip_layernorm_bwd_blocks(b.M)
    st = torch.full((1,), 2, dtype=torch.int64, device="cuda")
    # no second output
    part = torch.full((nblk * 2 * C,), float("nan"), device="cuda")
    dx = torch.full_like(b.x, float("nan"))
    assert L.fs2hip_layernorm_bwd_x(b.dy.data_ptr(), b.x.data_ptr(), b.gamma.data_ptr(), b.mean.data_ptr(),
                                    b.rstd.data_ptr(), b.add.data_ptr(), dx.data_ptr(), None, 0.0, 0.0, 0, None,
                                    part.data_ptr(), b.M, C, 0, s) == 0
    part0 = torch.full((nblk * 2 * C,), float("nan"), device="cuda")
    dx0 = torch.full_like(b.x, float("nan"))
    assert L.fs2hip_layernorm_bwd(b.dy.data_ptr(), b.x.data_ptr(), b.gamma.data_ptr(), b.mean.data_ptr(),
                                  b.rstd.data_ptr(), b.add.data_ptr(), dx0.data_ptr(), part0.data_ptr(), None, None,
                                  b.M, C, s) == 0
    assert torch.equal(dx, dx0) and torch.equal(part, part0) and bool(torch.isfinite(part).all())
    # with the second output
    part = torch.full((nblk * 3 * C,), float("nan"), device="cuda")
    dx, dz = torch.full_like(b.x, float("nan")), torch.full_like(b.x, float("nan"))
    assert L.fs2hip_layernorm_bwd_x(b.dy.data_ptr(), b.x.data_ptr(), b.gamma.data_ptr(), b.mean.data_ptr(),
                                    b.rstd.data_ptr(), None, dx.data_ptr(), dz.data_ptr(), 0.5, 0.3, 77, st.data_ptr(),
                                    part.data_ptr(), b.M, C, 0, s) == 0
    part0 = torch.full((nblk * 3 * C,), float("nan"), device="cuda")
    dx0, dz0 = torch.full_like(b.x, float("nan")), torch.full_like(b.x, float("nan"))
    assert L.fs2hip_layernorm_bwd_dz(b.dy.data_ptr(), b.x.data_ptr(), b.gamma.data_ptr(), b.mean.data_ptr(),
                                     b.rstd.data_ptr(), None, dx0.data_ptr(), dz0.data_ptr(), 0.5, 0.3, 77,
                                     st.data_ptr(), part0.data_ptr(), b.M, C, s) == 0
    assert torch.equal(dx, dx0) and torch.equal(dz, dz0) and torch.equal(part, part0)
    assert bool(torch.isfinite(part).all()) and torch.equal(dz.cpu() == 0, R.drop_factors(0.3, 77, 2, b.M * C).view(b.M, C) == 0)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bf16_predictor(H, bcase, p):
    b = bcase
    st = torch.full((1,), 4, dtype=torch.int64, device="cuda")
    drop = H.Drop(p, (1 << 36) + 5, st) if p else H.NO_DROP
    dg32, db32, dg, db = nan_vecs(b.C, 4)
    dx32 = H.layernorm_bwd_pred(b.dy, b.x, b.gamma, b.mean, b.rstd, dg32, db32, drop)
    dxb = H.layernorm_bwd_pred(b.dy, b.x, b.gamma, b.mean, b.rstd, dg, db, drop, out_dtype=torch.bfloat16)
    H.flush_grad_reductions()
    assert dxb.dtype == torch.bfloat16 and torch.equal(dxb, dx32.bfloat16())
    assert torch.equal(dg, dg32) and torch.equal(db, db32) and bool(torch.isfinite(dg).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals: FS2HIP_EINVAL before any launch, outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
EINVAL = -22
ENTRY_POINTS = ["fs2hip_layernorm_fwd", "fs2hip_layernorm_fwd_drop", "fs2hip_layernorm_fwd_b", "fs2hip_layernorm_bwd",
                "fs2hip_layernorm_bwd_dz", "fs2hip_layernorm_bwd_pred:fp32", "fs2hip_layernorm_bwd_pred:bf16",
                "fs2hip_layernorm_bwd_x:0", "fs2hip_layernorm_bwd_x:1", "fs2hip_layernorm_bwd_x:3"]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_refusals_leave_the_outputs_untouched(H, entry):
    """C not a multiple of 4, C > 1024, C = 0, M = 0, an x that is 4 bytes off a 16-byte boundary, and (where the caller
    must bring one) a null partial-sum buffer.  Every buffer is large enough for the widest refused shape."""
    L, s = H.lib(), H._stream()
    Mb, Cb = 8, 1032
    g = torch.Generator().manual_seed(3)
    x = torch.randn(Mb * Cb + 4, generator=g).cuda()
    dy, add = torch.randn(Mb * Cb, generator=g).cuda(), torch.randn(Mb * Cb, generator=g).cuda()
    dyb = dy.bfloat16()
    gamma, beta = torch.ones(Cb, device="cuda"), torch.zeros(Cb, device="cuda")
    mean_i, rstd_i = torch.zeros(Mb, device="cuda"), torch.ones(Mb, device="cuda")
    st = torch.zeros(1, dtype=torch.int64, device="cuda")
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    y, dx, dz, part = nan(Mb * Cb), nan(Mb * Cb), nan(Mb * Cb), nan(Mb * 3 * Cb)
    mean_o, rstd_o, dg, db = nan(Mb), nan(Mb), nan(Cb), nan(Cb)
    P = lambda t: t.data_ptr()
    name, _, form = entry.partition(":")
    fn = getattr(L, name)

    def call(M, C, xp, pp):
        if name == "fs2hip_layernorm_fwd" or name == "fs2hip_layernorm_fwd_b":
            return fn(xp, P(gamma), P(beta), P(y), P(mean_o), P(rstd_o), M, C, EPS, s)
        if name == "fs2hip_layernorm_fwd_drop":
            return fn(xp, P(gamma), P(beta), P(y), P(mean_o), P(rstd_o), M, C, EPS, 0.3, 17, P(st), s)
        if name == "fs2hip_layernorm_bwd":
            return fn(P(dy), xp, P(gamma), P(mean_i), P(rstd_i), P(add), P(dx), pp, P(dg), P(db), M, C, s)
        if name == "fs2hip_layernorm_bwd_dz":
            return fn(P(dy), xp, P(gamma), P(mean_i), P(rstd_i), P(add), P(dx), P(dz), 0.5, 0.3, 17, P(st), pp, M, C, s)
        if name == "fs2hip_layernorm_bwd_pred":
            return fn(P(dy), xp, P(gamma), P(mean_i), P(rstd_i), P(dx), int(form == "bf16"), pp, M, C, 0.3, 17, P(st), s)
        flags = int(form)
        return fn(P(dyb) if flags & 1 else P(dy), xp, P(gamma), P(mean_i), P(rstd_i), P(add), P(dx), P(dz), 0.5, 0.3, 17,
                  P(st), pp, M, C, flags, s)

    bad = [("C = 6", 8, 6, P(x), P(part)), ("C = 1028", 8, 1028, P(x), P(part)), ("C = 0", 8, 0, P(x), P(part)),
           ("M = 0", 0, 8, P(x), P(part)), ("M < 0", -1, 8, P(x), P(part)),
           ("x off by 4 bytes", 8, 8, P(x[1:]), P(part))]
    if name not in ("fs2hip_layernorm_fwd", "fs2hip_layernorm_fwd_b", "fs2hip_layernorm_fwd_drop"):
        bad.append(("null partial", 8, 8, P(x), None))
    assert P(x) % 16 == 0 and P(x[1:]) % 16 == 4
    for what, M, C, xp, pp in bad:
        assert call(M, C, xp, pp) == EINVAL, f"{entry}: {what}"
    torch.cuda.synchronize()
    for t in (y, dx, dz, part, mean_o, rstd_o, dg, db):
        assert bool(torch.isnan(t).all()), f"{entry}: an output was written"
