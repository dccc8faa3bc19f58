"""CPU: the references of ``tests/adaptor_references.py`` against torch's own operators, and the edge conditions the
generated inputs of ``tests/test_adaptor_kernels_gpu.py`` are there to produce -- so a mismatch on the GPU is the
kernel's, and an input generator that stops producing an edge fails here instead of hiding it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import adaptor_references as R


# ---------------------------------------------------------------------------------------------------------------------
# references against torch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", [(2048, 384), (257, 6), (1, 2)])
def test_table_is_float64_sin_of_the_fp32_matmul_angle(T, D):
    inv = R.inv_freq(D)
    assert inv.dtype == torch.float32 and inv.numel() == D // 2
    ang = torch.matmul(torch.arange(T, dtype=torch.float32)[:, None], inv[None, :])  # as the reference module forms it
    assert torch.equal(R.posenc_angles(inv, T), ang)
    tab = R.posenc_table64(inv, T)
    assert tab.dtype == torch.float64 and tab.shape == (T, D)
    assert torch.equal(tab[:, : D // 2], ang.double().sin()) and torch.equal(tab[:, D // 2:], ang.double().cos())
    if T > 1000:
        assert float(ang.max()) > 2000  # thousands of radians: an approximate sine is off here, not at T = 7
    # the module's own fp32 table lies within the GPU test's tolerance of this reference
    own = torch.cat([ang.sin(), ang.cos()], 1)
    np.testing.assert_allclose(own.numpy(), tab.numpy(), rtol=2e-6, atol=2e-7)


def test_add32_is_the_fp32_add():
    g = R.gen(1)
    a, b = torch.randn(100000, generator=g), torch.randn(100000, generator=g) * 10.0 ** torch.randint(-8, 3, (100000,), generator=g)
    assert torch.equal(R.add32(a, b), a + b)


def test_add_posenc_reference():
    B, T, D = 4, 9, 8
    g = R.gen(2)
    x, table = torch.randn(B, T, D, generator=g), torch.randn(T + 2, D, generator=g)
    lens = torch.tensor([0, 1, T, T + 3], dtype=torch.int32)
    mask = (torch.arange(T)[None, :] < lens[:, None]).float()
    want = x + table[:T][None] * mask[..., None]
    got = R.add_posenc(x, table, lens)
    assert torch.equal(got, want) and torch.equal(got[0], x[0]) and torch.equal(got[1, 1:], x[1, 1:])


@pytest.mark.parametrize("padding_idx", [0, -1])
def test_embedding_gradient_is_torchs(padding_idx):
    M, V, D = 501, 23, 8
    idx, _ = R.skewed_indices(M, V)
    W = torch.randn(V, D, generator=R.gen(3)).double().requires_grad_(True)
    dy = torch.randn(M, D, generator=R.gen(4))
    F.embedding(idx.long(), W, padding_idx=padding_idx if padding_idx >= 0 else None).backward(dy.double())
    dW, sc = R.embedding_bwd64(idx, dy, V, padding_idx)
    assert dW.dtype == torch.float64 and torch.allclose(dW, W.grad, rtol=1e-13, atol=1e-13)
    assert bool((sc >= dW.abs() - 1e-12).all())
    if padding_idx >= 0:
        assert int((idx == padding_idx).sum()) >= 1 and bool((dW[padding_idx] == 0).all())


@pytest.mark.parametrize("control", [1.0, 0.7, 1.3])
def test_bucketize_reference(control):
    bins = R.bucket_bins(255)
    val = R.bucket_values(bins, control)
    W, x = torch.randn(256, 4, generator=R.gen(5)), torch.randn(val.numel(), 4, generator=R.gen(6))
    out, idx, scaled = R.bucket_embed_add(val, control, bins, W, x)
    c32 = np.float32(control)
    with np.errstate(over="ignore"):  # 3e38 * 1.3 is inf, in both
        assert np.array_equal(scaled.numpy(), val.numpy() * c32, equal_nan=True)
    # bucketize (right=False): the number of edges strictly below the value; NaN takes the last bucket
    v = scaled.double()
    want = (bins.double()[None, :] < v[:, None]).sum(1)
    want[torch.isnan(v)] = bins.numel()
    assert torch.equal(idx, want)
    assert torch.equal(out, x + W[idx])


def test_control_of_rows():
    control = torch.tensor([[0.5, 2.0, 3.0], [1.5, 0.25, 4.0]])
    ctl_idx = torch.tensor([[0, 2, -1, 3, 1], [-1, -1, 1, 7, 2]], dtype=torch.int32)
    assert R.control_of_rows(control, ctl_idx).tolist() == [[0.5, 3.0, 1.0, 1.0, 2.0], [1.0, 1.0, 0.25, 1.0, 4.0]]


@pytest.mark.parametrize("shape", R.LR_SHAPES[1:] + [(3, 301, 2049, 4)], ids=str)
@pytest.mark.parametrize("with_table", [False, True])
def test_length_regulator_reference_is_repeat_interleave_and_its_autograd(shape, with_table):
    B, Ts, Tm, D = shape
    g = R.gen(7)
    dur = R.lr_durations(B, Ts, Tm)
    x = torch.randn(B, Ts, D, generator=g)
    table = torch.randn(Tm + 3, D, generator=g) if with_table else None
    out, cum, lens, src = R.length_regulate(x, dur, Tm, table)
    pos = dur.long().clamp(min=0)
    assert torch.equal(cum.long(), pos.cumsum(1)) and torch.equal(lens.long(), pos.sum(1).clamp(max=Tm))
    xr = x.double().requires_grad_(True)
    want = torch.zeros(B, Tm, D, dtype=torch.float64)
    for b in range(B):
        rows = torch.repeat_interleave(xr[b], pos[b], dim=0)[:Tm]
        n = rows.shape[0]
        assert n == int(lens[b])
        if with_table:
            rows = rows + table[:n].double()
        want = want.index_put((torch.tensor(b), torch.arange(n)), rows)
        # src_idx: frame t belongs to the first token whose cumulative duration exceeds t
        first = (cum[b].long()[None, :] > torch.arange(Tm)[:, None]).long().cumsum(1).eq(0).sum(1)
        assert torch.equal(src[b].long(), torch.where(first < Ts, first, torch.tensor(-1)))
    assert out.dtype == torch.float32 and torch.equal(out, want.detach().float())
    assert bool((out[src < 0] == 0).all())
    dy = torch.randn(B, Tm, D, generator=g)
    want.backward(dy.double())
    dx, sc = R.length_regulate_bwd64(dy, src, Ts)
    assert dx.dtype == torch.float64 and torch.allclose(dx, xr.grad, rtol=1e-13, atol=1e-13)
    assert bool((sc >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize("max_norm,grad_scale", R.OPT_CONFIGS)
def test_optimizer_reference_is_torch_adamw_clip_and_noam(max_norm, grad_scale):
    """float64 ``torch.optim.AdamW`` + ``clip_grad_norm_`` + the Noam formula, fed the fp32 hyperparameters."""
    n = 1000
    p0 = R.opt_params(n)
    ref = R.Optimizer64(p0, max_norm=max_norm, grad_scale=grad_scale, **R.OPT)
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], R.f32(R.OPT["base_lr"]), betas=(ref.b1, ref.b2), eps=ref.eps, weight_decay=ref.wd)
    for k in range(1, R.OPT_STEPS + 1):
        g = R.opt_grad(n, k)
        rec = ref.step(g)
        lr = R.noam_lr(R.f32(R.OPT["base_lr"]), R.OPT["warmup"], k)
        for grp in opt.param_groups:
            grp["lr"] = lr
        p.grad = g.double() * grad_scale
        norm = float(p.grad.norm())
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([p], max_norm)
            assert abs(float(total) - norm) <= 1e-12 * norm
        opt.step()
        assert rec["step"] == k and abs(rec["lr"] - lr) <= 1e-15 * lr
        assert abs(rec["grad_norm"] - norm) <= 1e-12 * max(norm, 1e-30)
        assert abs(rec["bc1"] - (1 - ref.b1 ** k)) < 1e-15 and abs(rec["bc2"] - (1 - ref.b2 ** k)) < 1e-15
        want_coef = grad_scale * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)
        assert abs(rec["clip_coef"] - want_coef) <= 1e-12 * want_coef
        state = opt.state[p]
        assert torch.allclose(ref.m, state["exp_avg"], rtol=1e-11, atol=1e-300)
        assert torch.allclose(ref.v, state["exp_avg_sq"], rtol=1e-11, atol=1e-300)
        assert torch.allclose(ref.p - p0.double(), p.detach() - p0.double(), rtol=1e-9, atol=1e-15)
        assert bool(torch.isfinite(ref.p).all())
    # the rate rose, peaked at the warmup step + 1 and decayed
    rates = [R.noam_lr(1.0, R.OPT["warmup"], k) for k in range(1, R.OPT_STEPS + 1)]
    peak = rates.index(max(rates))
    assert 0 < peak < R.OPT_STEPS - 1 and rates[0] < rates[peak] > rates[-1]


# ---------------------------------------------------------------------------------------------------------------------
# what the generated inputs are there to produce
# ---------------------------------------------------------------------------------------------------------------------
def test_optimizer_inputs():
    kinds = [R.opt_grad_kind(k) for k in range(1, R.OPT_STEPS + 1)]
    assert kinds.count("zero") == 1 and kinds.count("large") >= 4 and kinds.count("small") >= 4
    assert R.OPT_SIZES[-1] > 8192 * 256 and (R.OPT_SIZES[-1] // 4) > 1024 * 256 and R.OPT_SIZES[-1] % 4 == 3
    for n in R.OPT_SIZES:
        dead = R.opt_dead(n)
        if n >= 10:
            assert abs(int(dead.sum()) - n / 10) <= 1
        for k in range(1, R.OPT_STEPS + 1):
            g = R.opt_grad(n, k)
            assert bool((g[dead] == 0).all())
            for max_norm, scale in R.OPT_CONFIGS:
                norm = float(g.double().norm()) * scale
                if kinds[k - 1] == "large":    # clip active
                    assert norm > 1.0, (n, k, norm)
                elif kinds[k - 1] == "small":  # clip idle, the gradient at 1e-6 scale
                    assert 0 < norm < 1e-2 and float(g.abs().max()) < 1e-5, (n, k, norm)
                else:
                    assert norm == 0


@pytest.mark.parametrize("NB", [1, 2, 255, 256])
@pytest.mark.parametrize("control", [1.0, 0.7, 1.3])
def test_bucket_inputs(NB, control):
    bins = R.bucket_bins(NB)
    assert bins.numel() == NB and bins.dtype == torch.float32 and bool((bins[1:] >= bins[:-1]).all())
    if NB == 255:
        assert int((bins[1:] == bins[:-1]).sum()) >= 3  # repeated edges
    val = R.bucket_values(bins, control)
    assert val.shape == (R.BUCKET_M,) and val.dtype == torch.float32
    have = set(val.view(torch.int32).tolist())
    inf = torch.tensor(float("inf"))
    for want in (bins, torch.nextafter(bins, inf), torch.nextafter(bins, -inf)):
        assert set(want.view(torch.int32).tolist()) <= have
    assert int(torch.isnan(val).sum()) >= 2 and int((val == inf).sum()) >= 1 and int((val == -inf).sum()) >= 1
    fin = val[torch.isfinite(val)]
    assert float(fin.min()) < float(bins[0]) - 0.5 and float(fin.max()) > float(bins[-1]) + 0.5
    scaled = val * torch.tensor(control, dtype=torch.float32)
    idx = torch.bucketize(scaled, bins)
    assert int(idx.min()) == 0 and int(idx.max()) == NB
    if NB >= 255:
        assert idx.unique().numel() >= NB - 8  # nearly every bucket is selected (repeated edges leave empty ones)
    if control != 1.0:
        q = bins / torch.tensor(control, dtype=torch.float32)
        assert set(q.view(torch.int32).tolist()) <= have
        back = int((q * torch.tensor(control, dtype=torch.float32) == bins).sum())
        # with one or two edges there are not twenty quotients to begin with; the 255- and 256-edge vectors carry them
        assert back >= (20 if NB >= 255 else 0), back
    # on an edge the bucket is the edge's own index (right=False); one ulp above, the next one
    on_edge = (scaled[:, None] == bins[None, :]).any(1)
    assert int(on_edge.sum()) >= (NB if control == 1.0 else min(NB, 20) if NB >= 255 else 0)


@pytest.mark.parametrize("M,V", [(4099, 83), (37, 84), (25003, 84)])
def test_embedding_inputs(M, V):
    idx, never = R.skewed_indices(M, V)
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < V
    counts = torch.bincount(idx.long(), minlength=V)
    assert int(counts.max()) * 3 >= M and int(counts.argmax()) == 7
    assert never.numel() >= 5 and int(counts[never].sum()) == 0 and int((counts == 0).sum()) >= 5
    assert int(counts[0]) >= 1  # rows of the padding index exist
    if M > 4000:
        assert int(counts[7]) >= 1000  # one row of the gradient is a sum of more than a thousand terms


def test_length_regulator_inputs():
    B, Ts, Tm, D = R.LR_SHAPES[0]
    assert (B * Tm) % 4 and Ts & (Ts - 1) and D // 4 > 64 and (D // 4) % 64
    dur = R.lr_durations(B, Ts, Tm)
    assert dur.shape == (B, Ts) and dur.dtype == torch.int32
    pos = dur.long().clamp(min=0)
    cum, total = pos.cumsum(1), pos.sum(1)
    for b in (0, 1):
        assert float((pos[b] == 0).float().mean()) >= 0.15
        assert int(pos[b, :5].sum()) == 0 and int(pos[b, 150:160].sum()) == 0 and int(pos[b, -7:].sum()) == 0
        assert int((dur[b] < 0).sum()) >= 3
    assert float((pos == 0).float().mean()) >= 0.15
    assert int(pos.max()) >= 512 and int(pos[0, 100]) == R.LR_LONG
    assert int(total[0]) == Tm
    # utterance 1: past Tm, the cut inside a token (Tm is no token boundary), and tokens wholly past it
    assert int(total[1]) > Tm and not bool((cum[1] == Tm).any())
    j = int((cum[1] > Tm).nonzero()[0])
    assert (int(cum[1, j - 1]) if j else 0) < Tm < int(cum[1, j]) and int((pos[1, j + 1:] > 0).sum()) >= 3
    assert int(total[2]) == 0 and bool((dur[2] == 0).all())
    B2, Ts2, Tm2, _ = R.LR_SHAPES[1]
    d2 = R.lr_durations(B2, Ts2, Tm2)
    t2 = d2.long().clamp(min=0).sum(1)
    assert B2 > 64 and int((d2 < 0).sum()) > 0 and int((t2 > Tm2).sum()) > 0 and int((t2 < Tm2).sum()) > 0
    p2 = d2.long().clamp(min=0)
    assert int(((p2.cumsum(1) - p2 >= Tm2) & (p2 > 0)).sum()) > 0  # tokens wholly past Tm
    assert R.lr_durations(1, 1, 1).tolist() == [[2]]
