"""GPU parity of the conv / BatchNorm / gather / loss / optimizer kernels against plain
PyTorch fp32 references (integer outputs bit-exact, floats at ~1e-5 of scale)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    hip.lib()
    return hip


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(a, b, tol=2e-5, msg=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max()) / scale
    assert err < tol, f"{msg}: rel err {err:.3e}"


@pytest.mark.parametrize("K,C,glu", [(9, 256, True), (3, 256, False), (9, 32, True), (3, 32, False), (5, 80, False)])
def test_dwconv(H, K, C, glu):
    B, T = 3, 70
    x = rnd(B, T, 2 * C if glu else C, seed=1).requires_grad_(True)
    w = rnd(C, 1, K, seed=2, scale=0.3).requires_grad_(True)
    b = rnd(C, seed=3).requires_grad_(True)
    a = F.glu(x, dim=-1) if glu else x
    ref = F.conv1d(a.transpose(1, 2), w, b, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    wk = w.detach()[:, 0, :].t().contiguous().cuda()  # [K, C]
    y, parts = H.dwconv_fwd(x.detach().cuda(), wk, b.detach().cuda(), B, T, glu=glu, stats=True)
    close(y, ref, msg="dwconv fwd")
    # fused BatchNorm statistics: per part (mean, sum of squared deviations) over 64-step stripes of one utterance
    assert parts.part_rows == 64 and parts.group_rows == T and parts.count == B * T
    stripes = [ref[bb, t0:t0 + 64].double() for bb in range(B) for t0 in range(0, T, 64)]
    assert parts.nparts == len(stripes)
    close(parts.partial[:, 0], torch.stack([sp.mean(0) for sp in stripes]), 1e-5, "stripe means")
    close(parts.partial[:, 1], torch.stack([((sp - sp.mean(0)) ** 2).sum(0) for sp in stripes]), 1e-5, "stripe M2")
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    st = H.bn_finalize(parts, one, zero, None, None, training=True)
    flat = ref.reshape(-1, C).double()
    close(st[2], flat.mean(0), 1e-6, "fused mean")
    close(st[3], 1 / torch.sqrt(flat.var(0, unbiased=False) + 1e-5), 1e-6, "fused invstd")
    dy = rnd(B, T, C, seed=4)
    ref.backward(dy)
    dw, db = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
    dx = H.dwconv_bwd(dy.cuda(), x.detach().cuda(), wk, dw, db, B, T, glu=glu)
    close(dx, x.grad, msg="dwconv dx")
    close(dw, w.grad[:, 0, :].t(), 1e-4, "dwconv dw")
    close(db, b.grad, 1e-4, "dwconv db")


def _batchnorm_case(H, act, C, M, dtype=torch.float32):
    """BatchNorm + activation, training and eval, against ``F.batch_norm`` run in ``dtype`` on the CPU."""
    y32 = rnd(M, C, seed=1) * 2 + 0.5
    y = y32.to(dtype).requires_grad_(True)
    g, b = (1 + 0.1 * rnd(C, seed=2)).to(dtype).requires_grad_(True), rnd(C, seed=3).to(dtype).requires_grad_(True)
    rm, rv = 0.1 * rnd(C, seed=4), torch.rand(C, generator=torch.Generator().manual_seed(5)) + 0.5
    rm_ref, rv_ref = rm.clone().to(dtype), rv.clone().to(dtype)
    f = {"relu": F.relu, "silu": F.silu, "tanh": torch.tanh, None: lambda t: t}[act]
    pre = F.batch_norm(y, rm_ref, rv_ref, g, b, training=True, momentum=0.1, eps=1e-5)
    ref = f(pre)
    rm_d, rv_d = rm.cuda(), rv.cuda()
    g_d, b_d = g.detach().float().cuda(), b.detach().float().cuda()
    stats = H.bn_finalize(H.colstats(y32.cuda()), g_d, b_d, rm_d, rv_d, training=True)
    out = H.bn_act_fwd(y32.cuda(), stats, act)
    close(out, ref, msg="bn fwd")
    close(rm_d, rm_ref, msg="running mean")
    close(rv_d, rv_ref, msg="running var")
    dout = rnd(M, C, seed=6)
    if act == "relu":
        # ReLU's derivative jumps at 0: an element whose normalised value is a rounding error away from 0 may be kept
        # by one side and dropped by the other, and both are right.  The kernel's own decision (its forward output)
        # must agree with the reference's wherever the reference is not that close to 0; the backward reference
        # then differentiates with the kernel's decision.
        keep = out.cpu() > 0
        clear = pre.detach().abs() > 1e-5 * max(1.0, float(pre.detach().abs().max()))
        assert int(clear.sum()) > 0.99 * clear.numel()
        assert torch.equal(keep[clear], (pre.detach() > 0)[clear])
        pre.backward(dout.to(dtype) * keep)
    else:
        ref.backward(dout.to(dtype))
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dy = H.bn_act_bwd(dout.cuda(), y32.cuda(), stats, dg, db, act)
    close(dg, g.grad, 1e-4, "bn dgamma")
    close(db, b.grad, 1e-4, "bn dbeta")
    # eval mode uses the running statistics
    stats_e = H.bn_finalize(None, g_d, b_d, rm_d, rv_d, training=False)
    out_e = H.bn_act_fwd(y32.cuda(), stats_e, act)
    ref_e = f(F.batch_norm(y.detach(), rm_ref, rv_ref, g.detach(), b.detach(), training=False, eps=1e-5))
    close(out_e, ref_e, msg="bn eval")
    close(dy, y.grad, 5e-5, "bn dy")


@pytest.mark.parametrize("act,C", [("silu", 256), ("tanh", 512), (None, 80), ("relu", 32), ("relu", 128)])
def test_batchnorm_train_and_eval(H, act, C):
    _batchnorm_case(H, act, C, 1234)


def test_batchnorm_relu_two_rows(H):
    """What the last GST convolution's BatchNorm sees for one utterance with a short mel: two rows (each channel's
    batch statistics come from two numbers).  Float64 reference, the assertions of the cases above.

    With two rows the input gradient is, in exact arithmetic, (dz_0 - dz_1) / 2 * eps / (var + eps) per channel: terms
    of size 1 cancel to ~1e-3 (max |dy| = 3.6e-3 here).  The fp32 reduce / apply kernels kept three digits of it
    (1.355e-03 of max |dy| against the 5e-05 asked here; torch's own fp32 CPU backward is 1.306e-03 off float64 on the
    same input), which is why batches of up to 16 rows take ``bn_bwd_small_kernel``: statistics from y again and
    the whole difference in fp64."""
    _batchnorm_case(H, "relu", 128, 2, dtype=torch.float64)


@pytest.mark.parametrize("M,act,C", [(2, None, 32), (3, "relu", 128), (16, "silu", 256), (17, "tanh", 64)])
def test_batchnorm_few_rows(H, M, act, C):
    """Both sides of the 16-row limit of the fp64 few-rows backward (17 rows: the general fp32 kernels), float64 reference."""
    _batchnorm_case(H, act, C, M, dtype=torch.float64)


@pytest.mark.parametrize("M,C,offset,std", [
    (1234, 256, 50.0, 1e-2),    # |mean| / std = 5000: E[x^2] - E[x]^2 in fp32 has no correct digit left here
    (20736, 512, 100.0, 1.0),   # benchmark-size column, |mean| / std = 100
    (3, 256, 5.0, 0.05),        # three rows (the smallest decoder the ragged-batch test builds)
    (2, 64, -3.0, 0.5),         # two rows
    (70000, 32, 10.0, 0.1),     # more stripes than one finalize pass of 16 lanes (and cs_rows > 32)
])
def test_batchnorm_statistics_are_welford_accurate(H, M, C, offset, std):
    """Batch statistics of channels whose |mean| >> std, and of 2-3 rows, against float64 and ``F.batch_norm``
    (torch's CPU BatchNorm is Welford).  The variance must be right to fp32 accuracy OF THE VARIANCE: invstd within
    1e-4 relative where a sum / sum-of-squares formula is off by tens of percent."""
    g0 = torch.Generator().manual_seed(M + C)
    y = (offset * (1 + 0.1 * torch.randn(C, generator=g0)) + std * torch.randn(M, C, generator=g0)).float()
    yd = y.double()
    mean64, var64 = yd.mean(0), yd.var(0, unbiased=False)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    st = H.bn_finalize(H.colstats(y.cuda()), one, zero, rm, rv, training=True)
    inv64 = 1 / torch.sqrt(var64 + 1e-5)
    assert float(((st[2].cpu().double() - mean64).abs() / mean64.abs()).max()) < 1e-6
    assert float(((st[3].cpu().double() - inv64).abs() / inv64).max()) < 1e-4
    rm_ref, rv_ref = torch.zeros(C), torch.ones(C)
    ref = F.batch_norm(y, rm_ref, rv_ref, None, None, training=True, momentum=0.1, eps=1e-5)
    out = H.bn_act_fwd(y.cuda(), st, None).cpu().double()
    # the normalised values carry the rounding of mean * invstd (a number of size |mean| / std, per channel) whatever
    # the algorithm: bound each channel by that, against float64, and require to be no worse than torch's own result
    ref64 = (yd - mean64) * inv64
    bound = 2e-5 + 4 * 6e-8 * mean64.abs() * inv64
    assert bool(((out - ref64).abs().amax(0) < bound).all())
    assert float((out - ref64).abs().max()) < 2 * float((ref.double() - ref64).abs().max()) + 2e-5
    close(rv, rv_ref, 1e-4, "running var")
    close(rm, rm_ref, 1e-6, "running mean")


def test_dwconv_fused_statistics_large_offset(H):
    """The depthwise conv's fused statistics with a bias that puts every channel at |mean| / std ~ 1000."""
    B, T, C, K = 3, 150, 256, 9
    x = rnd(B, T, C, seed=11) * 0.01
    w = rnd(K, C, seed=12, scale=0.3)
    b = 20.0 + rnd(C, seed=13)
    ref = F.conv1d(x.transpose(1, 2), w.t().unsqueeze(1), b, padding=4, groups=C).transpose(1, 2).reshape(-1, C).double()
    y, parts = H.dwconv_fwd(x.cuda(), w.cuda(), b.cuda(), B, T, stats=True)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    st = H.bn_finalize(parts, one, zero, None, None, training=True)
    yd = y.reshape(-1, C).cpu().double()  # statistics of the values the kernel itself produced
    inv64 = 1 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5)
    assert float(((st[3].cpu().double() - inv64).abs() / inv64).max()) < 1e-4
    assert float(((st[2].cpu().double() - yd.mean(0)).abs() / yd.mean(0).abs()).max()) < 1e-6
    assert float((yd - ref).abs().max()) < 1e-4


def test_posenc_embedding_bucketize(H, golden_dir):
    g = dict(np.load(golden_dir / "units.npz"))
    D, T = 8, 7
    inv_freq = 1 / (10000 ** (torch.arange(0.0, D, 2.0) / D))
    table = H.posenc_table(inv_freq.cuda(), T, D)
    np.testing.assert_allclose(table.cpu().numpy(), g["pos/out"][0], rtol=2e-6, atol=2e-7)
    # masked add
    B, T, D = 3, 9, 16
    x = rnd(B, T, D, seed=1)
    inv = 1 / (10000 ** (torch.arange(0.0, D, 2.0) / D))
    lens = torch.tensor([9, 4, 1], dtype=torch.int32)
    tab = H.posenc_table(inv.cuda(), T, D)
    out = H.add_posenc(x.cuda(), tab, lens.cuda(), B, T)
    ang = torch.arange(T).float()[:, None] @ inv[None, :]
    pe = torch.cat([ang.sin(), ang.cos()], 1)
    mask = torch.arange(T)[None, :] < lens[:, None]
    close(out, x + pe[None] * mask[..., None], msg="add_posenc")
    # embedding fwd / bwd with padding row
    V = 11
    W = rnd(V, D, seed=2).requires_grad_(True)
    idx = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(3))
    ref = F.embedding(idx, W, padding_idx=0)
    out = H.embedding_fwd(idx.int().cuda(), W.detach().cuda())
    assert torch.equal(out.cpu(), ref.detach())
    dy = rnd(B, T, D, seed=4)
    ref.backward(dy)
    dW = torch.empty(V, D, device="cuda")
    H.embedding_bwd(idx.int().cuda(), dy.cuda(), dW, padding_idx=0)
    close(dW, W.grad, msg="embedding bwd")
    # bucketize: golden vector from the reference's own torch.bucketize call + random
    bins, v = torch.tensor(g["bucket/bins"]), torch.tensor(g["bucket/v"])
    emb = rnd(bins.numel() + 1, D, seed=5)
    xx = rnd(v.numel(), D, seed=6)
    out, bidx = H.bucket_embed_add(v.cuda(), bins.cuda(), emb.cuda(), xx.cuda())
    np.testing.assert_array_equal(bidx.cpu().numpy(), g["bucket/out"])
    assert torch.equal(out.cpu(), xx + emb[torch.tensor(g["bucket/out"])])
    bins = torch.linspace(-3, 3, 255)
    v = rnd(5000, seed=7) * 2
    v[:255] = bins  # exactly on the edges
    _, bidx = H.bucket_embed_add(v.cuda(), bins.cuda(), rnd(256, D).cuda(), rnd(5000, D).cuda())
    assert torch.equal(bidx.cpu().long(), torch.bucketize(v, bins))


def test_length_regulator(H, golden_dir):
    g = dict(np.load(golden_dir / "units.npz"))
    x, dur = torch.tensor(g["lr/x"]), torch.tensor(g["lr/dur"])
    D = x.shape[-1]
    x4 = torch.cat([x, torch.zeros(*x.shape[:2], 8 - D)], -1)  # kernel wants D % 4 == 0
    for tag in ("full", "trunc"):
        ref, mask = g[f"lr/{tag}/out"], g[f"lr/{tag}/mask"]
        Tm = ref.shape[1]
        out, cum, lens = H.length_regulate_fwd(x4.cuda(), dur.cuda(), Tm)
        np.testing.assert_array_equal(out.cpu().numpy()[..., :D], ref)
        got_mask = (torch.arange(Tm)[None, :] < lens.cpu()[:, None]).numpy()
        # reference mask uses the untruncated total; both agree on [0, Tm)
        np.testing.assert_array_equal(got_mask, mask)
    # random, with backward vs autograd of repeat_interleave
    B, Ts, D = 4, 19, 32
    x = rnd(B, Ts, D, seed=1).requires_grad_(True)
    dur = torch.randint(0, 6, (B, Ts), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    Tm = int(dur.sum(1).max())
    rows = [torch.repeat_interleave(x[b], dur[b].long(), dim=0) for b in range(B)]
    ref = torch.zeros(B, Tm, D)
    for b, r in enumerate(rows):
        ref[b, : r.shape[0]] = r
    out, cum, lens = H.length_regulate_fwd(x.detach().cuda(), dur.cuda(), Tm)
    assert torch.equal(out.cpu(), ref.detach())
    assert torch.equal(lens.cpu(), dur.sum(1).int())
    dy = rnd(B, Tm, D, seed=3)
    ref.backward(dy)
    dx = H.length_regulate_bwd(dy.cuda(), cum)
    close(dx, x.grad, msg="lr bwd")
    # fused positional add: valid frames are x[token] + table[t] (one fp32 add: exact), frames past the total stay 0.
    # Zero-duration tokens first and last, an utterance of zero frames, and Tm shorter than the longest total (25).
    B, Ts, D, Tm = 4, 9, 16, 20
    x = rnd(B, Ts, D, seed=5)
    dur = torch.tensor([[0, 3, 0, 2, 4, 0, 1, 2, 0], [0] * 9, [0, 5, 5, 5, 5, 5, 0, 0, 0], [0, 1, 1, 1, 1, 1, 1, 1, 0]],
                       dtype=torch.int32)
    table = rnd(Tm + 3, D, seed=6)
    ref = torch.zeros(B, Tm, D)
    for b in range(B):
        r = torch.repeat_interleave(x[b], dur[b].long(), dim=0)[:Tm]
        ref[b, : r.shape[0]] = r + table[: r.shape[0]]
    out, cum, lens = H.length_regulate_fwd(x.cuda(), dur.cuda(), Tm, table=table.cuda())
    assert torch.equal(out.cpu(), ref)
    assert int(out[1].count_nonzero()) == 0 and int(out[0, 12:].count_nonzero()) == 0
    assert torch.equal(lens.cpu(), dur.sum(1).clamp(max=Tm).int())
    assert torch.equal(cum.cpu(), dur.cumsum(1).int())
    plain, _, _ = H.length_regulate_fwd(x.cuda(), dur.cuda(), Tm)
    assert not torch.equal(plain.cpu(), ref)  # (the table does change the valid frames)


def test_duration_cumsum_expect_and_bad_count(H):
    """``duration_cumsum(expect=, bad_count=)``: negative durations count as 0, the per-utterance mismatch flags are
    exact, and the persistent counter grows by the number of mismatches of every call."""
    dur = torch.tensor([[3, -2, 4, 0], [1, 1, 1, 1], [-5, -1, 0, 0], [2, 2, 2, 2], [7, 0, -1, 1]], dtype=torch.int32)
    pos = dur.clamp(min=0)
    assert pos.sum(1).tolist() == [7, 4, 0, 8, 8]
    Tm = 6
    bad = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    for expect, flags, total in (([7, 5, 0, 8, 9], [0, 1, 0, 0, 1], 5), ([0, 4, 1, 8, 8], [1, 0, 1, 0, 0], 7)):
        cum, lens, mism = H.duration_cumsum(dur.cuda(), Tm, expect=torch.tensor(expect, dtype=torch.int32).cuda(),
                                            bad_count=bad)
        assert torch.equal(cum.cpu(), pos.cumsum(1).int())
        assert torch.equal(lens.cpu(), pos.sum(1).clamp(max=Tm).int())
        assert mism.dtype == torch.int32 and mism.cpu().tolist() == flags
        assert int(bad) == total
    # without a counter the flags are still written; without ``expect`` two results, as before
    _, _, mism = H.duration_cumsum(dur.cuda(), Tm, expect=torch.tensor([7, 4, 0, 8, 8], dtype=torch.int32).cuda())
    assert mism.cpu().tolist() == [0] * 5 and int(bad) == 7
    assert len(H.duration_cumsum(dur.cuda(), Tm)) == 2
    # more utterances than one 64-thread workgroup
    g = torch.Generator().manual_seed(1)
    dur = torch.randint(-3, 6, (70, 13), generator=g, dtype=torch.int32)
    pos = dur.clamp(min=0)
    expect = pos.sum(1).int()
    expect[::3] += torch.randint(1, 4, expect[::3].shape, generator=g, dtype=torch.int32) * (1 - 2 * (torch.arange(24) % 2)).int()
    cum, lens, mism = H.duration_cumsum(dur.cuda(), 30, expect=expect.cuda(), bad_count=bad)
    assert torch.equal(cum.cpu(), pos.cumsum(1).int()) and torch.equal(lens.cpu(), pos.sum(1).clamp(max=30).int())
    assert torch.equal(mism.cpu(), (pos.sum(1) != expect).int()) and int(mism.sum()) == 24
    assert int(bad) == 7 + 24


def test_rowdot_and_losses(H):
    B, T, C = 3, 21, 256
    x = rnd(B, T, C, seed=1).requires_grad_(True)
    w, b = rnd(1, C, seed=2, scale=0.1).requires_grad_(True), rnd(1, seed=3).requires_grad_(True)
    lens = torch.tensor([21, 10, 3], dtype=torch.int32)
    mask = torch.arange(T)[None, :] < lens[:, None]
    ref = F.linear(x, w, b).squeeze(-1) * mask
    out = H.rowdot_fwd(x.detach().cuda(), w.detach().cuda(), b.detach().cuda(), lens.cuda(), B, T)
    close(out, ref, msg="rowdot fwd")
    tgt = rnd(B, T, seed=4)
    for kind, fn in (("mse", F.mse_loss), ("mae", F.l1_loss)):
        for t_ in (x, w, b):
            t_.grad = None
        loss = fn(ref * mask, tgt * mask) * 0.1
        loss.backward(retain_graph=True)
        slot = torch.zeros(1, device="cuda")
        dpred = H.masked_loss(out, tgt.cuda(), lens.cuda(), B, T, 1, kind=kind, weight=0.1, loss_out=slot)
        close(slot, loss.detach().reshape(1), msg=f"{kind} value")
        dw, db = torch.empty(C, device="cuda"), torch.empty(1, device="cuda")
        dx = H.rowdot_bwd(dpred, x.detach().cuda(), w.detach().cuda(), lens.cuda(), dw, db, B, T)
        close(dx, x.grad, msg=f"{kind} dx")
        close(dw, w.grad.reshape(-1), msg=f"{kind} dw")
        close(db, b.grad, msg=f"{kind} db")
    # duration loss: log(d + 1) target; spec loss with channels
    dur = torch.randint(0, 9, (B, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    pred = rnd(B, T, seed=6)
    ref = F.mse_loss(pred * mask, torch.log(dur.float() + 1) * mask) * 0.1
    slot = torch.zeros(1, device="cuda")
    H.masked_loss(pred.cuda(), dur.cuda(), lens.cuda(), B, T, 1, weight=0.1, loss_out=slot)
    close(slot, ref.reshape(1), msg="duration loss")
    spec, mel = rnd(B, T, 80, seed=7).requires_grad_(True), rnd(B, T, 80, seed=8)
    ref = F.mse_loss(spec * mask[..., None], mel * mask[..., None])
    ref.backward()
    d = H.masked_loss(spec.detach().cuda(), mel.cuda(), lens.cuda(), B, T, 80, loss_out=slot)
    close(slot, ref.detach().reshape(1), msg="spec loss")
    close(d, spec.grad, msg="spec grad")


def test_adamw_noam_clip(H):
    n = 100003
    p0, steps = rnd(n, seed=1), 5
    p_ref = p0.clone().requires_grad_(True)
    base_lr, warm, betas, eps, wd = 1e-3, 3, (0.9, 0.98), 1e-8, 0.01
    opt = torch.optim.AdamW([p_ref], base_lr, betas=betas, eps=eps, weight_decay=wd)
    p = p0.clone().cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    st = H.new_step_state("cuda")
    for k in range(1, steps + 1):
        gk = rnd(n, seed=10 + k) * (3.0 if k % 2 else 0.001)
        s = max(1, k - 1)
        lr = base_lr * warm ** 0.5 * min(s ** -0.5, s * warm ** -1.5)
        for grp in opt.param_groups:
            grp["lr"] = lr
        p_ref.grad = gk.clone()
        torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
        opt.step()
        H.step_advance(st, base_lr, warm, betas[0], betas[1])
        H.grad_clip_coef(gk.cuda(), 1.0, 1.0, st)
        H.adamw_step(p, gk.cuda(), m, v, st, betas[0], betas[1], eps, wd)
        rec = st.cpu()
        assert int(rec[0]) == k
        assert abs(float(rec.view(torch.float32)[2]) - lr) < 1e-9
        assert abs(float(rec.view(torch.float32)[6]) - float(gk.norm())) < 1e-3 * float(gk.norm())
    close(p, p_ref, 1e-5, "adamw params")


def test_axpby_and_rowvec(H):
    x, y = rnd(1000, seed=1), rnd(1000, seed=2)
    close(H.axpby(x.cuda(), y.cuda(), 0.5, 2.0), 0.5 * x + 2 * y, msg="axpby")
    d = H.Drop(0.25, 5)
    a = H.axpby(x.cuda(), None, 1.0, 0.0, d)
    b = H.axpby(torch.ones(1000, device="cuda"), None, 1.0, 0.0, d)
    assert torch.allclose(a, x.cuda() * b)
    assert abs((b == 0).float().mean().item() - 0.25) < 0.05
    # the device step counter changes the mask without changing the kernel arguments
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    d2 = H.Drop(0.25, 5, step)
    m0 = H.axpby(torch.ones(1000, device="cuda"), None, 1.0, 0.0, d2)
    step += 1
    m1 = H.axpby(torch.ones(1000, device="cuda"), None, 1.0, 0.0, d2)
    assert not torch.equal(m0, m1)
    B, T, D = 2, 5, 8
    xx, e = rnd(B, T, D, seed=3), rnd(B, D, seed=4)
    close(H.add_rowvec(xx.cuda(), e.cuda(), B, T), xx + e[:, None], msg="rowvec")


def test_duration_round_half_to_even(H, golden_dir):
    g = dict(np.load(golden_dir / "units.npz"))
    out = H.duration_round(torch.tensor(g["round/logd"]).cuda())
    np.testing.assert_array_equal(out.cpu().numpy(), g["round/out"])
    logd = torch.log(torch.tensor([0.5, 1.5, 2.5, 3.5, 0.2]) + 1)
    ref = torch.clamp(torch.round(torch.exp(logd) - 1) * 1.7, min=0).int()
    assert torch.equal(H.duration_round(logd.cuda(), 1.7).cpu(), ref)


@pytest.mark.parametrize("control", [1.0, 1.7])
def test_duration_round_dense_sweep_around_every_tie(H, control):
    """Integer output, bit-exact where it can flip: for every k in 0..399 the 129 floats around log(k + 1.5) (where
    exp(x) - 1 crosses k + 0.5; 51 600 inputs, ~90 of them exact ties) plus 200 000 random log-durations.  The
    reference is the reference's own expression on the CPU, ``clamp(round(exp(x) - 1) * control, min=0).int()``
    (fs2/variance_adaptor.py:360-366).  torch's CPU fp32 ``exp`` is a <= 1 ulp routine (it differs from the correctly
    rounded value on ~1 % of these inputs): where it IS correctly rounded the kernel must agree bit for bit, and
    where it is not, the kernel must give the answer of the correctly rounded exponential (float64 exp, rounded
    once)."""
    ks = np.arange(0, 400)
    x0 = np.log(ks + 1.5).astype(np.float32)
    xs = [x0.copy()]
    up, dn = x0.copy(), x0.copy()
    for _ in range(64):
        up = np.nextafter(up, np.float32(np.inf)).astype(np.float32)
        dn = np.nextafter(dn, np.float32(-np.inf)).astype(np.float32)
        xs += [up.copy(), dn.copy()]
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.from_numpy(np.concatenate(xs)), torch.rand(200000, generator=g) * 7 - 1])
    e32, e64 = torch.exp(x), torch.exp(x.double()).float()
    ref32 = torch.clamp(torch.round(e32 - 1) * control, min=0).int()
    ref64 = torch.clamp(torch.round(e64 - 1) * control, min=0).int()
    assert int(((e64 - 1) % 1 == 0.5).sum()) > 50  # the sweep does contain exact ties
    got = H.duration_round(x.cuda(), control).cpu()
    assert torch.equal(got, ref64)
    same = e32 == e64
    assert torch.equal(got[same], ref32[same])
    # (on the hosts seen so far the two references agree everywhere: report it if that ever changes)
    assert int((ref32 != ref64).sum()) <= 8, int((ref32 != ref64).sum())


@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout", [(2, 37, 80, 1, 32), (1, 5, 7, 1, 8), (3, 19, 40, 32, 32), (2, 10, 5, 64, 128), (1, 3, 2, 128, 128),
                                               (2, 8, 6, 6, 10),
                                               # direct weight-gradient route, more than 2048 output rows: 3 and 2 partials
                                               (3, 70, 80, 1, 32), (2, 90, 50, 3, 6)])
def test_conv2d_stride2_fwd_bwd(H, B, Hh, Ww, Cin, Cout):
    """GST reference-encoder convolution (3x3, stride 2, pad 1, no bias, channels-last): the gather + MFMA GEMM route
    (Cin, Cout multiples of 4) and the direct kernels (first layer / odd widths) against torch's conv2d."""
    g = torch.Generator().manual_seed(B * 100 + Hh)
    x = torch.randn(B, Cin, Hh, Ww, generator=g, requires_grad=True)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).requires_grad_(True)
    ref = F.conv2d(x, w, stride=2, padding=1)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    xc = x.detach().permute(0, 2, 3, 1).contiguous().cuda()           # [B, H, W, Cin]
    wc = w.detach().permute(2, 3, 1, 0).contiguous().cuda()           # [kh, kw, Cin, Cout]
    y = H.conv2d_s2_fwd(xc, wc)
    assert y.shape == (B, (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1, Cout)
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((y.cpu() - ref.detach().permute(0, 2, 3, 1)).abs().max()) < tol
    dw = torch.empty_like(wc)
    if Cin == 1:  # the first layer needs no input gradient: its weight gradient takes the padded-gather GEMM route
        dw1 = torch.empty_like(wc)
        assert H.conv2d_s2_bwd(dy.permute(0, 2, 3, 1).contiguous().cuda(), xc, wc, dw1, need_dx=False) is None
        assert float((dw1.cpu() - w.grad.permute(2, 3, 1, 0)).abs().max()) < 1e-4 * max(1.0, float(w.grad.abs().max()))
    if Cin % 4 or Cout % 4:
        assert H.lib().fs2hip_conv2d_s2_wgrad_parts(B, Hh, Ww) == -(-(B * y.shape[1] * y.shape[2]) // 2048)
    dx = H.conv2d_s2_bwd(dy.permute(0, 2, 3, 1).contiguous().cuda(), xc, wc, dw)
    assert float((dx.cpu() - x.grad.permute(0, 2, 3, 1)).abs().max()) < 2e-5 * max(1.0, float(x.grad.abs().max()))
    assert float((dw.cpu() - w.grad.permute(2, 3, 1, 0)).abs().max()) < 1e-4 * max(1.0, float(w.grad.abs().max()))


# ------------------------------------------------------------------------------------------------
# GST style encoder kernels (csrc/gst.hip) and the small helpers its branch uses.  References: float64 on the CPU
# from the fp32 inputs (tests/gst_references.py, checked without a GPU by tests/test_gst_reference_cpu.py).
# ------------------------------------------------------------------------------------------------
def rel_err(a, b):
    """The number ``close`` bounds: max |a - b| over max |b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-6)


def close_abs(a, b, tol=2e-5, msg=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert bool(torch.isfinite(a).all()), f"{msg}: not finite"
    err = float((a - b).abs().max())
    assert err < tol, f"{msg}: abs err {err:.3e}"


SENTINEL = -777.25


def _gru_gate_case(H, gi_all, gh, hprev, dh, check):
    """One ``gru_gate_fwd`` + ``gru_gate_bwd`` call on step t = 1 of gi_all [B, 3, 3U] (row stride 3 * 3U, the other
    steps hold different data) against ``gru_step_ref`` and its autograd.  ``dhprev`` is dh * z ONLY: the share of the
    recurrent matmul (dgh W_hh) is added by the caller, so the reference treats gh as a leaf of its own."""
    from tests import gst_references as R
    B, Hh, U3 = gi_all.shape
    U, t = U3 // 3, 1
    gi64, gh64, h64 = (v.double().requires_grad_(True) for v in (gi_all[:, t], gh, hprev))
    want, (r, z, n, hn) = R.gru_step_ref(gi64, gh64, h64)
    want.backward(dh.double())
    gi_d = gi_all.cuda()
    hnew, gates = H.gru_gate_fwd(gi_d.view(-1)[t * U3:], Hh * U3, gh.cuda(), hprev.cuda(), U)
    assert hnew.shape == (B, U) and gates.shape == (B, 4 * U)
    check(hnew, want, msg="h'")
    for i, (name, ref) in enumerate((("r", r), ("z", z), ("n", n), ("gh_n", hn))):
        check(gates[:, i * U:(i + 1) * U], ref, msg=f"gate {name}")
    rz = gates[:, :2 * U]
    assert float(rz.min()) >= 0.0 and float(rz.max()) <= 1.0
    dgi_all = torch.full((B, Hh, U3), SENTINEL, device="cuda")
    dgh, dhprev = H.gru_gate_bwd(dh.cuda(), gates, hprev.cuda(), dgi_all.view(-1)[t * U3:], Hh * U3, U)
    check(dgi_all[:, t], gi64.grad, msg="dgi")
    check(dgh, gh64.grad, msg="dgh")
    check(dhprev, h64.grad, msg="dhprev")
    other = dgi_all[:, [0, 2]].cpu()
    assert torch.equal(other.view(torch.int32), torch.full_like(other, SENTINEL).view(torch.int32)), "dgi rows of other steps"


GRU_SHAPES = [(1, 128), (3, 128), (64, 128), (5, 32), (2, 200)]


@pytest.mark.parametrize("B,U", GRU_SHAPES)
def test_gru_gate_step(H, B, U):
    _gru_gate_case(H, rnd(B, 3, 3 * U, seed=1), rnd(B, 3 * U, seed=2), rnd(B, U, seed=3), rnd(B, U, seed=4), close)


@pytest.mark.parametrize("B,U", GRU_SHAPES)
def test_gru_gate_step_saturated(H, B, U):
    """Pre-activations from {0, +-1e-3, +-20, +-87, +-89, +-100, +-1e4} mixed with random ones: ``fs2_sigmoid`` is
    rcp(1 + __expf(-x)), whose exponential overflows below x = -88.  Everything stays finite, r and z in [0, 1], and
    within 2e-5 ABSOLUTE (gates and tanh are bounded by 1).  A special value sits in gi OR in gh_n of an element,
    never both (1e4 - r * 1e4 is a cancellation no fp32 evaluation resolves)."""
    g = torch.Generator().manual_seed(B * 1000 + U)
    special = torch.tensor([0.0, 1e-3, -1e-3, 20, -20, 87, -87, 89, -89, 100, -100, 1e4, -1e4])
    gi_all, gh = rnd(B, 3, 3 * U, seed=1), rnd(B, 3 * U, seed=2)
    pick = special[torch.randint(0, len(special), (B, 3 * U), generator=g)]
    where = torch.rand(B, 3 * U, generator=g)
    in_gi = where < 0.6
    gi_all[:, 1] = torch.where(in_gi, pick, gi_all[:, 1])
    gh[:, :2 * U] = torch.where(in_gi[:, :2 * U] & (where[:, :2 * U] < 0.3), torch.zeros(()), gh[:, :2 * U])  # some exact
    gh[:, 2 * U:] = torch.where(where[:, 2 * U:] > 0.8, pick[:, 2 * U:], gh[:, 2 * U:])
    assert float(gi_all[:, 1].max()) == 1e4 or B * U < 64
    _gru_gate_case(H, gi_all, gh, rnd(B, U, seed=3), rnd(B, U, seed=4), close_abs)


def _ref_bound(err32, floor=2e-5, factor=4.0):
    """Allowed error of a multi-launch fp32 computation: 4x the error the fp32 CPU run of the SAME torch reference
    shows against its float64 run (the factor covers another summation order in the MFMA GEMMs and split-K), and never
    below the single-kernel tolerance of this file."""
    return max(floor, factor * err32)


@pytest.mark.parametrize("Hh", [1, 2, 11])
def test_gru_sequence_matches_nn_gru(H, Hh):
    """The GRU loop exactly as ``StyleEncoder.fwd`` / ``.bwd`` drive it, against ``nn.GRU(256, 128).double()``."""
    B, U, I = 3, 128, 256
    gru64 = torch.nn.GRU(I, U, batch_first=True).double()
    with torch.no_grad():
        for i, p in enumerate(gru64.parameters()):
            p.copy_(rnd(*p.shape, seed=20 + i, scale=U ** -0.5))
    x, dy = rnd(B, Hh, I, seed=1), rnd(B, U, seed=2)
    names = ("h_last", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh")

    def run(gru, dtype):
        xx = x.to(dtype).requires_grad_(True)
        _, h = gru(xx)
        (h[0] * dy.to(dtype)).sum().backward()
        return dict(zip(names, [h[0].detach(), xx.grad] + [p.grad for p in gru.parameters()]))

    want = run(gru64, torch.float64)
    gru32 = torch.nn.GRU(I, U, batch_first=True)
    gru32.load_state_dict({k: v.float() for k, v in gru64.state_dict().items()})
    ref32 = run(gru32, torch.float32)
    wih, whh, bih, bhh = (p.detach().float().cuda() for p in gru64.parameters())
    feat = x.reshape(B * Hh, I).cuda()                       # rows (b, t)
    gi = H.linear_fwd(feat, wih, bih)
    hs = H.zeros(Hh + 1, B, U, device="cuda")
    gates = []
    for t in range(Hh):
        gh = H.linear_fwd(hs[t], whh, bhh)
        _, g = H.gru_gate_fwd(gi.view(-1)[t * 3 * U:], Hh * 3 * U, gh, hs[t], U, hnew=hs[t + 1])
        gates.append(g)
    dh = dy.cuda()
    dgi = torch.empty(B * Hh, 3 * U, device="cuda")
    dgh_all = torch.empty(Hh, B, 3 * U, device="cuda")
    got = dict(h_last=hs[Hh].clone())
    try:
        for t in range(Hh - 1, -1, -1):
            _, dhprev = H.gru_gate_bwd(dh, gates[t], hs[t], dgi.view(-1)[t * 3 * U:], Hh * 3 * U, U, dgh=dgh_all[t])
            dh = H.axpby(dhprev, H.linear_bwd_data(dgh_all[t], whh))
        got["dW_hh"], got["db_hh"] = torch.empty(3 * U, U, device="cuda"), torch.empty(3 * U, device="cuda")
        got["dW_ih"], got["db_ih"] = torch.empty(3 * U, I, device="cuda"), torch.empty(3 * U, device="cuda")
        H.linear_bwd_weight(dgh_all.view(Hh * B, 3 * U), hs[:Hh].reshape(Hh * B, U), got["dW_hh"], bias_grad=got["db_hh"])
        H.linear_bwd_weight(dgi, feat, got["dW_ih"], bias_grad=got["db_ih"])
        got["dx"] = H.linear_bwd_data(dgi, wih).view(B, Hh, I)
        H.flush_grad_reductions()
    finally:
        H.drop_pending_reductions()
    report, failed = [], []
    for k in names:
        e32, e = rel_err(ref32[k], want[k]), rel_err(got[k], want[k])
        bound = _ref_bound(e32)
        report.append(f"{k}: kernel {e:.2e}, fp32 reference {e32:.2e}, bound {bound:.2e}")
        if not (e < bound):
            failed.append(k)
    print(f"GRU Hh={Hh}: " + "; ".join(report))
    assert not failed, (failed, report)


GST_ATTN_SHAPES = [(1, 10, 4), (5, 10, 4), (64, 10, 4), (3, 1, 4), (3, 32, 4), (2, 7, 1), (2, 13, 3)]


def _gst_attention_case(H, B, NT, heads, q_scale):
    from tests import gst_references as R
    F = heads * 64
    q, k, v, dctx = rnd(B, F, seed=1) * q_scale, rnd(NT, F, seed=2), rnd(NT, F, seed=3), rnd(B, F, seed=4)
    q64 = q.double().requires_grad_(True)
    k64 = k.double().unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)   # one leaf per utterance: dk_part, dv_part
    v64 = v.double().unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)
    p64, ctx64 = R.gst_attention_ref(q64, k64, v64, heads)
    (ctx64 * dctx.double()).sum().backward()
    p, ctx = H.gst_attn_fwd(q.cuda(), k.cuda(), v.cuda(), heads)
    assert p.shape == (B, heads, NT) and ctx.shape == (B, F)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ctx).all())
    close(p, p64, msg="p")
    assert float((p.double().sum(-1) - 1).abs().max()) < 2e-5
    close(ctx, ctx64, msg="ctx")
    dq, dkp, dvp = H.gst_attn_bwd(dctx.cuda(), q.cuda(), k.cuda(), v.cuda(), p, heads)
    assert dkp.shape == (B, NT, F) and dvp.shape == (B, NT, F)
    close(dq, q64.grad, msg="dq")
    close(dkp, k64.grad, msg="dk_part")
    close(dvp, v64.grad, msg="dv_part")
    return p64


@pytest.mark.parametrize("B,NT,heads", GST_ATTN_SHAPES)
def test_gst_attention(H, B, NT, heads):
    _gst_attention_case(H, B, NT, heads, 1.0)


def test_gst_attention_near_one_hot(H):
    """q scaled until the scores reach +-60: the softmax is one-hot to fp32 for many (utterance, head) pairs."""
    p64 = _gst_attention_case(H, 5, 10, 4, 30.0)
    s = rnd(5, 256, seed=1).double().view(5, 4, 1, 64) * 30.0 * rnd(10, 256, seed=2).double().view(10, 4, 64).transpose(0, 1)
    assert float(s.sum(-1).abs().max()) / 8 > 60 and float(p64.max()) > 0.999999


def test_gst_attention_refuses_unsupported_sizes(H):
    """More than 32 tokens or more than 4 heads: the entry points return EINVAL before launching anything (their
    per-thread score array holds 32 entries and a workgroup has four wavefronts), and the binding raises."""
    for B, NT, heads in ((2, 33, 4), (2, 10, 5)):
        F = heads * 64
        q, k, v = rnd(B, F, seed=1).cuda(), rnd(NT, F, seed=2).cuda(), rnd(NT, F, seed=3).cuda()
        with pytest.raises(RuntimeError, match="invalid arguments"):
            H.gst_attn_fwd(q, k, v, heads)
        with pytest.raises(RuntimeError, match="invalid arguments"):
            H.gst_attn_bwd(q, q, k, v, torch.zeros(B, heads, NT, device="cuda"), heads)
        outs = [torch.full(s, SENTINEL, device="cuda") for s in ((B, heads, NT), (B, F), (B, F), (B, NT, F), (B, NT, F))]
        p, ctx, dq, dk, dv = outs
        L, st = H.lib(), H._stream()
        assert L.fs2hip_gst_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), p.data_ptr(), ctx.data_ptr(), B, NT, heads, st) == -22
        pin = torch.zeros(B, heads, NT, device="cuda")
        assert L.fs2hip_gst_attn_bwd(q.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), pin.data_ptr(), dq.data_ptr(),
                                     dk.data_ptr(), dv.data_ptr(), B, NT, heads, st) == -22
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == SENTINEL).all())


ACTS = ["relu", "silu", "tanh", None]
ACT_EDGES = torch.tensor([0.0, -0.0, 88.0, -88.0, 100.0, -100.0, 1e-3, -1e-3, 20.0, -20.0, 89.0, -89.0])


def _act64(act, x):
    return {"relu": lambda t: t.clamp(min=0), "silu": lambda t: t * torch.sigmoid(t), "tanh": torch.tanh, None: lambda t: t}[act](x)


def _dact64(act, x):
    if act == "silu":
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    if act == "tanh":
        return 1 - torch.tanh(x) ** 2
    return (x > 0).double() if act == "relu" else torch.ones_like(x)


@pytest.mark.parametrize("act", ACTS)
def test_act_apply(H, act):
    """n = 1, n = 1000 and a size past the 4096-workgroup cap (grid-stride loop), with the values where SiLU's fast
    sigmoid saturates.  The edge values and the random rest are compared separately: the +-100 would otherwise set
    the scale of the whole comparison."""
    for n in (1, 1000, 4096 * 256 + 777):
        x = rnd(n, seed=n) * 2
        ne = min(n, len(ACT_EDGES)) if n > 1 else 0
        x[:ne] = ACT_EDGES[:ne]
        out = H.act_apply(x.cuda(), act)
        ref = _act64(act, x.double())
        assert bool(torch.isfinite(out).all())
        close(out[ne:], ref[ne:], msg=f"act_apply {act} n={n}")
        if ne:
            close(out[:ne], ref[:ne], msg=f"act_apply {act} edges")
        if act in ("relu", None):
            assert torch.equal(out.cpu(), ref.float())
    xin = torch.tensor([-100.0]).cuda()
    H.act_apply(xin, act)
    assert float(xin) == -100.0  # (out of place)


@pytest.mark.parametrize("act", ACTS)
def test_dact_mul(H, act):
    """out = dy * act'(aux); aux is the activation's OUTPUT for ReLU (with exact zeros) and its input otherwise.  Past
    the 8192-workgroup cap."""
    n = 8192 * 256 + 5
    x, dy = rnd(n, seed=1) * 2, rnd(n, seed=2)
    x[:len(ACT_EDGES)] = ACT_EDGES
    aux = x.clamp(min=0) if act == "relu" else x
    if act == "relu":
        assert int((aux == 0).sum()) > n // 3
    out = H.dact_mul(dy.cuda(), aux.cuda(), act)
    ref = dy.double() * _dact64(act, aux.double())
    assert bool(torch.isfinite(out).all())
    close(out, ref, msg=f"dact_mul {act}")
    close(out[:len(ACT_EDGES)], ref[:len(ACT_EDGES)], msg=f"dact_mul {act} edges")
    close(out[-300:], ref[-300:], msg=f"dact_mul {act} tail")
    if act in ("relu", None):
        assert torch.equal(out.cpu(), ref.float())


def test_scale_dev(H):
    """x *= s with s in device memory: one fp32 multiply per element (exactly the CPU product), and NOTHING is
    rewritten when s is exactly 1 (NaN payloads and -0.0 keep their bits).  Past the 8192-workgroup cap."""
    n = 8192 * 256 + 3
    x = rnd(n, seed=1)
    x[1] = -0.0
    special = x.clone()
    special[0] = float("nan")
    bits = special.view(torch.int32).clone()
    bits[2] = 0x7FC12345  # a NaN with a payload
    special = bits.view(torch.float32)
    d = special.cuda()
    assert H.scale_dev(d, torch.tensor([1.0], device="cuda")) is d
    assert torch.equal(d.cpu().view(torch.int32), bits)
    for s in (0.37, 0.0):
        st = torch.tensor([s])
        d = x.cuda()
        H.scale_dev(d, st.cuda())
        assert torch.equal(d.cpu(), x * st), f"scale_dev {s}"
    assert float(d[-1]) == 0.0 and float(d.abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 7, 16])
def test_sum_slots(H, n):
    x = rnd(16, seed=n, scale=100.0)
    buf = torch.full((5,), SENTINEL, device="cuda")
    H.sum_slots(x.cuda(), n, buf[2:3])
    seq = np.float32(0)
    for v in x[:n].numpy():
        seq = np.float32(seq + v)
    assert float(buf[2]) == float(seq)
    close(buf[2:3], x[:n].double().sum().reshape(1), msg="sum_slots")
    assert buf.cpu()[[0, 1, 3, 4]].tolist() == [SENTINEL] * 4


def test_mask_from_lens(H):
    T = 37
    lens = torch.tensor([0, 1, T - 1, T, T + 5, 12, 36], dtype=torch.int32)
    assert (lens.numel() * T) % 256
    mask = H.mask_from_lens(lens.cuda(), T)
    assert mask.dtype == torch.bool and mask.shape == (7, T)
    assert torch.equal(mask.cpu(), torch.arange(T)[None, :] < lens[:, None])
    assert torch.equal(mask.view(torch.uint8).cpu(), (torch.arange(T)[None, :] < lens[:, None]).to(torch.uint8))


@pytest.mark.parametrize("B,T,D", [(1, 1, 256), (3, 70, 256), (48, 5, 256), (49, 5, 256), (64, 33, 256), (2, 1300, 80)])
def test_segment_colsum(H, B, T, D):
    """Per-utterance sums over time; ``REDUCE_MAX_JOBS`` = 48 utterances per launch, so B = 49 and 64 take two."""
    assert H.REDUCE_MAX_JOBS == 48
    x = rnd(B, T, D, seed=B + T) + 0.25 * torch.arange(B)[:, None, None]  # (utterances differ in their mean as well)
    out = torch.empty(B, D, device="cuda")
    assert H.segment_colsum(x.cuda(), out) is out
    close(out, x.double().sum(1), 1e-4, "segment_colsum")
    for b in (0, B - 1, min(B - 1, 48)):
        close(out[b], x[b].double().sum(0), 1e-4, f"segment_colsum utterance {b}")


def test_colsum_grad_deferred(H):
    """``colsum_grad`` + ``flush_grad_reductions``: one partial row (finished at once), several (deferred), and more
    pending jobs than one launch takes.  ``reduce_rows_multi_kernel`` adds the partial rows in the order of
    ``reduce_rows_small_kernel`` (16 row lanes, four-at-a-time then singly, lanes summed 0..15), so the deferred result is
    ``colsum``'s bit for bit."""
    assert not H._PENDING_REDUCTIONS
    L = H.lib()
    cases = [(64, 256), (300, 256), (65, 80), (1234, 512)] + [(130 + i, 64 + 4 * (i % 5)) for i in range(50)]
    assert L.fs2hip_colsum_rows(64) == 1 and L.fs2hip_colsum_rows(65) == 2 and L.fs2hip_colsum_rows(300) == 5
    try:
        xs, outs = [], []
        for i, (M, N) in enumerate(cases):
            x = (rnd(M, N, seed=i) + 0.1 * i).cuda()
            out = torch.full((N,), SENTINEL, device="cuda")
            assert H.colsum_grad(x, out) is out
            xs.append(x); outs.append(out)
        assert len(H._PENDING_REDUCTIONS) == len(cases) - 1 > H.REDUCE_MAX_JOBS
        close(outs[0], xs[0].double().sum(0), 1e-4, "colsum_grad, one partial row")
        assert bool((outs[1] == SENTINEL).all())  # (not written before the flush)
        used = H.flush_grad_reductions()
        assert len(used) == len(cases) - 1 and not H._PENDING_REDUCTIONS
        for (M, N), x, out in zip(cases, xs, outs):
            close(out, x.double().sum(0), 1e-4, f"colsum_grad {M}x{N}")
            assert torch.equal(out, H.colsum(x, torch.empty(N, device="cuda"))), f"colsum_grad vs colsum {M}x{N}"
    finally:
        H.drop_pending_reductions()
    assert not H._PENDING_REDUCTIONS and not H._PENDING_SLABS


# rowdot_bwd: 16 rows per workgroup; from 8 workgroups on (every real step: M >= 128) the partial sums are reduced by
# fs2_reduce_rows in one launch, below that by two reduce_slabs launches.
@pytest.mark.parametrize("C", [256, 80])
@pytest.mark.parametrize("B,T", [(7, 16), (8, 16), (3, 43), (32, 128), (32, 648)])
def test_rowdot_reduction_branches(H, B, T, C):
    M = B * T
    nblk = H.lib().fs2hip_rowdot_blocks(M)
    assert nblk == (M + 15) // 16
    assert (nblk >= 8) == (M != 16 * 7), "the branch condition of fs2hip_rowdot_bwd moved"  # M = 112: reduce_slabs twice
    g = torch.Generator().manual_seed(M + C)
    x, w, b = rnd(B, T, C, seed=M), rnd(C, seed=C, scale=0.1), rnd(1, seed=3)
    lens = torch.randint(1, T + 1, (B,), generator=g).to(torch.int32)
    lens[0], lens[B // 2] = T, 0
    dout = torch.randn(B, T, generator=g)
    mask = torch.arange(T)[None, :] < lens[:, None]
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = (xr @ wr + br) * mask
    (ref * dout.double()).sum().backward()
    out = H.rowdot_fwd(x.cuda(), w.cuda(), b.cuda(), lens.cuda(), B, T)
    close(out, ref, msg="rowdot fwd")
    assert bool((out.cpu()[~mask] == 0).all())
    dw, db = torch.empty(C, device="cuda"), torch.empty(1, device="cuda")
    dx = H.rowdot_bwd(dout.cuda(), x.cuda(), w.cuda(), lens.cuda(), dw, db, B, T)
    close(dx, xr.grad, msg="dx")
    close(dw, wr.grad, msg="dw")
    close(db, br.grad, msg="dbias")
    assert bool((dx.cpu()[~mask] == 0).all())


# masked_loss: at most 1024 workgroups of 256 threads, so the mel loss at the benchmark size (32 x 648 x 80 = 1.66 M
# elements) walks its grid-stride loop seven times; (32, 648, 1) is 81 workgroups, one pass.
@pytest.mark.parametrize("kind", ["mse", "mae"])
@pytest.mark.parametrize("B,T,Cc", [(32, 648, 80), (32, 648, 1)])
def test_masked_loss_full_size(H, B, T, Cc, kind):
    assert (B * T * Cc > 1024 * 256) == (Cc == 80)
    g = torch.Generator().manual_seed(B * T * Cc)
    lens = torch.randint(1, T + 1, (B,), generator=g).to(torch.int32)
    lens[0], lens[5] = T, 0  # an utterance of length 0
    mask = (torch.arange(T)[None, :] < lens[:, None])[..., None]
    pred, tgt = torch.randn(B, T, Cc, generator=g), torch.randn(B, T, Cc, generator=g)
    same = torch.rand(B, T, Cc, generator=g) < 0.1
    pred[same] = tgt[same]  # |0| has gradient sign(0) = 0
    pr = pred.double().requires_grad_(True)
    fn = F.mse_loss if kind == "mse" else F.l1_loss
    ref = fn(pr * mask, tgt.double() * mask) * 0.1
    ref.backward()
    slot = torch.zeros(1, device="cuda")
    d = H.masked_loss(pred.cuda(), tgt.cuda(), lens.cuda(), B, T, Cc, kind=kind, weight=0.1, loss_out=slot)
    close(slot, ref.detach().reshape(1), msg=f"{kind} value")
    close(d, pr.grad, msg=f"{kind} grad")
    dc = d.cpu()
    assert bool((same & mask).any()) and bool((dc[same] == 0).all()), "gradient where pred == target"
    assert bool((dc[~mask.expand_as(dc)] == 0).all()), "gradient beyond the utterance"
    slot2 = torch.zeros(1, device="cuda")
    assert H.masked_loss(pred.cuda(), tgt.cuda(), lens.cuda(), B, T, Cc, kind=kind, weight=0.1, loss_out=slot2,
                         want_grad=False) is None
    assert torch.equal(slot, slot2)


@pytest.mark.parametrize("kind", ["mse", "mae"])
def test_masked_loss_int_duration_target_full_size(H, kind):
    """The duration loss' target form, log(int + 1), at 32 x 128 tokens with an empty utterance."""
    B, T = 32, 128
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(1, T + 1, (B,), generator=g).to(torch.int32)
    lens[0], lens[9] = T, 0
    mask = torch.arange(T)[None, :] < lens[:, None]
    dur = torch.randint(0, 40, (B, T), generator=g).to(torch.int32)
    pred = torch.randn(B, T, generator=g) + 1.5
    pr = pred.double().requires_grad_(True)
    fn = F.mse_loss if kind == "mse" else F.l1_loss
    ref = fn(pr * mask, torch.log(dur.double() + 1) * mask) * 0.1
    ref.backward()
    slot = torch.zeros(1, device="cuda")
    d = H.masked_loss(pred.cuda(), dur.cuda(), lens.cuda(), B, T, 1, kind=kind, weight=0.1, loss_out=slot)
    close(slot, ref.detach().reshape(1), msg=f"{kind} duration value")
    close(d, pr.grad, msg=f"{kind} duration grad")
