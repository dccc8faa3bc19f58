"""GPU: the depthwise convolution at widths no kernel is instantiated for (conv.hip's run-time-K kernels) against
PyTorch, in every form the model uses; and, with FS2_DWCONV_GENERIC=1, the run-time-K kernels at the six instantiated
widths giving the instantiated kernels' bits."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KS = (1, 11, 13, 17, 21, 33, 63)
BUILT = (3, 5, 7, 9, 15, 31)


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


@pytest.mark.parametrize("glu", [True, False])
@pytest.mark.parametrize("T", [5, 70, 200])
@pytest.mark.parametrize("C", [256, 80, 32])
@pytest.mark.parametrize("K", KS)
def test_dwconv_any_width(H, K, C, T, glu):
    """Forward, fused BatchNorm statistics, dx, dw and dbias against F.conv1d (C = 256: the tiled kernels in the GLU
    form; 80 and 32: the per-thread-window ones).  T = 5 with K = 33 or 63: the kernel is wider than the sequence."""
    B = 2
    x = rnd(B, T, 2 * C if glu else C, seed=K + 1).requires_grad_(True)
    w = rnd(C, 1, K, seed=K + 2, scale=0.3).requires_grad_(True)
    b = rnd(C, seed=K + 3).requires_grad_(True)
    a = F.glu(x, dim=-1) if glu else x
    ref = F.conv1d(a.transpose(1, 2), w, b, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    wk = w.detach()[:, 0, :].t().contiguous().cuda()  # [K, C]
    y, parts = H.dwconv_fwd(x.detach().cuda(), wk, b.detach().cuda(), B, T, glu=glu, stats=True)
    close(y, ref, msg="dwconv fwd")
    stripes = [ref[bb, t0:t0 + 64].double() for bb in range(B) for t0 in range(0, T, 64)]
    assert parts.nparts == len(stripes)
    close(parts.partial[:, 0], torch.stack([sp.mean(0) for sp in stripes]), 1e-5, "stripe means")
    close(parts.partial[:, 1], torch.stack([((sp - sp.mean(0)) ** 2).sum(0) for sp in stripes]), 1e-5, "stripe M2")
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    st = H.bn_finalize(parts, one, zero, None, None, training=True)
    flat = ref.reshape(-1, C).double()
    close(st[2], flat.mean(0), 1e-5, "fused mean")
    close(st[3], 1 / torch.sqrt(flat.var(0, unbiased=False) + 1e-5), 1e-5, "fused invstd")
    dy = rnd(B, T, C, seed=K + 4)
    ref.backward(dy)
    dw, db = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
    dx = H.dwconv_bwd(dy.cuda(), x.detach().cuda(), wk, dw, db, B, T, glu=glu)
    close(dx, x.grad, msg="dwconv dx")
    close(dw, w.grad[:, 0, :].t(), 1e-4, "dwconv dw")
    close(db, b.grad, 1e-4, "dwconv db")


@pytest.mark.parametrize("K,C,T", [(17, 256, 200), (33, 256, 70), (63, 64, 130), (11, 80, 70), (21, 32, 5)])
def test_dwconv_any_width_bf16_forms(H, K, C, T):
    """bf16 tensors (GLU form) give what the fp32 kernels give on the same rounded values; the plain fp32-in / bf16-out
    form gives the rounded fp32 result."""
    B = 2
    g = torch.Generator().manual_seed(T + K)
    x = torch.randn(B * T, 2 * C, generator=g).bfloat16().cuda()
    w = (0.3 * torch.randn(K, C, generator=g)).cuda()
    bias = (0.1 * torch.randn(C, generator=g)).cuda()
    y32, _ = H.dwconv_fwd(x.float(), w, bias, B, T, glu=True, stats=True)
    yb, partsb = H.dwconv_fwd(x, w, bias, B, T, glu=True, stats=True)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, y32.bfloat16())
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    st_b = H.bn_finalize(partsb, gam, bet, None, None)
    st_r = H.bn_finalize(H.colstats(yb.float().view(B * T, C)), gam, bet, None, None)
    assert (st_b[2] - st_r[2]).abs().max().item() < 1e-5 and ((st_b[3] - st_r[3]).abs() / st_r[3]).max().item() < 1e-5
    dy = torch.randn(B, T, C, generator=g).bfloat16().cuda()
    dw32, db32 = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
    dwb, dbb = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
    dx32 = H.dwconv_bwd(dy.float(), x.float(), w, dw32, db32, B, T, glu=True, out_dtype=torch.bfloat16)
    dxb = H.dwconv_bwd(dy, x, w, dwb, dbb, B, T, glu=True, out_dtype=torch.bfloat16)
    assert torch.equal(dxb, dx32) and torch.equal(dwb, dw32) and torch.equal(dbb, db32)
    xp = torch.randn(B * T, C, generator=g).cuda()
    yp = H.dwconv_fwd(xp, w, bias, B, T, out_dtype=torch.bfloat16)[0]
    assert yp.dtype == torch.bfloat16 and torch.equal(yp, H.dwconv_fwd(xp, w, bias, B, T)[0].bfloat16())


@pytest.mark.parametrize("K", [2, 8, 65])
def test_unsupported_width_is_refused(H, K):
    C, B, T = 64, 1, 20
    x, w = torch.randn(B * T, C, device="cuda"), torch.randn(K, C, device="cuda")
    with pytest.raises(ValueError, match="odd, 1 to 63"):
        H.dwconv_fwd(x, w, None, B, T)
    with pytest.raises(ValueError, match="odd, 1 to 63"):
        H.dwconv_bwd(torch.randn(B, T, C, device="cuda"), x, w, torch.empty_like(w), None, B, T)


def _all_forms(H, K, C, T):
    """Every variant of the four kernel families at one shape: a list of (name, tensor)."""
    B = 2
    g = torch.Generator().manual_seed(100 * K + C)
    x2 = torch.randn(B * T, 2 * C, generator=g).cuda()
    x1 = torch.randn(B * T, C, generator=g).cuda()
    w = (0.3 * torch.randn(K, C, generator=g)).cuda()
    bias = (0.1 * torch.randn(C, generator=g)).cuda()
    dy = torch.randn(B, T, C, generator=g).cuda()
    out = []
    for glu, x in ((True, x2), (False, x1)):
        for stats in (True, False):
            y, p = H.dwconv_fwd(x, w, bias, B, T, glu=glu, stats=stats)
            out += [(f"y glu={glu} stats={stats}", y)] + ([(f"partial glu={glu}", p.partial)] if stats else [])
        for od in (torch.float32, torch.bfloat16):
            dw, db = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
            dx = H.dwconv_bwd(dy, x, w, dw, db, B, T, glu=glu, out_dtype=od)
            out += [(f"dx glu={glu} {od}", dx), (f"dw glu={glu} {od}", dw), (f"db glu={glu} {od}", db)]
    xb, dyb = x2.bfloat16(), dy.bfloat16()
    for stats in (True, False):
        y, p = H.dwconv_fwd(xb, w, bias, B, T, glu=True, stats=stats)
        out += [(f"y bf16 stats={stats}", y)] + ([("partial bf16", p.partial)] if stats else [])
    dw, db = torch.empty(K, C, device="cuda"), torch.empty(C, device="cuda")
    dx = H.dwconv_bwd(dyb, xb, w, dw, db, B, T, glu=True, out_dtype=torch.bfloat16)
    out += [("dx bf16", dx), ("dw bf16", dw), ("db bf16", db)]
    out.append(("y fp32 -> bf16", H.dwconv_fwd(x1, w, bias, B, T, out_dtype=torch.bfloat16)[0]))
    return out


@pytest.mark.parametrize("C,tiles", [(256, "1"), (256, "0"), (80, "1")])
@pytest.mark.parametrize("K", BUILT)
def test_generic_kernels_give_the_instantiated_widths_bits(H, K, C, tiles, monkeypatch):
    """FS2_DWCONV_GENERIC=1 sends the six instantiated widths to the run-time-K kernels: the same operations in the
    same order, so y, statistics partials, dx, dw and dbias are equal bit for bit in every variant (C = 256 with the
    tiled kernels, and C = 256 / 80 on the per-thread-window ones)."""
    monkeypatch.setenv("FS2_DWCONV_TILE", tiles)
    monkeypatch.delenv("FS2_DWCONV_GENERIC", raising=False)
    want = _all_forms(H, K, C, 200)
    monkeypatch.setenv("FS2_DWCONV_GENERIC", "1")
    got = _all_forms(H, K, C, 200)
    for (name, a), (_, b) in zip(want, got):
        assert torch.equal(a, b), (K, C, tiles, name, float((a.float() - b.float()).abs().max()))
