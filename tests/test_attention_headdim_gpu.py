"""GPU: attention at head dimensions the kernels are not built for (any integer 1..256).  16 / 32 / 64 / 128 run as
they are; the others run zero-padded to the next of 16 / 32 / 64 / 128 / 256 with the softmax scale 1/sqrt(HD) of the
true head dimension (``hip.attention_padded_dim``; 256 itself is the 256-wide first-generation instance, no padding).
Every fresh float allocation of this file is poisoned with NaN, so a pad column or output element no kernel writes
shows up."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    """NaN in every fresh CUDA float tensor (the same hook as tests/conftest.py's ``poison_fresh_allocations``)."""
    from fastspeech2_lightning_amd import plan
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.is_floating_point() and t.numel():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: poisoned(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poisoned(real_empty_like(*a, **k)))
    monkeypatch.setattr(plan, "GUARD_ALLOW", plan.GUARD_ALLOW | {"fill_"})


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    hip.lib()
    return hip


@pytest.fixture
def precision(H):
    saved = H.get_precision()
    yield H.set_precision
    H.set_precision(saved)


def ref_attention(qkv, lens, B, T, Hh):
    """Plain fp32 softmax(Q K^T / sqrt(HD) + key-padding mask) V per head, and the log-sum-exp of each query row."""
    D = qkv.shape[-1] // 3
    hd = D // Hh
    q, k, v = qkv.view(B, T, 3, Hh, hd).permute(2, 0, 3, 1, 4)  # each (B, H, T, hd)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    pad = torch.arange(T)[None, :] >= lens[:, None]
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, D), torch.logsumexp(s, dim=-1)


def inputs(B, T, D, lens, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 3 * D, generator=g), torch.randn(B, T, D, generator=g), torch.tensor(lens, dtype=torch.int32)


HEAD_DIMS = (8, 24, 48, 80, 96, 112, 160, 192, 256)
SHAPES = [  # B, T, H, lens: a length-1 row, odd T, T = 130
    (3, 130, 2, [130, 64, 1]),
    (2, 37, 2, [37, 5]),
]
CASES = [(hd,) + s for hd in HEAD_DIMS for s in SHAPES] + [
    (96, 4, 648, 2, [648, 500, 40, 333]),
    (256, 4, 648, 2, [648, 500, 40, 333]),
]


@pytest.mark.parametrize("hd,B,T,Hh,lens", CASES)
def test_forward_and_backward_against_pytorch(H, hd, B, T, Hh, lens):
    D = Hh * hd
    qkv, dout, lens_t = inputs(B, T, D, lens, seed=hd * 7 + T)
    qr = qkv.clone().requires_grad_(True)
    ref, ref_lse = ref_attention(qr, lens_t, B, T, Hh)
    ref.backward(dout)
    gscale = qr.grad.abs().max().item()
    q_d, l_d, do_d = qkv.cuda(), lens_t.cuda(), dout.cuda()
    o, lse = H.attention_fwd(q_d, l_d, B, T, Hh)
    assert o.shape == (B, T, D) and lse.shape == (B, Hh, T)
    assert (o.cpu() - ref).abs().max() < 2e-5 * max(1.0, ref.abs().max().item())
    assert (lse.cpu() - ref_lse).abs().max() < 2e-5 * max(1.0, ref_lse.abs().max().item())
    dqkv = H.attention_bwd(q_d, l_d, o, do_d, lse, B, T, Hh)
    assert dqkv.shape == qkv.shape
    err = (dqkv.cpu() - qr.grad).abs().max().item()
    assert err < 3e-5 * gscale, f"dqkv err {err} scale {gscale}"
    # the training forward's kept scores and the backward that reads them (padded widths 64 / 128)
    if H.attention_scores_kept(hd):
        o2, lse2, sc = H.attention_fwd(q_d, l_d, B, T, Hh, save_scores=True)
        assert sc is not None and sc.shape == (B, Hh, T, (T + 31) // 32 * 32)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)
        got = H.attention_bwd(q_d, l_d, o2, do_d, lse2, B, T, Hh, scores=sc)
        err = (got.cpu() - qr.grad).abs().max().item()
        assert err < 3e-5 * gscale, f"dqkv (kept scores) err {err} scale {gscale}"
    else:
        assert H.attention_padded_dim(hd) not in (64, 128)


def test_padded_widths(H):
    want = {1: 16, 8: 16, 16: 16, 17: 32, 24: 32, 33: 64, 48: 64, 64: 64, 65: 128, 80: 128, 96: 128, 112: 128,
            128: 128, 129: 256, 160: 256, 192: 256, 255: 256, 256: 256, 0: 0, 257: 0, 512: 0}
    assert {hd: H.attention_padded_dim(hd) for hd in want} == want


@pytest.mark.parametrize("hd", [96, 192])
def test_bf16_mixed(H, precision, hd):
    """Same bounds as tests/test_attention_gpu.py::test_attention_bf16_mixed at HD 128: against the fp32 reference on
    bf16-rounded Q, K, V, dO, outputs within 1e-2 of scale, gradients within 2e-2, and not fp32-exact."""
    B, T, Hh, lens = 3, 130, 2, [130, 64, 1]
    qkv, dout, lens_t = inputs(B, T, Hh * hd, lens, seed=hd + 1)
    qr = qkv.bfloat16().float().requires_grad_(True)
    ref, ref_lse = ref_attention(qr, lens_t, B, T, Hh)
    ref.backward(dout.bfloat16().float())
    precision("bf16-mixed")
    o, lse = H.attention_fwd(qkv.cuda(), lens_t.cuda(), B, T, Hh)
    dqkv = H.attention_bwd(qkv.cuda(), lens_t.cuda(), o, dout.cuda(), lse, B, T, Hh)
    eo = (o.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    el = (lse.cpu() - ref_lse).abs().max().item() / max(1.0, ref_lse.abs().max().item())
    eg = (dqkv.cpu() - qr.grad).abs().max().item() / qr.grad.abs().max().item()
    assert eo < 1e-2 and el < 1e-2 and eg < 2e-2, (eo, el, eg)
    assert eo > 2e-5 or eg > 3e-5, "bf16 operands requested, fp32-exact result: the bf16 kernels did not run"


@pytest.mark.parametrize("hd", [96, 192])
def test_split(H, precision, hd):
    """"32-split": the fp32 bounds (tests/test_attention_gpu.py::test_attention_split), kept-scores forms included."""
    B, T, Hh, lens = 3, 130, 2, [130, 64, 1]
    qkv, dout, lens_t = inputs(B, T, Hh * hd, lens, seed=hd + 2)
    qr = qkv.clone().requires_grad_(True)
    ref, ref_lse = ref_attention(qr, lens_t, B, T, Hh)
    ref.backward(dout)
    gscale = qr.grad.abs().max().item()
    precision("32-split")
    q_d, l_d, do_d = qkv.cuda(), lens_t.cuda(), dout.cuda()
    o, lse = H.attention_fwd(q_d, l_d, B, T, Hh)
    assert (o.cpu() - ref).abs().max() < 2e-5 * max(1.0, ref.abs().max().item())
    assert (lse.cpu() - ref_lse).abs().max() < 2e-5 * max(1.0, ref_lse.abs().max().item())
    dqkv = H.attention_bwd(q_d, l_d, o, do_d, lse, B, T, Hh)
    assert (dqkv.cpu() - qr.grad).abs().max().item() < 3e-5 * gscale
    o2, lse2, sc = H.attention_fwd(q_d, l_d, B, T, Hh, save_scores=True)
    assert (sc is not None) == (hd == 96)
    got = H.attention_bwd(q_d, l_d, o2, do_d, lse2, B, T, Hh, scores=sc)
    assert (got.cpu() - qr.grad).abs().max().item() < 3e-5 * gscale


def _pad_by_hand(x, B, T, groups, hd, hdp):
    out = torch.zeros(B, T, groups, hdp, dtype=x.dtype, device=x.device)
    out[..., :hd] = x.view(B, T, groups, hd)
    return out.reshape(B, T, groups * hdp)


@pytest.mark.parametrize("kept", [False, True])
def test_padding_is_invisible_with_dropout(H, kept):
    """HD 96 with attention dropout 0.2 equals the HD 128 kernels run on the same tensors zero-padded by hand, with Q
    pre-scaled by sqrt(128/96) and dQ scaled back: to 1e-6 relative -- the mask indexing does not see the head width, and
    the scale is 1/sqrt(96)."""
    B, T, Hh, hd, hdp, lens = 3, 130, 2, 96, 128, [130, 77, 1]
    qkv, dout, lens_t = (t.cuda() for t in inputs(B, T, Hh * hd, lens, seed=4))
    drop = H.Drop(0.2, 1234)
    c = math.sqrt(hdp / hd)
    q, k, v = qkv.split(Hh * hd, dim=-1)
    qkv_p = torch.cat([_pad_by_hand(q * c, B, T, Hh, hd, hdp), _pad_by_hand(k, B, T, Hh, hd, hdp),
                       _pad_by_hand(v, B, T, Hh, hd, hdp)], dim=-1).contiguous()
    dout_p = _pad_by_hand(dout, B, T, Hh, hd, hdp).contiguous()

    def fwd(x):
        r = H.attention_fwd(x, lens_t, B, T, Hh, drop, save_scores=kept)
        return r if kept else (r[0], r[1], None)

    o, lse, sc = fwd(qkv)
    o_p, lse_p, sc_p = fwd(qkv_p)
    assert (sc is None) == (sc_p is None) == (not kept)
    o_cut = o_p.view(B, T, Hh, hdp)[..., :hd].reshape(B, T, Hh * hd)
    assert torch.equal(o_p.view(B, T, Hh, hdp)[..., hd:], torch.zeros_like(o_p.view(B, T, Hh, hdp)[..., hd:]))
    assert float((o - o_cut).abs().max()) <= 1e-6 * float(o_cut.abs().max())
    assert float((lse - lse_p).abs().max()) <= 1e-6 * float(lse_p.abs().max())
    dqkv = H.attention_bwd(qkv, lens_t, o, dout, lse, B, T, Hh, drop, scores=sc)
    dqkv_p = H.attention_bwd(qkv_p, lens_t, o_p, dout_p, lse_p, B, T, Hh, drop, scores=sc_p)
    parts = [g.view(B, T, Hh, hdp)[..., :hd].reshape(B, T, Hh * hd) for g in dqkv_p.split(Hh * hdp, dim=-1)]
    want = torch.cat([parts[0] * c, parts[1], parts[2]], dim=-1)
    assert float((dqkv - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # and dropout did act
    o0, _ = H.attention_fwd(qkv, lens_t, B, T, Hh)
    assert float((o - o0).abs().max()) > 1e-3


PAD_ENTRY_POINTS = ("fs2hip_attention_pad_heads", "fs2hip_attention_unpad_heads")


@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_built_head_dims_keep_their_route(H, monkeypatch, hd):
    """Head dims 16 / 32 / 64 / 128 launch no pad or unpad kernel (those entry points raise here if called), with and
    without kept scores, and the returned o and dqkv are the very tensors the kernels wrote: no copy."""
    L = H.lib()

    def refuse(*a, **k):
        raise AssertionError("padded attention route taken for a built head dimension")

    for name in PAD_ENTRY_POINTS:
        monkeypatch.setattr(L, name, refuse)
    written = {}
    for name, out in (("fs2hip_attention_fwd", 2), ("fs2hip_attention_bwd", 9)):  # the positions of o and dqkv
        def spy(*a, _real=getattr(L, name), _name=name, _out=out):
            written[_name] = a[_out]
            return _real(*a)
        monkeypatch.setattr(L, name, spy)
    B, T, Hh, lens = 2, 37, 2, [37, 5]
    qkv, dout, lens_t = (t.cuda() for t in inputs(B, T, Hh * hd, lens, seed=hd))
    for kept in (False, True):
        if kept:
            o, lse, sc = H.attention_fwd(qkv, lens_t, B, T, Hh, save_scores=True)
        else:
            (o, lse), sc = H.attention_fwd(qkv, lens_t, B, T, Hh), None
        assert o.shape == (B, T, Hh * hd) and o.data_ptr() == written["fs2hip_attention_fwd"]
        dqkv = H.attention_bwd(qkv, lens_t, o, dout, lse, B, T, Hh, scores=sc)
        assert dqkv.shape == qkv.shape and dqkv.data_ptr() == written["fs2hip_attention_bwd"]


def test_refusals(H):
    B, T, Hh = 1, 8, 1
    lens = torch.tensor([8], dtype=torch.int32).cuda()
    qkv = torch.randn(B * T, 3 * 257).cuda()
    with pytest.raises(ValueError, match="head dimension"):
        H.attention_fwd(qkv, lens, B, T, Hh)
    o = torch.randn(B, T, 257).cuda()
    lse = torch.randn(B, Hh, T).cuda()
    with pytest.raises(ValueError, match="head dimension"):
        H.attention_bwd(qkv, lens, o, o, lse, B, T, Hh)
    assert H.attention_padded_dim(257) == 0
    # the bf16-storage kernels keep their contract: head dim 128 only
    assert not H.attention_b_supported(64) and not H.attention_b_supported(96)
    qkv_b = torch.randn(B * T, 3 * 2 * 96).cuda().bfloat16()
    with pytest.raises(ValueError, match="head dimension"):
        H.attention_fwd_b(qkv_b, lens, B, T, 2)
    # the argument contract of the library's own entry points (include/fs2hip.h): each of these returns before any launch
    L, EINVAL, Tp = H.lib(), -22, 32

    held = []

    def buf(n, dtype=torch.float32):
        held.append(torch.zeros(n, dtype=dtype, device="cuda"))
        return held[-1].data_ptr()

    lens_p, lse_p, aux, sc, ds = lens.data_ptr(), lse.data_ptr(), buf(2 * T + 4), buf(T * Tp), buf(T * Tp)
    qkv_p, o_p, dqkv_p = buf(T * 3 * 64), buf(T * 64), buf(T * 3 * 64)
    # kept scores with bf16 operands
    assert L.fs2hip_attention_fwd(qkv_p, lens_p, o_p, lse_p, sc, T * Tp, B, T, Hh, 64, 0.0, 0, None, 1, None) == EINVAL
    # scores for a backward that does not spill
    assert L.fs2hip_attention_bwd(qkv_p, lens_p, o_p, o_p, lse_p, sc, aux, None, 0, dqkv_p, B, T, Hh, 64, 0.0, 0, None, 0,
                                  None) == EINVAL
    # spilled dS at a width without it
    assert L.fs2hip_attention_bwd(qkv_p, lens_p, o_p, o_p, lse_p, None, aux, ds, T * Tp, dqkv_p, B, T, Hh, 16, 0.0, 0, None, 0,
                                  None) == EINVAL
    # a bf16 dS scratch one element short
    qkv_b, o_b, dqkv_b, ds_b = (buf(n, torch.bfloat16) for n in (T * 3 * 128, T * 128, T * 3 * 128, T * Tp))
    assert L.fs2hip_attention_bwd_b(qkv_b, lens_p, o_b, o_b, lse_p, aux, ds_b, T * Tp - 1, dqkv_b, B, T, Hh, 128, 0.0, 0, None,
                                    None) == EINVAL
