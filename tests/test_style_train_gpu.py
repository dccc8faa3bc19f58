"""GPU: length-aware TRAINING of the GST style encoder -- ``hip.gru_fwd_states`` / ``hip.gru_bwd_states``,
``hip.bn_stats_lens`` / ``hip.bn_act_bwd_lens``, ``StyleEncoder.fwd_train`` + ``bwd``, ``FastSpeech2.style_lengths`` and
``fs2l train --style-lengths``.

The yardstick is ``tests/style_train_references.py``: a float64 restatement of the definition in plain torch with autograd,
on the oracle's parameters.  Bounds are those of ``tests/test_style_lens_gpu.py``: the error relative to the largest element
(the l2 error for a gradient tensor of the module, as ``tests/test_gst_module_gpu.py`` takes it) stays below ``max(2e-5, 4 x
the fp32 CPU restatement's own error against float64)``, measured inside the test and printed; whole-model values to
``1e-4 * max(1, |ref|.max())`` (``tests/test_exact_lengths_gpu.py``)."""
import json

import pytest
import torch

from fastspeech2_lightning_amd.config import Stats
from oracle import cases as C
from oracle import fs2_oracle as O
from tests.gst_references import gru_step_ref
from tests.style_train_references import LengthAwareStyle, masked_batchnorm, style_lens_ref
from tests.test_style_lens_gpu import FACTOR, FLOOR, GRU_CASES, REF_FRAMES, U, _gru_inputs, _poisoned, _rel

pytestmark = pytest.mark.gpu

_SHARED = {}


def _check(report, failed, name, got, want, ref32, err=_rel):
    e, e32 = err(got, want), err(ref32, want)
    bound = max(FLOOR, FACTOR * e32)
    report.append(f"{name}: kernel {e:.2e}, fp32 restatement {e32:.2e}, bound {bound:.2e}")
    if not (e < bound):
        failed.append(name)


def _l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


# ---- 1. the GRU pair ---------------------------------------------------------------------------------------------------
def _gru_train_ref(gi, w_hh, b_hh, steps, dh_last, dtype):
    """Row by row: the recurrence over the row's first ``min(steps[b], T)`` projections with autograd.  Returns h_last,
    hs [B, T + 1, U], gates [B, T, 4U], dgi [B, T, 3U], dgh [B, T, 3U] (the gradient of ``w_hh h + b_hh``), dh0 [B, U];
    rows beyond a row's steps are zero."""
    B, T, _ = gi.shape
    w, bias = w_hh.to(dtype), b_hh.to(dtype)
    h_last, hs, gates = torch.zeros(B, U, dtype=dtype), torch.zeros(B, T + 1, U, dtype=dtype), torch.zeros(B, T, 4 * U, dtype=dtype)
    dgi, dgh, dh0 = torch.zeros(B, T, 3 * U, dtype=dtype), torch.zeros(B, T, 3 * U, dtype=dtype), torch.zeros(B, U, dtype=dtype)
    for b in range(B):
        n = min(max(int(steps[b]), 0), T)
        x = gi[b:b + 1, :n].to(dtype).clone().requires_grad_(True)
        probe = torch.zeros(1, n, 3 * U, dtype=dtype, requires_grad=True)
        h0 = torch.zeros(1, U, dtype=dtype, requires_grad=True)
        h = h0
        for t in range(n):
            h, (r, z, c, hn) = gru_step_ref(x[:, t], h @ w.t() + bias + probe[:, t], h)
            hs[b, t + 1] = h.detach()[0]
            gates[b, t] = torch.cat([r, z, c, hn], dim=1).detach()[0]
        h_last[b] = h.detach()[0]
        (h * dh_last[b:b + 1].to(dtype)).sum().backward()
        dh0[b] = h0.grad[0]
        if n:
            dgi[b, :n], dgh[b, :n] = x.grad[0], probe.grad[0]
    return h_last, hs, gates, dgi, dgh, dh0


@pytest.mark.parametrize("name", list(GRU_CASES))
def test_gru_states_pair_matches_the_float64_recurrence_and_its_gradient(name):
    from fastspeech2_lightning_amd import hip as H
    B, T, steps = GRU_CASES[name]
    gi, w_hh, b_hh = _gru_inputs(B, T, 100 + B)
    if steps is None:
        steps = torch.randint(0, T + 1, (B,), generator=torch.Generator().manual_seed(3)).tolist()
        assert {0, T} <= set(steps)
    dh_last = torch.randn(B, U, generator=torch.Generator().manual_seed(9))
    want = _gru_train_ref(gi, w_hh, b_hh, steps, dh_last, torch.float64)
    ref32 = _gru_train_ref(gi, w_hh, b_hh, steps, dh_last, torch.float32)
    dev_steps = torch.tensor(steps, dtype=torch.int32).cuda()
    poisoned = _poisoned(gi, steps).cuda()
    h, hs, gates = H.gru_fwd_states(poisoned, w_hh.cuda(), b_hh.cuda(), dev_steps)
    dgi, dgh, dh0 = H.gru_bwd_states(dh_last.cuda(), hs, gates, w_hh.cuda(), dev_steps)
    last = H.gru_last_state(poisoned, w_hh.cuda(), b_hh.cuda(), dev_steps)
    torch.cuda.synchronize()
    assert torch.equal(h, last)                      # the same recurrence in the same order
    assert tuple(hs.shape) == (B, T + 1, U) and tuple(gates.shape) == (B, T, 4 * U)
    assert tuple(dgi.shape) == (B, T, 3 * U) and tuple(dgh.shape) == (B, T + 1, 3 * U) and tuple(dh0.shape) == (B, U)
    got = (h, hs, gates, dgi, dgh[:, :T], dh0)
    report, failed = [], []
    for tag, g, w64, w32 in zip(("h_last", "hs", "gates", "dgi", "dgh", "dh0"), got, want, ref32):
        assert torch.isfinite(g).all(), tag      # (finite: the NaN rows of gi were not read)
        _check(report, failed, tag, g, w64, w32)
    print(f"\nGRU pair {name}:\n  " + "\n  ".join(report))
    assert not failed, (failed, report)
    for b, n in enumerate(steps):
        n = min(max(n, 0), T)
        assert int((dgi[b, n:] != 0).sum()) == 0 and int((dgh[b, n:] != 0).sum()) == 0, (b, "gradient rows beyond the steps")
        assert int((hs[b, n + 1:] != 0).sum()) == 0 and int((hs[b, 0] != 0).sum()) == 0, (b, "state rows beyond the steps")
        assert torch.equal(hs[b, n], h[b])
        if n == 0:
            assert torch.equal(dh0[b], dh_last[b].cuda())
    if name == "ragged":
        for b in range(B):   # a row's outputs are a function of that row alone: bit-equal as a batch of one
            one_steps = dev_steps[b:b + 1].contiguous()
            h1, hs1, g1 = H.gru_fwd_states(poisoned[b:b + 1].contiguous(), w_hh.cuda(), b_hh.cuda(), one_steps)
            one = H.gru_bwd_states(dh_last[b:b + 1].cuda(), hs1, g1, w_hh.cuda(), one_steps)
            assert torch.equal(h1[0], h[b]) and torch.equal(hs1[0], hs[b]) and torch.equal(g1[0], gates[b]), b
            for a, full in zip(one, (dgi, dgh, dh0)):
                assert torch.equal(a[0], full[b]), b


def test_gru_states_pair_refusals():
    from fastspeech2_lightning_amd import hip as H
    gi, w_hh, b_hh = (t.cuda() for t in _gru_inputs(2, 3, 1))
    steps = torch.tensor([1, 2], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="only 128"):
        H.gru_fwd_states(torch.zeros(2, 3, 192).cuda(), torch.zeros(192, 64).cuda(), torch.zeros(192).cuda(), steps)
    with pytest.raises(ValueError, match="do not fit"):
        H.gru_fwd_states(gi, w_hh, b_hh[:-1].contiguous(), steps)
    with pytest.raises(ValueError, match="entries"):
        H.gru_fwd_states(gi, w_hh, b_hh, steps[:1].contiguous())
    with pytest.raises(ValueError, match=r"\[B, T, 3U\]"):
        H.gru_fwd_states(gi.view(6, 3 * U), w_hh, b_hh, steps)
    with pytest.raises(TypeError):
        H.gru_fwd_states(gi, w_hh, b_hh, steps.long())
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.gru_fwd_states(gi.cpu(), w_hh, b_hh, steps)
    h, hs, gates = H.gru_fwd_states(gi, w_hh, b_hh, steps)
    dh = torch.zeros(2, U).cuda()
    with pytest.raises(ValueError, match="only 128"):
        H.gru_bwd_states(dh, hs, gates, torch.zeros(192, 64).cuda(), steps)
    with pytest.raises(ValueError, match="do not fit"):
        H.gru_bwd_states(dh, hs[:, :-1].contiguous(), gates, w_hh, steps)
    with pytest.raises(ValueError, match="do not fit"):
        H.gru_bwd_states(dh[:1].contiguous(), hs, gates, w_hh, steps)
    with pytest.raises(ValueError, match="entries"):
        H.gru_bwd_states(dh, hs, gates, w_hh, steps[:1].contiguous())
    with pytest.raises(TypeError):
        H.gru_bwd_states(dh, hs, gates, w_hh, steps.long())
    # the entry points themselves: null pointers, non-positive extents and U != 128 are FS2HIP_EINVAL before any launch
    lib, p = H.real_lib(), (lambda t: t.data_ptr())
    ok_f = (p(gi), p(w_hh), p(b_hh), p(steps), p(hs), p(gates), p(h))
    assert lib.fs2hip_gru_fwd_states(*ok_f, 2, 3, 64, None) == -22
    assert lib.fs2hip_gru_fwd_states(*ok_f, 0, 3, 128, None) == -22 and lib.fs2hip_gru_fwd_states(*ok_f, 2, 0, 128, None) == -22
    for i in range(len(ok_f)):
        assert lib.fs2hip_gru_fwd_states(*ok_f[:i], None, *ok_f[i + 1:], 2, 3, 128, None) == -22, i
    dgi, dgh, dh0 = H.gru_bwd_states(dh, hs, gates, w_hh, steps)
    ok_b = (p(dh), p(hs), p(gates), p(w_hh), p(steps), p(dgi), p(dgh), p(dh0))
    assert lib.fs2hip_gru_bwd_states(*ok_b, 2, 3, 64, None) == -22 and lib.fs2hip_gru_bwd_states(*ok_b, 2, -1, 128, None) == -22
    for i in range(len(ok_b)):
        assert lib.fs2hip_gru_bwd_states(*ok_b[:i], None, *ok_b[i + 1:], 2, 3, 128, None) == -22, i
    torch.cuda.synchronize()


# ---- 2. masked BatchNorm statistics, 3. their backward -----------------------------------------------------------------
#: name -> (B, H, W, C, lens, channel with mean 1e3 and std 1 or None)
BN_CASES = {
    "small": (3, 5, 2, 32, [5, 0, 3], 7),
    "wide": (3, 5, 2, 128, [5, 0, 3], None),
    "several_parts": (2, 3000, 2, 32, [3000, 1], 3),      # stripes of 32 rows: the first utterance spans 188 of them
    "above_the_few_row_form": (3, 9, 2, 32, [9, 0, 4], None),   # 26 valid rows: the general backward (the first two: 16)
    "clamped": (2, 4, 2, 32, [9, -3], None),
}


def _bn_inputs(name):
    B, Hh, Ww, Cc, lens, big = BN_CASES[name]
    g = torch.Generator().manual_seed(Hh * Cc + B)
    y = torch.randn(B, Hh, Ww, Cc, generator=g)
    if big is not None:
        y[..., big] += 1e3
    gamma, beta = 1 + 0.3 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    rmean, rvar = torch.randn(Cc, generator=g), 1 + torch.rand(Cc, generator=g)
    dout = torch.randn(B, Hh, Ww, Cc, generator=g)
    return y, gamma, beta, rmean, rvar, dout


def _tail_poisoned(t, lens):
    t = t.clone()
    for b, n in enumerate(lens):
        t[b, max(min(n, t.shape[1]), 0):] = float("nan")
    return t


def _bn_ref(name, dtype):
    """The restatement's masked BatchNorm + ReLU on the case (channels first, as the oracle's module), with autograd:
    (mean, var, running_mean, running_var, dgamma, dbeta, dy [B, H, W, C])."""
    B, Hh, Ww, Cc, lens, _ = BN_CASES[name]
    y, gamma, beta, rmean, rvar, dout = (t.to(dtype) for t in _bn_inputs(name))
    bn = torch.nn.BatchNorm2d(Cc).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rmean); bn.running_var.copy_(rvar)
    # (the values beyond the lengths as they are: the restatement masks them, and autograd would turn NaN * 0 into NaN)
    raw = y.permute(0, 3, 1, 2).contiguous().requires_grad_(True)     # [B, C, H, W]
    out = torch.relu(masked_batchnorm(raw, lens, bn, True))
    L = [min(max(n, 0), Hh) for n in lens]
    keep = torch.zeros(B, 1, Hh, 1, dtype=torch.bool)
    for b, n in enumerate(L):
        keep[b, :, :n] = True
    torch.where(keep, out * dout.permute(0, 3, 1, 2), torch.zeros_like(out)).sum().backward()
    kept = torch.cat([y[b, :n].reshape(-1, Cc) for b, n in enumerate(L)])
    mean, var = kept.mean(0), kept.var(0, unbiased=False)
    dy = torch.where(keep, raw.grad, torch.zeros_like(raw.grad)).permute(0, 2, 3, 1)
    return mean, var, bn.running_mean.detach(), bn.running_var.detach(), bn.weight.grad, bn.bias.grad, dy


@pytest.mark.parametrize("name", list(BN_CASES))
def test_masked_batchnorm_statistics_and_backward_match_float64(name):
    from fastspeech2_lightning_amd import hip as H
    B, Hh, Ww, Cc, lens, big = BN_CASES[name]
    y, gamma, beta, rmean, rvar, dout = _bn_inputs(name)
    want, ref32 = _bn_ref(name, torch.float64), _bn_ref(name, torch.float32)
    dev_lens = torch.tensor(lens, dtype=torch.int32).cuda()
    raw = _tail_poisoned(y, lens).cuda()
    rm, rv = rmean.cuda(), rvar.cuda()
    stats = H.bn_stats_lens(raw, dev_lens, gamma.cuda(), beta.cuda(), rm, rv)
    dgamma, dbeta = torch.empty(Cc).cuda(), torch.empty(Cc).cuda()
    dy = H.bn_act_bwd_lens(_tail_poisoned(dout, lens).cuda(), raw, stats, dev_lens, dgamma, dbeta, "relu")
    again = H.bn_stats_lens(raw, dev_lens, gamma.cuda(), beta.cuda())
    torch.cuda.synchronize()
    assert torch.equal(again, stats)                 # deterministic, and the running buffers are optional
    for t in (stats, rm, rv, dgamma, dbeta, dy):
        assert torch.isfinite(t).all()               # (finite: nothing beyond the lengths was read)
    eps = 1e-5
    var = 1.0 / stats[3].double() ** 2 - eps
    report, failed = [], []
    _check(report, failed, "mean", stats[2], want[0], ref32[0])
    _check(report, failed, "variance", var, want[1], ref32[1])
    _check(report, failed, "scale", stats[0], gamma.double() / torch.sqrt(want[1] + eps), gamma / torch.sqrt(ref32[1] + eps))
    _check(report, failed, "shift", stats[1], beta.double() - want[0] * gamma.double() / torch.sqrt(want[1] + eps),
           beta - ref32[0] * gamma / torch.sqrt(ref32[1] + eps))
    _check(report, failed, "running_mean", rm, want[2], ref32[2])
    _check(report, failed, "running_var", rv, want[3], ref32[3])
    if big is not None:   # |mean| >> std: the channel's own variance, relative to itself
        _check(report, failed, f"variance of channel {big} (mean 1e3)", var[big], want[1][big], ref32[1][big])
        assert 0.3 < float(want[1][big]) < 3.0
    _check(report, failed, "dgamma", dgamma, want[4], ref32[4])
    _check(report, failed, "dbeta", dbeta, want[5], ref32[5])
    _check(report, failed, "dy", dy, want[6], ref32[6])
    print(f"\nmasked BatchNorm {name} ({Ww * sum(min(max(n, 0), Hh) for n in lens)} valid rows):\n  " + "\n  ".join(report))
    assert not failed, (failed, report)
    for b, n in enumerate(lens):
        assert int((dy[b, max(min(n, Hh), 0):] != 0).sum()) == 0, (b, "rows of dy beyond the lengths are exactly 0")


@pytest.mark.parametrize("name", ["small", "several_parts"])
def test_masked_statistics_with_full_lengths_agree_with_colstats(name):
    from fastspeech2_lightning_amd import hip as H
    B, Hh, Ww, Cc, _, _ = BN_CASES[name]
    y, gamma, beta, rmean, rvar, _ = _bn_inputs(name)
    raw = y.cuda()
    rm0, rv0, rm1, rv1 = rmean.cuda(), rvar.cuda(), rmean.cuda(), rvar.cuda()
    plain = H.bn_finalize(H.colstats(raw.view(-1, Cc)), gamma.cuda(), beta.cuda(), rm0, rv0)
    full = torch.full((B,), Hh, dtype=torch.int32).cuda()
    masked = H.bn_stats_lens(raw, full, gamma.cuda(), beta.cuda(), rm1, rv1)
    for tag, a, b in (("stats", masked[:4], plain[:4]), ("running_mean", rm1, rm0), ("running_var", rv1, rv0)):
        e = _rel(a, b)
        print(f"{name}: {tag} with full lengths against colstats + bn_finalize {e:.2e}")
        assert e < FLOOR, (tag, e)


def test_masked_batchnorm_refusals():
    from fastspeech2_lightning_amd import hip as H
    y, gamma, beta, rmean, rvar, dout = (t.cuda() for t in _bn_inputs("small"))
    lens = torch.tensor([5, 0, 3], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        H.bn_stats_lens(y.view(30, 32), lens, gamma, beta)
    with pytest.raises(ValueError, match="entries"):
        H.bn_stats_lens(y, lens[:2].contiguous(), gamma, beta)
    with pytest.raises(ValueError, match="both running buffers"):
        H.bn_stats_lens(y, lens, gamma, beta, rmean, None)
    with pytest.raises(TypeError):
        H.bn_stats_lens(y, lens.long(), gamma, beta)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.bn_stats_lens(y.cpu(), lens, gamma, beta)
    stats = H.bn_stats_lens(y, lens, gamma, beta)
    with pytest.raises(ValueError, match="shape mismatch"):
        H.bn_act_bwd_lens(dout[:2].contiguous(), y, stats, lens, torch.empty(32).cuda(), torch.empty(32).cuda(), "relu")
    lib, p = H.real_lib(), (lambda t: t.data_ptr())
    ws = torch.empty(4096).cuda()
    ok = (p(y), p(lens), p(ws), p(gamma), p(beta), None, None, 0.1, 1e-5, p(stats))
    assert lib.fs2hip_bn_stats_lens(*ok, 3, 5, 2, 32, None) == 0
    assert lib.fs2hip_bn_stats_lens(*ok, 0, 5, 2, 32, None) == -22 and lib.fs2hip_bn_stats_lens(*ok, 3, 5, 0, 32, None) == -22
    assert lib.fs2hip_bn_stats_lens(*ok, 3, 5, 2, 0, None) == -22
    for i in (0, 1, 2, 3, 4, 9):
        assert lib.fs2hip_bn_stats_lens(*ok[:i], None, *ok[i + 1:], 3, 5, 2, 32, None) == -22, i
    dy, dg, db = torch.empty_like(y), torch.empty(32).cuda(), torch.empty(32).cuda()
    ok = (p(dout), p(y), p(stats), p(lens), p(ws), p(ws) + 8192, p(dg), p(db), p(dy))
    assert lib.fs2hip_bn_act_bwd_lens(*ok, 3, 5, 2, 32, 1, None) == 0
    assert lib.fs2hip_bn_act_bwd_lens(*ok, 3, 0, 2, 32, 1, None) == -22
    for i in range(len(ok)):
        assert lib.fs2hip_bn_act_bwd_lens(*ok[:i], None, *ok[i + 1:], 3, 5, 2, 32, 1, None) == -22, i
    assert lib.fs2hip_bn_lens_parts(0, 5, 2) == 0 and lib.fs2hip_bn_lens_parts(3, 5, 2) == 3
    torch.cuda.synchronize()


# ---- 4. module ---------------------------------------------------------------------------------------------------------
def _padded(refs, T):
    mel = torch.zeros(len(refs), T, refs[0].shape[1])
    for b, r in enumerate(refs):
        mel[b, :len(r)] = r
    return mel


def _restatement(sd_gst, mel, lens, d_style, dtype):
    enc = O.StyleEncoder(idim=mel.shape[-1])
    enc.load_state_dict(sd_gst)
    enc = enc.to(dtype).train()
    style = style_lens_ref(enc, mel.to(dtype), lens)
    (style * d_style.to(dtype)).sum().backward()
    grads = {k: p.grad.detach() for k, p in enc.named_parameters()}
    stats = {k: v.detach() for k, v in enc.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return style.detach(), stats, grads


def _module_case():
    """The model, the references, their two paddings and the restatement's runs at 257 frames: computed once, shared."""
    if "module" not in _SHARED:
        from tests.test_gst_module_gpu import build
        model, sd = build(80)
        sd_gst = {k[len("gst."):]: v for k, v in sd.items() if k.startswith("gst.")}
        g = torch.Generator().manual_seed(7)
        refs = [torch.randn(n, 80, generator=g) for n in REF_FRAMES]
        d_style = torch.randn(len(refs), 256, generator=g)
        mel = _padded(refs, 257)
        runs = {dt: _restatement(sd_gst, mel, REF_FRAMES, d_style, dt) for dt in (torch.float64, torch.float32)}
        _SHARED["module"] = model, sd, sd_gst, refs, d_style, runs
    return _SHARED["module"]


def _run_module(model, sd, mel, d_style, lens=None):
    """One training forward + backward of ``model.gst`` from the state ``sd``: (style, running buffers, gst.* gradients)."""
    from fastspeech2_lightning_amd import hip as H
    model.load_state_dict(sd)
    model.train()
    model.store.grad.zero_()
    try:
        if lens is None:
            style, ctx = model.gst.fwd(mel.cuda())
        else:
            style, ctx = model.gst.fwd_train(mel.cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
        model.gst.bwd(d_style.cuda(), ctx)
        H.flush_grad_reductions()
    finally:
        H.drop_pending_reductions()
        model.eval()
    torch.cuda.synchronize()
    after = model.state_dict()
    stats = {k[len("gst."):]: v.clone() for k, v in after.items() if k.startswith("gst.") and k.endswith(("running_mean", "running_var"))}
    grads = {k[len("gst."):]: v.clone() for k, v in model.store.grad_state_dict().items() if k.startswith("gst.")}
    return style.clone(), stats, grads


def _compare_runs(tag, got, want, ref32):
    """style and running buffers by the largest element, gradients by their l2 norm; the key bias's gradient is zero in
    exact arithmetic (tests/test_gst_module_gpu.py) and is held below 1e-5 of the largest gradient norm instead."""
    from tests.test_gst_module_gpu import ZERO_ALWAYS
    report, failed = [], []
    _check(report, failed, "style", got[0], want[0], ref32[0])
    assert len(want[1]) == 12 and set(got[1]) == set(want[1])
    for k in want[1]:
        _check(report, failed, k, got[1][k], want[1][k], ref32[1][k])
    assert set(got[2]) == set(want[2])
    top = max(float(v.norm()) for v in want[2].values())
    for k in want[2]:
        if k == ZERO_ALWAYS:
            n = float(got[2][k].double().norm())
            report.append(f"{k}: zero in exact arithmetic, kernel norm {n / top:.2e} of the largest")
            if not (n < 1e-5 * top):
                failed.append(k)
        else:
            _check(report, failed, k, got[2][k], want[2][k], ref32[2][k], _l2)
    print(f"\n{tag}:\n  " + "\n  ".join(report))
    assert not failed, (failed, report)


def test_fwd_train_and_bwd_match_the_float64_restatement():
    model, sd, sd_gst, refs, d_style, runs = _module_case()
    got = _run_module(model, sd, _padded(refs, 257), d_style, REF_FRAMES)
    assert tuple(got[0].shape) == (len(REF_FRAMES), 256)
    _compare_runs("fwd_train + bwd, references padded to 257 frames", got, runs[torch.float64], runs[torch.float32])


def test_fwd_train_does_not_depend_on_the_padded_length_and_todays_training_path_does():
    model, sd, sd_gst, refs, d_style, runs = _module_case()
    # the discriminating half: today's train-mode path reads the padding -- in the float64 oracle and on the GPU, padding
    # the same references to 300 frames instead of 257 moves every row's style (BatchNorm's batch statistics count the
    # padded rows, so the longest reference moves too)
    plain = {}
    for T in (257, 300):
        enc = O.StyleEncoder(idim=80)
        enc.load_state_dict(sd_gst)
        with torch.no_grad():
            plain[T] = (enc.double().train()(_padded(refs, T).double()), _run_module(model, sd, _padded(refs, T), d_style)[0].cpu())
    for b in range(len(refs)):
        dev64 = float((plain[300][0][b] - plain[257][0][b]).abs().max())
        dev = float((plain[300][1][b] - plain[257][1][b]).abs().max())
        print(f"reference {b} ({REF_FRAMES[b]} frames): today's path, 300 against 257 frames of padding: oracle {dev64:.2e}, "
              f"GPU {dev:.2e}, largest element {float(plain[257][0][b].abs().max()):.2f}")
        assert dev64 > 1e-3 and dev > 1e-3, (b, dev64, dev)
    got = _run_module(model, sd, _padded(refs, 300), d_style, REF_FRAMES)
    _compare_runs("fwd_train + bwd, the same references padded to 300 frames, against the restatement at 257", got,
                  runs[torch.float64], runs[torch.float32])


def test_fwd_train_with_full_lengths_agrees_with_todays_training_path():
    from tests.test_gst_module_gpu import run_oracle
    model, sd, sd_gst, refs, d_style, _ = _module_case()
    mel = torch.randn(len(refs), 257, 80, generator=torch.Generator().manual_seed(8))
    want = run_oracle(sd_gst, 80, mel, d_style, torch.float64)
    ref32 = run_oracle(sd_gst, 80, mel, d_style, torch.float32)
    today = _run_module(model, sd, mel, d_style)
    full = _run_module(model, sd, mel, d_style, [257] * len(refs))
    # both against the float64 oracle (which has no padding to read here), then one against the other with the fp32
    # oracle's error as the measure
    _compare_runs("all lengths = 257: fwd_train + bwd against the float64 oracle", full, want, ref32)
    report, failed = [], []
    pairs = [("style", full[0], today[0], want[0], ref32[0], _rel)]
    pairs += [(k, full[1][k], today[1][k], want[1][k], ref32[1][k], _rel) for k in want[1]]
    from tests.test_gst_module_gpu import ZERO_ALWAYS
    pairs += [(k, full[2][k], today[2][k], want[2][k], ref32[2][k], _l2) for k in want[2] if k != ZERO_ALWAYS]
    for k, a, b, w64, w32, err in pairs:
        e, bound = err(a, b), max(FLOOR, FACTOR * err(w32, w64))
        report.append(f"{k}: fwd_train against fwd {e:.2e}, bound {bound:.2e}")
        if not (e < bound):
            failed.append(k)
    print("\nall lengths = 257, the two GPU paths:\n  " + "\n  ".join(report))
    assert not failed, (failed, report)


def test_fwd_train_refusals_and_the_pinned_ones():
    model, sd, sd_gst, refs, d_style, _ = _module_case()
    model.load_state_dict(sd)
    lens = torch.tensor(REF_FRAMES, dtype=torch.int32).cuda()
    model.eval()
    with pytest.raises(ValueError, match="train mode"):
        model.gst.fwd_train(_padded(refs, 257).cuda(), lens)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):      # (pinned by tests/test_style_lens_gpu.py: stays)
            model.gst.fwd(_padded(refs, 257).cuda(), lens)
        kept = _padded(refs, 257).cuda()
        kept[0, REF_FRAMES[0]:] = 3.0
        given = kept.clone()
        model.gst.fwd_train(given, lens)
        assert torch.equal(given, kept)                          # the caller's mel is not written to
    finally:
        model.eval()


# ---- 5. model ----------------------------------------------------------------------------------------------------------
def _fresh_pair():
    from tests.test_exact_lengths_gpu import _pair
    cfg, batch, _ = C.build("e2e_gst_multispeaker_train")
    model, oracle = _pair(cfg)
    oracle = oracle.double()
    oracle.gst = LengthAwareStyle(oracle.gst)
    model.postnet.dropout_p = oracle.postnet.dropout_p = 0.0
    return cfg, model, oracle, batch


def _double(batch):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}


def test_style_lengths_training_step_and_validation_forward_match_the_restated_oracle():
    cfg, model, oracle, batch = _fresh_pair()
    assert len(set(batch["mel_lens"].tolist())) > 1
    model.style_lengths = True
    assert model.style_lengths is True
    oracle.gst.lens = batch["mel_lens"].tolist()
    # a teacher-forced eval forward (validation): the running statistics, every row over its own frames
    kept = batch["mel"].clone()
    with torch.no_grad():
        ref = oracle.eval()(_double(batch))
    out = model.eval()(dict(batch))
    assert torch.equal(batch["mel"], kept)
    for key in ("output", "postnet_output"):
        err, tol = float((out[key].cpu().double() - ref[key]).abs().max()), 1e-4 * max(1.0, float(ref[key].abs().max()))
        print(f"validation forward: {key} error {err:.2e}, bound {tol:.2e}")
        assert err < tol, (key, err, tol)
    # ... which the default (flag off) does not give: the padding moves the style, far above fp32 rounding
    model.style_lengths = False
    off = model(dict(batch))
    model.style_lengths = True
    moved = float((off["output"] - out["output"]).abs().max())
    print(f"validation forward: flag off against on {moved:.2e}")
    assert moved > 1e-4
    # a training step: loss terms and the flat gradient
    oracle.train()
    model.train()
    ref = oracle(_double(batch))
    ref_losses = oracle.loss(ref, _double(batch), 0)
    ref_losses["total"].backward()
    model.training_step(dict(batch))
    got_losses = model.losses_to_host()
    assert set(got_losses) == set(ref_losses)
    for k, v in ref_losses.items():
        v = float(v.detach())
        print(f"loss {k}: {got_losses[k]:.8f} against {v:.8f}")
        assert abs(got_losses[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got_losses[k], v)
    got = model.store.grad_state_dict()
    names = [k for k, p in oracle.named_parameters() if p.grad is not None]
    assert any(k.startswith("gst.ref_enc.convs.0") for k in names) and all(k in got for k in names)
    want_flat = torch.cat([dict(oracle.named_parameters())[k].grad.reshape(-1) for k in names])
    got_flat = torch.cat([got[k].cpu().double().reshape(-1) for k in names])
    err, tol = float((got_flat - want_flat).abs().max()), 1e-4 * max(1.0, float(want_flat.abs().max()))
    gst_err = max(float((got[k].cpu().double() - dict(oracle.named_parameters())[k].grad).abs().max()) for k in names
                  if k.startswith("gst."))
    print(f"flat gradient ({want_flat.numel()} elements, largest {float(want_flat.abs().max()):.3e}): error {err:.2e} "
          f"(gst.* {gst_err:.2e}), bound {tol:.2e}")
    assert err < tol, (err, tol)
    model.eval()


def _geometry_batches():
    """Three ragged batches of one bucket geometry with different mel_lens."""
    from fastspeech2_lightning_amd.synthetic import synthetic_batch
    out = []
    for seed in (15, 16, 17):
        b = synthetic_batch(seed=seed, B=3, ts_lo=6, ts_hi=12, n_symbols=C.N_SYMBOLS, n_mels=80, dur_hi=9)
        b["speaker_id"] = torch.arange(3, dtype=torch.int32) % len(C.SPEAKER2ID)
        b["language_id"] = torch.arange(3, dtype=torch.int32) % len(C.LANG2ID)
        out.append(b)
    Ts_b, Tm_b = max(b["text"].shape[1] for b in out), max(b["mel"].shape[1] for b in out) + 5
    assert len({tuple(b["mel_lens"].tolist()) for b in out}) == 3
    return [dict(b, bucket_geometry=(Ts_b, Tm_b)) for b in out]


def test_replayed_steps_read_the_lengths_of_the_batch_they_are_fed():
    from fastspeech2_lightning_amd.model import FastSpeech2
    cfg, _, _ = C.build("e2e_gst_multispeaker_train")
    batches = _geometry_batches()
    runs = {}
    for planned in (True, False):
        model = FastSpeech2(cfg, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID, seed=3)
        model.style_lengths = True
        model.plan_enabled = planned
        model.train()
        steps = []
        for b in batches + batches[:1]:       # eager, recorded, replayed, replayed
            model.training_step(dict(b))
            torch.cuda.synchronize()
            steps.append((model.losses_to_host(), model.store.grad.clone(), dict(model.plans.counters())))
        runs[planned] = steps
        model.eval()
    counters = [s[2] for s in runs[True]]
    print("plan counters per step:", counters)
    assert [c["plans_replayed"] for c in counters] == [0, 0, 1, 2] and counters[-1]["plans_recorded"] == 1
    assert runs[False][-1][2]["plans_replayed"] == 0
    for i, (a, b) in enumerate(zip(runs[True], runs[False])):
        assert a[0] == b[0], (i, a[0], b[0])
        assert torch.equal(a[1], b[1]), (i, "flat gradient")
    # (the steps differ from one another: the lengths are read, not baked in)
    assert not torch.equal(runs[True][2][1], runs[True][1][1])


def test_style_lengths_needs_the_style_encoder():
    from tests.test_exact_lengths_gpu import _pair
    plain, _ = _pair(C.small_config(learn_alignment=False))
    assert plain.style_lengths is False
    with pytest.raises(ValueError, match="global style token"):
        plain.style_lengths = True
    plain.style_lengths = False


def test_style_reference_lens_outside_inference_is_still_refused():
    cfg, model, oracle, batch = _fresh_pair()
    model.style_lengths = True
    with pytest.raises(ValueError, match="inference=True"):     # (pinned by tests/test_style_lens_gpu.py: stays)
        model(dict(batch, mel_style_reference=batch["mel"], style_reference_lens=batch["mel_lens"]))


def test_bf16_mixed_training_step_with_style_lengths_is_finite():
    """A smoke test only: the project holds no bf16 bound for this path."""
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.model import FastSpeech2
    cfg, batch, _ = C.build("e2e_gst_multispeaker_train")
    try:
        model = FastSpeech2(cfg, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID, precision="bf16-mixed")
        model.style_lengths = True
        model.train()
        model.training_step(dict(batch))
        torch.cuda.synchronize()
        losses = model.losses_to_host()
        assert all(v == v and abs(v) != float("inf") for v in losses.values()), losses
        assert torch.isfinite(model.store.grad).all()
        model.eval()
    finally:
        hip.set_precision("32-true")


# ---- 6. command --------------------------------------------------------------------------------------------------------
def test_fs2l_train_with_style_lengths_and_buckets(tmp_path):
    import yaml

    from fastspeech2_lightning_amd import cli
    from tests.test_cli_cpu import make_project
    cfg = make_project(tmp_path, n_train=10, n_val=3, write_features=True, n_mels=80)
    conf = yaml.safe_load(cfg.read_text())
    wide = dict(layers=1, heads=2, input_dim=256, feedforward_dim=64, conv_kernel_size=9, dropout=0.1)
    vp = dict(n_layers=1, kernel_size=3, dropout=0.1, input_dim=256, n_bins=16)
    conf["model"].update(encoder=wide, decoder=wide, use_global_style_token_module=True,
                         variance_predictors=dict(energy=vp, pitch=vp, duration=vp))
    cfg.write_text(yaml.safe_dump(conf))
    out = tmp_path / "run"
    assert cli.main(["train", str(cfg), "--output-dir", str(out), "--log-every", "1", "--devices", "1", "--max-steps", "3",
                     "--style-lengths", "--bucket-lengths", "2"]) == 0
    recs = [json.loads(l) for l in (out / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "training/total_loss" in r]
    assert [r["step"] for r in train] == [1, 2, 3]
    for r in train:
        assert r["style_lengths"] is True
        assert all(v == v and abs(v) != float("inf") for k, v in r.items() if k.endswith("_loss")), r
