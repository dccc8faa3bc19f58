"""GPU: ``modules.StyleEncoder`` (``model.gst``: forward + backward of a built model) against the oracle's
``StyleEncoder`` in float64 with the same weights, training mode, loss = (style * d_style).sum().

The comparison spans six BatchNorm layers and up to five recurrent steps, so its bound is not a constant: the fp32 CPU
run of the SAME oracle is measured against the float64 run, per tensor, inside the test, and the kernels may be off by
4x that (another summation order in the MFMA GEMMs and split-K), never less than the 2e-5 of the kernel-unit tests.

Two gradients are zero in exact arithmetic and hold only fp32 noise: ``stl.mha.linear_k.bias`` (a key bias shifts all
scores of a query equally) and ``ref_enc.gru.weight_hh_l0`` when the GRU runs a single step from h0 = 0.  They are the
only tensors exempt from the relative comparison (the test asserts that) and must be below 1e-5 of the largest
gradient norm of the case instead."""
import pytest
import torch

from fastspeech2_lightning_amd import config as cfgmod
from fastspeech2_lightning_amd.config import Stats
from oracle import cases as C
from oracle import fs2_oracle as O

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 2e-5, 4.0
ZERO_ALWAYS, ZERO_ONE_STEP = "stl.mha.linear_k.bias", "ref_enc.gru.weight_hh_l0"
_BUILT = {}


def build(n_mels):
    """(model, gst.* state dict without the prefix) -- one model per mel width for the whole module; the test reloads
    the state dict (the BatchNorm running statistics move with every training forward)."""
    if n_mels not in _BUILT:
        from fastspeech2_lightning_amd.model import FastSpeech2
        config, _, _ = C.build("e2e_gst_multispeaker_train")
        if n_mels != config.preprocessing.audio.n_mels:
            dump = config.model_checkpoint_dump()
            dump["preprocessing"]["audio"]["n_mels"] = n_mels
            config = cfgmod.FastSpeech2Config(**dump)
        model = FastSpeech2(config, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID)
        oracle = O.FastSpeech2Oracle(config, Stats(**C.STATS), n_symbols=C.N_SYMBOLS, n_speakers=len(C.SPEAKER2ID),
                                     n_langs=len(C.LANG2ID))
        _BUILT[n_mels] = model, O.seeded_state_dict(oracle.state_dict())
    return _BUILT[n_mels]


def run_oracle(sd_gst, n_mels, mel, d_style, dtype):
    enc = O.StyleEncoder(idim=n_mels)
    enc.load_state_dict(sd_gst)
    enc = enc.to(dtype).train()
    style = enc(mel.to(dtype))
    (style * d_style.to(dtype)).sum().backward()
    grads = {k: p.grad.detach() for k, p in enc.named_parameters()}
    stats = {k: v.detach() for k, v in enc.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return style.detach(), stats, grads


def max_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def l2_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def gru_steps(T):
    for _ in range(6):
        T = (T - 1) // 2 + 1
    return T


@pytest.mark.parametrize("B,T,n_mels", [(1, 20, 80), (2, 64, 80), (2, 65, 80), (3, 257, 80), (50, 130, 80),
                                         (2, 130, 65), (2, 130, 128)])
def test_style_encoder_matches_float64_oracle(B, T, n_mels):
    from fastspeech2_lightning_amd import hip as H
    model, sd = build(n_mels)
    model.load_state_dict(sd)
    model.train()
    sd_gst = {k[len("gst."):]: v for k, v in sd.items() if k.startswith("gst.")}
    g = torch.Generator().manual_seed(1000 * B + T + n_mels)
    mel = torch.randn(B, T, n_mels, generator=g)
    d_style = torch.randn(B, 256, generator=g)
    style64, stats64, grads64 = run_oracle(sd_gst, n_mels, mel, d_style, torch.float64)
    style32, stats32, grads32 = run_oracle(sd_gst, n_mels, mel, d_style, torch.float32)

    model.store.grad.zero_()
    try:
        style, ctx = model.gst.fwd(mel.cuda())
        model.gst.bwd(d_style.cuda(), ctx)
        H.flush_grad_reductions()
    finally:
        H.drop_pending_reductions()
    torch.cuda.synchronize()
    assert len(ctx.gates) == gru_steps(T)
    after = model.state_dict()
    grads = {k[len("gst."):]: v for k, v in model.store.grad_state_dict().items() if k.startswith("gst.")}
    assert set(grads) == set(grads64)

    report, failed = [], []

    def check(name, got, want, ref32, err):
        e, e32 = err(got, want), err(ref32, want)
        bound = max(FLOOR, FACTOR * e32)
        report.append(f"{name}: kernel {e:.2e}, fp32 oracle {e32:.2e}, bound {bound:.2e}")
        if not (e < bound):
            failed.append(name)

    check("style", style, style64, style32, max_err)
    assert len(stats64) == 12
    for k in stats64:
        check(k, after["gst." + k], stats64[k], stats32[k], max_err)
    norms = {k: float(v.norm()) for k, v in grads64.items()}
    top = max(norms.values())
    exempt = {k for k, n in norms.items() if n < 1e-6 * top}
    assert exempt == ({ZERO_ALWAYS, ZERO_ONE_STEP} if gru_steps(T) == 1 else {ZERO_ALWAYS}), exempt
    for k in grads64:
        if k in exempt:
            n = float(grads[k].double().norm())
            report.append(f"{k}: zero in exact arithmetic, kernel norm {n:.2e} = {n / top:.2e} of the largest, "
                          f"fp32 oracle {float(grads32[k].norm()) / top:.2e}")
            if not (n < 1e-5 * top):
                failed.append(k)
        else:
            check(k, grads[k], grads64[k], grads32[k], l2_err)
    print(f"\nGST B={B} T={T} n_mels={n_mels} ({gru_steps(T)} GRU steps):\n  " + "\n  ".join(report))
    assert not failed, (failed, report)
