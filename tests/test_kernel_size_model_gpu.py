"""GPU: whole models whose depthwise convolution widths are not among the instantiated ones (3, 5, 7, 9, 15, 31; the
run-time-K kernels of conv.hip take them) against the CPU oracle sharing one state dict, in the pattern of
tests/test_headdim_model_gpu.py."""
import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd.config import Stats
from oracle import cases as C
from oracle import fs2_oracle as O

pytestmark = pytest.mark.gpu

N_SYMBOLS = 41
D = 256


def config_for(conv_k=9, pred_k=3, depthwise=True, learn_alignment=False, dropout=0.0):
    from fastspeech2_lightning_amd.config import FastSpeech2Config
    conf = dict(layers=1, heads=2, input_dim=D, feedforward_dim=2 * D, conv_kernel_size=conv_k, dropout=dropout)
    vp = dict(dropout=dropout, input_dim=D, kernel_size=pred_k, depthwise=depthwise, n_layers=2)
    return FastSpeech2Config(
        model=dict(encoder=conf, decoder=conf, learn_alignment=learn_alignment,
                   variance_predictors=dict(energy=vp, pitch=vp, duration=vp)),
        text=dict(symbols=dict(letters=[f"s{i}" for i in range(N_SYMBOLS - 1)])))


def pair(precision="32-true", lr=None, **kw):
    from fastspeech2_lightning_amd.model import FastSpeech2
    config = config_for(**kw)
    if lr is not None:
        config.training.optimizer.learning_rate = lr
        config.training.optimizer.warmup_steps = 2
    model = FastSpeech2(config, Stats(**C.STATS), precision=precision)
    oracle = O.FastSpeech2Oracle(config, Stats(**C.STATS), n_symbols=N_SYMBOLS)
    sd = O.seeded_state_dict(oracle.state_dict())
    oracle.load_state_dict(sd)
    model.load_state_dict(sd)
    model.postnet.dropout_p = 0.0
    oracle.postnet.dropout_p = 0.0
    return model, oracle, config


def rel(a, b, floor=1e-6):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


@pytest.mark.parametrize("kw", [dict(conv_k=11), dict(conv_k=17), dict(conv_k=33), dict(pred_k=11), dict(pred_k=13),
                                dict(pred_k=7, depthwise=False), dict(conv_k=17, learn_alignment=True)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_training_step_against_oracle(kw):
    model, oracle, _ = pair(**kw)
    model.train(); oracle.train()
    la = dict(learn_alignment=True) if kw.get("learn_alignment") else {}
    batch = O.synthetic_batch(B=2, ts_lo=20, ts_hi=33, n_symbols=N_SYMBOLS, n_mels=80, seed=3, dur_hi=5, **la)
    ref_losses = oracle.loss(oracle(batch), batch, 0)
    ref_losses["total"].backward()
    total = model.training_step(batch)
    want = float(ref_losses["total"])
    assert abs(float(total) - want) < 1e-4 * want, (float(total), want)
    got = model.store.grad_state_dict()
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in oracle.parameters() if p.grad is not None)
    worst = ("", 0.0)
    for k, p in oracle.named_parameters():
        if p.grad is None:
            continue
        r = rel(got[k].cpu().numpy(), p.grad.numpy(), floor)
        if float(p.grad.abs().max()) < floor:  # true gradient exactly zero: rounding residue on both sides
            assert r < 2e-2, (k, r)
            continue
        if r > worst[1]:
            worst = (k, r)
    assert worst[1] < 2e-3, worst


@pytest.mark.parametrize("kw", [dict(conv_k=33, pred_k=11), dict(conv_k=17, pred_k=7, depthwise=False)])
def test_eval_and_free_inference_against_oracle(kw):
    model, oracle, _ = pair(**kw)
    model.eval(); oracle.eval()
    batch = O.synthetic_batch(B=2, ts_lo=20, ts_hi=33, n_symbols=N_SYMBOLS, n_mels=80, seed=7, dur_hi=5)
    with torch.no_grad():
        ref_tf = oracle(dict(batch))
    out_tf = model(dict(batch))
    a, b = out_tf["postnet_output"].cpu().numpy(), ref_tf["postnet_output"].numpy()
    assert np.abs(a - b).max() < 1e-4 * max(1.0, np.abs(b).max())
    infer = {k: v for k, v in batch.items() if k not in ("mel", "pitch", "energy", "duration")}
    infer.update(mel=None, mel_lens=None, max_mel_len=1_000_000, duration=None)
    with torch.no_grad():
        ref = oracle(dict(infer), inference=True)
    out = model(dict(infer), inference=True)
    assert torch.equal(out["tgt_lens"].cpu(), ref["tgt_lens"].cpu().int())
    for k in ("output", "postnet_output"):
        a, b = out[k].cpu().numpy(), ref[k].numpy()
        assert a.shape == b.shape, k
        assert np.abs(a - b).max() < 1e-4 * max(1.0, np.abs(b).max()), k


def _trained(plan, steps=4):
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthetic import synthetic_batch
    config = config_for(conv_k=17, pred_k=11, dropout=0.2)
    config.training.optimizer.learning_rate = 1e-2
    config.training.optimizer.warmup_steps = 3
    model = FastSpeech2(config, Stats(**C.STATS), seed=5)
    model.plan_enabled = plan
    model.train()
    opt = model.configure_optimizers()[0][0]
    model.configure_gradient_clipping(opt, 1.0, "norm")
    rows = []
    for i in range(steps):
        b = synthetic_batch(B=4, ts_lo=6, ts_hi=12, n_symbols=N_SYMBOLS, n_mels=80, seed=21, content_seed=100 + i, dur_hi=4)
        with torch.no_grad():
            model.training_step(b)
        rows.append(model._loss_slots.clone())
        opt.step()
    torch.cuda.synchronize()
    return model, rows


def test_plan_replay_equals_eager():
    """Four steps with dropout on at K = 17 (predictors 11): replayed launch plans bit for bit equal to eager."""
    eager, want = _trained(plan=False)
    planned, got = _trained(plan=True)
    assert planned.plans.replayed >= 1 and eager.plans.recorded == 0
    for i, (w, g) in enumerate(zip(want, got)):
        assert torch.isfinite(w).all() and torch.equal(w, g), (i, w.tolist(), g.tolist())
    for name in ("flat", "adam_m", "adam_v", "grad"):
        assert torch.equal(getattr(eager.store, name), getattr(planned.store, name)), name


def test_five_bf16_mixed_steps_track_fp32_oracle():
    """Bounds of tests/test_headdim_model_gpu.py::test_five_bf16_mixed_steps_track_fp32_oracle, at K = 17 with
    depthwise predictors of width 11 (the bf16-tensor and fp32-in / bf16-out forms of the run-time-K kernels)."""
    model, oracle, config = pair(precision="bf16-mixed", lr=1e-4, conv_k=17, pred_k=11)
    model.train(); oracle.train()
    batch = O.synthetic_batch(B=4, ts_lo=8, ts_hi=20, n_symbols=N_SYMBOLS, n_mels=80, seed=21, dur_hi=5)
    o = config.training.optimizer
    ref_opt = torch.optim.AdamW(oracle.parameters(), o.learning_rate, betas=tuple(o.betas), eps=o.eps,
                                weight_decay=o.weight_decay)
    opt = model.configure_optimizers()[0][0]
    model.configure_gradient_clipping(opt, 1.0, "norm")
    totals = []
    for k in range(1, 6):
        for grp in ref_opt.param_groups:
            grp["lr"] = o.learning_rate * O.noam_scale(k - 1, o.warmup_steps)
        ref_opt.zero_grad()
        ref_losses = oracle.loss(oracle(batch), batch, 0)
        ref_losses["total"].backward()
        torch.nn.utils.clip_grad_norm_(oracle.parameters(), 1.0)
        ref_opt.step()
        model.training_step(batch)
        opt.step()
        tot = float(ref_losses["total"].detach())
        for name, v in ref_losses.items():
            got, want = float(model.last_losses[name]), float(v.detach())
            assert got == got and abs(got) < 1e6, (k, name, got)
            tol = 3e-2 * tot if name == "total" else max(0.15 * abs(want), 1e-2 * tot)
            assert abs(got - want) < tol, (k, name, got, want)
        totals.append(float(model.last_losses["total"]))
    assert totals[-1] < 0.8 * totals[0], totals


def test_checkpoint_round_trip(tmp_path):
    from fastspeech2_lightning_amd.model import FastSpeech2
    model, oracle, _ = pair(conv_k=17)
    model.eval()
    path = tmp_path / "k17.ckpt"
    model.save_checkpoint(path, global_step=3)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    dw = [k for k in ckpt["state_dict"] if k.endswith("conv_module.sequential.2.weight")]
    assert dw and all(tuple(ckpt["state_dict"][k].shape) == (D, 1, 17) for k in dw), dw
    oracle.load_state_dict(ckpt["state_dict"])
    m2 = FastSpeech2.load_from_checkpoint(path)
    m2.eval()
    batch = O.synthetic_batch(B=2, ts_lo=20, ts_hi=33, n_symbols=N_SYMBOLS, n_mels=80, seed=7, dur_hi=5)
    assert torch.equal(model(dict(batch))["postnet_output"], m2(dict(batch))["postnet_output"])


def test_construction():
    from fastspeech2_lightning_amd.model import FastSpeech2
    FastSpeech2(config_for(conv_k=63, pred_k=1), Stats(**C.STATS))
    for kw in (dict(conv_k=2), dict(conv_k=8), dict(conv_k=65), dict(pred_k=4), dict(pred_k=65)):
        with pytest.raises(ValueError, match="odd, 1 to 63"):
            FastSpeech2(config_for(**kw), Stats(**C.STATS))
