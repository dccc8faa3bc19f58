"""Attention forward + backward at B=32, T=648 (ragged lengths) for Conformer widths whose head dimension is or is not
one the kernels are built for, the share of the zero-padding launches in it, and a 32-true training step of a full-size
model at each width (GPU only).

usage: python tools/bench_attn_headdim.py [--no-step]     -- widths: (256, 2) baseline, (384, 4), (384, 2), (256, 1)
Prints one JSON line per measurement."""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fastspeech2_lightning_amd import hip as H  # noqa: E402

WIDTHS = [(256, 2), (384, 4), (384, 2), (256, 1)]
B, T = 32, 648
LENS = [648, 430, 40] + [430 + 7 * i for i in range(29)]


def timeit(fn, n=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def attention(d, heads):
    hd = d // heads
    hdp = H.attention_padded_dim(hd)
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * T, 3 * d, generator=g).cuda()
    dout = torch.randn(B, T, d, generator=g).cuda()
    lens = torch.tensor(LENS, dtype=torch.int32).cuda()
    drop = H.Drop(0.2, 7)
    o, lse, sc = H.attention_fwd(qkv, lens, B, T, heads, drop, save_scores=True)
    t_fwd = timeit(lambda: H.attention_fwd(qkv, lens, B, T, heads, drop, save_scores=True))
    t_bwd = timeit(lambda: H.attention_bwd(qkv, lens, o, dout, lse, B, T, heads, drop, scores=sc))
    t_pad = 0.0
    if hdp != hd:  # the route's own launches: fwd pads qkv, unpads o; bwd pads qkv, o, dout, unpads dqkv
        rows = B * T
        L = H.lib()
        qkvp = torch.empty(rows, 3 * heads * hdp, device="cuda")
        op = torch.empty(rows, heads * hdp, device="cuda")
        o2 = torch.empty(rows, d, device="cuda")
        dq = torch.empty(rows, 3 * d, device="cuda")

        def pads():
            L.fs2hip_attention_pad_heads(H._p(qkv), H._p(qkvp), rows, 3 * heads, hd, hdp, H._stream())
            L.fs2hip_attention_unpad_heads(H._p(op), H._p(o2), rows, heads, hdp, hd, H._stream())
            L.fs2hip_attention_pad_heads(H._p(qkv), H._p(qkvp), rows, 3 * heads, hd, hdp, H._stream())
            L.fs2hip_attention_pad_heads(H._p(o), H._p(op), rows, heads, hd, hdp, H._stream())
            L.fs2hip_attention_pad_heads(H._p(dout), H._p(op), rows, heads, hd, hdp, H._stream())
            L.fs2hip_attention_unpad_heads(H._p(qkvp), H._p(dq), rows, 3 * heads, hdp, hd, H._stream())

        t_pad = timeit(pads)
    total = t_fwd + t_bwd
    return dict(what="attention", d=d, heads=heads, head_dim=hd, kernel_width=hdp, B=B, T=T,
                fwd_ms=round(t_fwd * 1e3, 4), bwd_ms=round(t_bwd * 1e3, 4), total_ms=round(total * 1e3, 4),
                pad_unpad_ms=round(t_pad * 1e3, 4), pad_share=round(t_pad / total, 4))


def step(d, heads, steps=20):
    from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_batch
    conf = dict(input_dim=d, heads=heads)
    vp = dict(input_dim=d)
    config = FastSpeech2Config(model=dict(learn_alignment=False, encoder=conf, decoder=conf,
                                          variance_predictors=dict(energy=vp, pitch=vp, duration=vp)),
                               text=default_symbols(64))
    model = FastSpeech2(config, Stats(**DEFAULT_STATS), device="cuda:0", seed=1234, precision="32-true")
    model.train()
    opt = model.configure_optimizers()[0][0]
    model.configure_gradient_clipping(opt, 1.0, "norm")
    batch = model.prepare_batch(synthetic_batch(B=32, ts_lo=96, ts_hi=128, n_symbols=64, n_mels=80, seed=1234, dur_hi=9))

    def one():
        with torch.no_grad():
            model.training_step(batch)
        opt.step()

    for _ in range(6):  # tile tuning, then a recorded plan
        one()
    dt = timeit(one, steps)
    loss = float(model.last_losses["total"])
    return dict(what="step", d=d, heads=heads, precision="32-true", B=32, step_ms=round(dt * 1e3, 3),
                replayed=model.plans.replayed, last_total_loss=loss, mel_frames=int(batch["mel_lens"].sum()))


if __name__ == "__main__":
    H.lib()
    for d, heads in WIDTHS:
        print(json.dumps(attention(d, heads)), flush=True)
    if "--no-step" not in sys.argv:
        for d, heads in WIDTHS[:2]:
            print(json.dumps(step(d, heads)), flush=True)
