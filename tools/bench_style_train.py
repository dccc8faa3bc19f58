#!/usr/bin/env python
"""Cost of length-aware training of the GST style encoder (``FastSpeech2.style_lengths``, ``fs2l train --style-lengths``).

    python tools/bench_style_train.py [--steps 20] [--passes 50] [--rounds 5] [--off-only] [--out FILE]

Geometries: the training batch of ``bench.py --gst`` (fp32, B = 32, texts of 96 to 128 tokens, the longest mel about 1 300
frames) and a short one (texts of 24 to 32 tokens, mels padded to 257 frames).  Per geometry, with the flag off and on:
  * ``encoder`` -- the style encoder's forward + backward alone on the batch's mels (``StyleEncoder.fwd`` /
    ``fwd_train`` + ``bwd``, eager): launches (calls of C-ABI entry points that take a stream, counted once outside the
    timed windows), a host clock around ``--passes`` passes ending in a device synchronise, and HIP events around the same
    window;
  * ``step`` -- the whole training step (forward, loss, backward, optimizer) as ``bench.py`` times it, replayed from its
    launch plan: HIP events around ``--steps`` steps.
The variants alternate ``--rounds`` times; median, fastest and slowest round are reported.  ``--off-only`` measures the
flag-off variants alone and touches nothing this flag added, so the same script also runs on a checkout that predates it
(the comparison with the parent commit).  Prints one JSON line per geometry."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fastspeech2_lightning_amd import hip as H  # noqa: E402

from bench_style_lens import count_launches  # noqa: E402  (tools/ is the script's directory)


def short_batch(B, frames):
    """A batch of short utterances whose mel is padded with zeros to ``frames`` frames (what a length bucket does)."""
    from fastspeech2_lightning_amd.synthetic import synthetic_batch
    b = synthetic_batch(B=B, ts_lo=24, ts_hi=32, n_symbols=64, n_mels=80, seed=1234, dur_hi=13)   # (the longest mel: 247 frames)
    Tm = b["mel"].shape[1]
    assert Tm <= frames, (Tm, frames)
    b["mel"] = F.pad(b["mel"], (0, 0, 0, frames - Tm))
    b["max_mel_len"] = frames
    b["speaker_id"] = torch.arange(B, dtype=torch.int32) % 16
    return b


def spread(values, digits=1):
    s = sorted(values)
    return {"median": round(s[len(s) // 2], digits), "min": round(s[0], digits), "max": round(s[-1], digits)}


def time_encoder(fn, passes):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(passes):
        fn()
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / passes * 1e6, start.elapsed_time(end) / passes * 1e3   # us per pass


def time_steps(rig, steps):
    for _ in range(2):
        rig.step()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        rig.step()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps   # ms per step


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    import bench
    flags = (False,) if args.off_only else (False, True)
    lines = []
    for name in ("bench_gst", "short_257"):
        rig = bench.Rig("32-true", 32, gst=True)
        if name == "short_257":
            rig.batch = short_batch(32, 257)
            rig.dev_batch = rig.model.prepare_batch(rig.batch)
        model, gst = rig.model, rig.model.gst
        mel, lens = rig.dev_batch["mel"], rig.dev_batch["mel_lens"]
        B, T, _ = mel.shape
        gru_steps = T
        for _ in range(6):
            gru_steps = (gru_steps - 1) // 2 + 1
        rec = {"geometry": name, "B": B, "padded_frames": T, "frames": int(lens.sum()), "shortest": int(lens.min()),
               "longest": int(lens.max()), "gru_steps": gru_steps, "steps": args.steps, "passes": args.passes,
               "rounds": args.rounds}
        d_style = torch.randn(B, 256, device=mel.device)

        def encoder(on):
            style, ctx = gst.fwd_train(mel, lens) if on else gst.fwd(mel)
            gst.bwd(d_style, ctx)
            H.flush_grad_reductions()

        tag = {False: "off", True: "on"}
        for on in flags:
            calls = count_launches(lambda: encoder(on))
            rec[f"encoder_{tag[on]}_launches"] = sum(calls.values())
            rec[f"encoder_{tag[on]}_launches_by_entry_point"] = calls
        enc = {on: [] for on in flags}
        for _ in range(args.rounds):
            for on in flags:
                enc[on].append(time_encoder(lambda: encoder(on), args.passes))
        for on in flags:
            rec[f"encoder_{tag[on]}_host_us"] = spread([t[0] for t in enc[on]])
            rec[f"encoder_{tag[on]}_device_us"] = spread([t[1] for t in enc[on]])
        H.drop_pending_reductions()
        step = {on: [] for on in flags}
        for _ in range(2):   # every variant's plan is recorded before the rounds (twice: a variant's first steps tune the
            for on in flags:  # tiles of its own GEMM shapes, and the tile table is part of the other's plan signature)
                if on or not args.off_only:
                    model.style_lengths = on
                rig.reset_training_state()
                rig.settle()
        for _ in range(args.rounds):
            for on in flags:
                if on or not args.off_only:
                    model.style_lengths = on
                rig.reset_training_state()
                step[on].append(time_steps(rig, args.steps))
        for on in flags:
            rec[f"step_{tag[on]}_ms"] = spread(step[on], 3)
        rec["plans"] = model.plans.counters()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del rig, model, gst
        H.release_scratch()
        torch.cuda.empty_cache()
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
