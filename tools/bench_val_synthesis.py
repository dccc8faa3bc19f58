#!/usr/bin/env python
"""What ``fs2l train --val-synthesis [--val-cepstra K]`` costs, and the new kernel beside its neighbours.

    python tools/bench_val_synthesis.py [--utterances 256] [--batch 32] [--runs 5] [--out FILE.md]

1. One validation pass -- ``data.validate`` over the same in-memory batches (the ragged synthetic epoch of
   ``synthetic_lengths``: 20-160 tokens, about 5 frames per token, full-size default model) -- plain, with
   ``synthesis=SynthesisValidation()`` and with ``SynthesisValidation(cepstra=13)``, alternating, after one untimed pass of each;
   a host clock around work that ends in the pass's own device-to-host read, then a synchronise.  The model is untrained; its
   duration predictor's bias is set so that free synthesis produces about the corpus' frames per token, i.e. cost matrices
   of the size a trained model would give.
2. ``fs2hip_cepstra`` alone at B = 32, T = 648, C = 80, K = 13 (every row valid) next to ``fs2hip_frame_dist`` at the same
   shape (648 x 648 boxes, C = 80, and C = 13 as the cepstral distance runs it) and ``fs2hip_dtw`` on that matrix: device
   events around 50 back-to-back launches, 5 windows each, the median per launch.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from fastspeech2_lightning_amd import data as D  # noqa: E402
from fastspeech2_lightning_amd import hip as H  # noqa: E402
from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats  # noqa: E402
from fastspeech2_lightning_amd.model import FastSpeech2  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_item, synthetic_lengths  # noqa: E402


def kernel_times(B=32, T=648, C=80, K=13, launches=50, windows=5) -> dict:
    g = torch.Generator().manual_seed(0)
    a = torch.randn(B, T, C, generator=g).cuda()
    b = torch.randn(B, T, C, generator=g).cuda()
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ca, cb = H.cepstra(a, lens, K), H.cepstra(b, lens, K)
    cost = H.frame_dist(a, lens, b, lens)
    out = torch.empty_like(ca)
    total, steps = H.dtw(cost, lens, lens)
    calls = {"cepstra (C = 80, K = 13)": lambda: H.cepstra(a, lens, K, out=out),
             "frame_dist (C = 80)": lambda: H.frame_dist(a, lens, b, lens, out=cost),
             "frame_dist (C = 13)": lambda: H.frame_dist(ca, lens, cb, lens, out=cost),
             "dtw": lambda: H.dtw(cost, lens, lens, total=total, steps=steps)}
    res = {}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(windows):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                fn()
            end.record()
            torch.cuda.synchronize()
            per.append(start.elapsed_time(end) * 1000.0 / launches)
        res[name] = {"us_per_launch": [round(x, 2) for x in per], "median_us": round(statistics.median(per), 2)}
        print(json.dumps({"kernel": name, **res[name]}), flush=True)
    # bytes the cepstra launch has to move (x in, out out; the table stays in cache) over its time
    moved = B * T * (C + K) * 4
    res["cepstra bytes"] = moved
    return res


def validation_times(utterances: int, batch: int, runs: int) -> tuple:
    config = FastSpeech2Config(model=dict(learn_alignment=False), text=default_symbols(64))
    model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234)
    lengths = list(synthetic_lengths(utterances, seed=1234))
    per_token = sum(f for _, f in lengths) / sum(t for t, _ in lengths)
    sd = model.state_dict()
    sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([math.log(per_token + 1.0)])
    model.load_state_dict(sd)
    model.train()
    n_mels = config.preprocessing.audio.n_mels
    items = []
    for u, (n_tok, n_frames) in enumerate(lengths):
        item = synthetic_item(n_tok, n_frames, n_symbols=64, n_mels=n_mels, seed=1234 + u)
        item.update(basename=f"utt{u:04d}", speaker="default", language="default", speaker_id=0, language_id=0)
        items.append(item)
    batches = [model.prepare_batch(D.collate(items[i:i + batch], learn_alignment=False)) for i in range(0, len(items), batch)]
    variants = [("plain", None), ("--val-synthesis", D.SynthesisValidation()),
                ("--val-synthesis --val-cepstra 13", D.SynthesisValidation(cepstra=13))]
    results = {name: [] for name, _ in variants}
    last = {}
    for run in range(runs + 1):   # run 0 is the untimed warm-up of every variant's shapes
        for name, opts in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = D.validate(model, batches) if opts is None else D.validate(model, batches, synthesis=opts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if run:
                results[name].append(dt)
                print(json.dumps({"variant": name, "run": run, "seconds": round(dt, 4)}), flush=True)
    print(json.dumps({"metrics": last["--val-synthesis --val-cepstra 13"], "frames_recorded": sum(f for _, f in lengths)}), flush=True)
    return results, last, len(batches)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_val_synthesis needs the GPU: a CPU run cannot time anything")
    kt = kernel_times()
    vt, last, n_batches = validation_times(args.utterances, args.batch, args.runs)
    if args.out is not None:
        lines = [f"Validation pass, {args.utterances} utterances in {n_batches} batches of {args.batch}, seconds:", "",
                 "| variant | run by run | median |", "|---|---|---|"]
        for name, secs in vt.items():
            lines.append(f"| {name} | {', '.join(f'{s:.3f}' for s in secs)} | {statistics.median(secs):.3f} |")
        lines += ["", "Kernels at B = 32, T = 648 (every row valid), microseconds per launch:", "",
                  "| kernel | window by window | median |", "|---|---|---|"]
        for name, r in kt.items():
            if isinstance(r, dict):
                lines.append(f"| {name} | {', '.join(f'{x:.1f}' for x in r['us_per_launch'])} | {r['median_us']:.1f} |")
        lines += ["", "Metrics of the last pass: " + json.dumps(last["--val-synthesis --val-cepstra 13"])]
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n", encoding="utf8")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
