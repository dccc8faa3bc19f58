#!/usr/bin/env python
"""The ``fs2l train`` step loop on a synthetic RAGGED epoch, with and without length-bucketed batches.

``bench.py`` times one fixed batch geometry, which always replays its launch plan; real data pads every random batch
differently and never does.  This tool measures the loop a user of ``fs2l train`` gets: utterance lengths drawn as
``synthetic.synthetic_lengths`` draws them (LJSpeech-like spread), items resident in host memory, ``collate`` ->
``DevicePrefetcher`` -> ``training_step`` -> optimizer, one GPU.  It is not part of ``bench.py``.

    python tools/bench_ragged.py                       # both settings, 3 alternations of (unbucketed, bucketed)
    python tools/bench_ragged.py --settings bf16-mixed:64 --rounds 1
    python tools/bench_ragged.py --worker --precision bf16-mixed --batch 64 --mode bucketed   # one measurement

Every measurement is a fresh child process under a time limit (``--limit`` seconds); the first failure ends the run.
Reported per measurement: ms per step (wall, device-synchronised per epoch), host enqueue ms per step (the loop's own time
before the closing synchronisation), real mel frames per second, the padded share of the mel frames, and the three plan
counters.  The yardstick for the bucketed loop is the unbucketed loop of the same process chain on the same items.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

def worker(args) -> dict:
    import torch

    from fastspeech2_lightning_amd import data as D
    from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_item, synthetic_lengths

    torch.cuda.set_device(0)
    config = FastSpeech2Config(model=dict(learn_alignment=False), text=default_symbols(64))
    model = FastSpeech2(config, Stats(**DEFAULT_STATS), device="cuda:0", seed=1234, precision=args.precision)
    model.train()
    opt = model.configure_optimizers()[0][0]
    model.configure_gradient_clipping(opt, 1.0, "norm")
    lengths = synthetic_lengths(args.items, seed=args.seed)
    items = [synthetic_item(t, m, n_symbols=64, n_mels=80, seed=i) for i, (t, m) in enumerate(lengths)]
    bucketed = args.mode == "bucketed"

    def epoch_batches(epoch):
        if bucketed:
            s = D.LengthBucketBatchSampler(lengths, args.batch, args.buckets or None, seed=args.seed, epoch=epoch)
            ds = D.BucketedDataset(items, s)
            return [D.collate_bucketed([ds[i] for i in b], learn_alignment=False, pin_memory=True) for b in s]
        idx = D.random_batches(len(items), args.batch, args.seed + epoch)
        return [D.collate([items[i] for i in b], learn_alignment=False, pin_memory=True) for b in idx]

    def run_epoch(epoch):
        """(steps, wall seconds, host seconds, real frames, padded frames) of one epoch; collation is not timed (data
        resident), the H2D copies run on the prefetcher's stream as in ``Trainer.fit``."""
        batches = epoch_batches(epoch)
        real = sum(int(b["mel_lens"].sum()) for b in batches)
        padded = sum(len(b["mel_lens"]) * (b["bucket_geometry"][1] if bucketed else int(b["max_mel_len"])) for b in batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in D.DevicePrefetcher(batches, model.prepare_batch, model.device_):
            with torch.no_grad():
                model.training_step(batch)
            opt.step()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        return len(batches), time.perf_counter() - t0, host, real, padded

    epoch = 0
    for _ in range(args.warmup_epochs):
        run_epoch(epoch)
        epoch += 1
    base = (model.plans.replayed, model.plans.recorded, model.plans.eager)
    steps = wall = host = real = padded = 0
    while steps < args.steps:
        n, w, h, r, p = run_epoch(epoch)
        steps, wall, host, real, padded, epoch = steps + n, wall + w, host + h, real + r, padded + p, epoch + 1
    now = (model.plans.replayed, model.plans.recorded, model.plans.eager)
    loss = model.losses_to_host()["total"]
    return dict(mode=args.mode, precision=args.precision, batch=args.batch, items=args.items, steps=steps,
                ms_per_step=round(wall / steps * 1e3, 3), host_enqueue_ms_per_step=round(host / steps * 1e3, 3),
                real_mel_frames_per_s=round(real / wall, 1), padded_frame_share=round(1.0 - real / padded, 4),
                plans_replayed=now[0] - base[0], plans_recorded=now[1] - base[1], plans_eager=now[2] - base[2],
                warmup_epochs=args.warmup_epochs, last_total_loss=round(float(loss), 5))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--settings", nargs="+", default=["bf16-mixed:64", "32-true:32"], metavar="PRECISION:BATCH")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of (unbucketed, bucketed) per setting")
    ap.add_argument("--steps", type=int, default=200, help="timed steps per measurement, at least (whole epochs)")
    ap.add_argument("--warmup-epochs", type=int, default=3, help="untimed epochs first (tile tuner, plans recorded)")
    ap.add_argument("--items", type=int, default=0, help="utterances in the epoch (default: 24 batches' worth plus 3/8 of a batch, so that buckets leave short leftover batches)")
    ap.add_argument("--buckets", type=int, default=0, help="bucket count (default: the launch-plan limit)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--limit", type=int, default=420, help="seconds a measurement's process may take")
    ap.add_argument("--out", type=Path, default=None, help="also append every result line to this file")
    ap.add_argument("--worker", action="store_true", help="one measurement in this process (what the driver starts)")
    ap.add_argument("--precision", default="bf16-mixed")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--mode", choices=["bucketed", "unbucketed"], default="bucketed")
    args = ap.parse_args()
    if args.worker:
        args.items = args.items or 24 * args.batch + 3 * args.batch // 8   # not a multiple of batch * buckets: leftovers
        print(json.dumps(worker(args)), flush=True)
        return 0
    results = []
    for setting in args.settings:
        precision, batch = setting.split(":")
        for rnd in range(args.rounds):
            for mode in ("unbucketed", "bucketed"):
                cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--precision", precision, "--batch", batch,
                       "--mode", mode, "--steps", str(args.steps), "--warmup-epochs", str(args.warmup_epochs),
                       "--items", str(args.items), "--buckets", str(args.buckets), "--seed", str(args.seed)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    print(json.dumps(dict(setting=setting, round=rnd, mode=mode, error="time limit")), flush=True)
                    return 1
                if r.returncode != 0:   # nothing more is started on the GPU after a failure
                    print(json.dumps(dict(setting=setting, round=rnd, mode=mode, error=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                    return 1
                rec = dict(json.loads(r.stdout.strip().splitlines()[-1]), round=rnd)
                results.append(rec)
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a", encoding="utf8") as f:
                        f.write(line + "\n")
    summary = {}
    for setting in args.settings:
        precision, batch = setting.split(":")
        for mode in ("unbucketed", "bucketed"):
            rows = [r for r in results if r["precision"] == precision and r["batch"] == int(batch) and r["mode"] == mode]
            for key in ("ms_per_step", "host_enqueue_ms_per_step", "real_mel_frames_per_s", "padded_frame_share"):
                vals = sorted(r[key] for r in rows)
                summary[f"{setting} {mode} {key}"] = dict(min=vals[0], median=vals[len(vals) // 2], max=vals[-1])
    line = json.dumps(dict(summary=summary))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a", encoding="utf8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
