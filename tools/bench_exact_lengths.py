#!/usr/bin/env python
"""What exact-length inference costs: the free-inference forward of one batch, ``exact_lengths`` off against on.

    python tools/bench_exact_lengths.py [--batch 32] [--reps 200] [--rounds 3] [--precisions 32-true bf16-mixed] [--out FILE]

Headline model configuration, random weights, the duration predictor's bias set so that a token lasts ~5 frames
(tools/bench_synthesize.py's set-up), 512 synthetic texts of LJSpeech-like length (20-160 tokens).  Two batches of
``--batch`` texts: "sorted" is one batch of ``synthesis_batches(sort=True)`` from the middle of the length order (little
padding), "unsorted" the first ``--batch`` texts in input order (ragged).  Per batch, after a warm-up of both variants (the
GEMM tile tuner times each new shape once), the two variants alternate ``--rounds`` times with ``--reps`` forwards each:
a host clock around the forwards, ending in a device synchronise (a free-inference forward reads the frame totals on the
host once, so its time is host enqueue + that wait, which is what a caller sees).  The mask's launches are counted
(``hip.ZERO_TAIL_CALLS``), and the two variants' frame counts are printed: the flag changes the durations, hence the work.
Prints one JSON line per precision.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from fastspeech2_lightning_amd import data as D  # noqa: E402
from fastspeech2_lightning_amd import hip  # noqa: E402
from fastspeech2_lightning_amd.config import FastSpeech2Config, InferenceControl, Stats  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols  # noqa: E402
from tools.bench_synthesize import entries  # noqa: E402


def timed(model, batch, exact, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = model(batch, InferenceControl(), inference=True, exact_lengths=exact)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precisions", nargs="+", default=["32-true", "bf16-mixed"])
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    lines = []
    for precision in args.precisions:
        config = FastSpeech2Config(text=default_symbols(64))
        model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234,
                            precision=precision)
        sd = model.state_dict()
        sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([1.79])  # exp(1.79) - 1 ~ 5 frames a token
        model.load_state_dict(sd)
        model.eval()
        ds = D.SynthesisDataset(entries(args.utterances), config, model.lang2id, model.speaker2id)
        by_length = D.synthesis_batches(ds.token_counts, args.batch, True)
        picks = {"sorted": by_length[len(by_length) // 2], "unsorted": list(range(args.batch))}
        rec = {"precision": precision, "batch": args.batch, "reps": args.reps, "rounds": args.rounds, "batches": {}}
        for name, idx in picks.items():
            batch = D.collate([ds[i] for i in idx], learn_alignment=False, pin_memory=True)
            tokens = [ds.token_counts[i] for i in idx]
            r = {"tokens_min_max": [min(tokens), max(tokens)], "off_ms": [], "on_ms": []}
            for exact in (False, True):   # warm-up: both variants tune their GEMM shapes
                timed(model, batch, exact, 5)
            for _ in range(args.rounds):
                for exact in (False, True):
                    n0 = hip.ZERO_TAIL_CALLS[0]
                    ms, out = timed(model, batch, exact, args.reps)
                    r["on_ms" if exact else "off_ms"].append(round(ms, 4))
                    key = "on" if exact else "off"
                    r[f"{key}_mask_launches_per_forward"] = (hip.ZERO_TAIL_CALLS[0] - n0) // args.reps
                    lens = out["tgt_lens"].cpu()
                    r[f"{key}_frames"] = int(lens.sum())
                    r[f"{key}_padded_frames"] = int(out["output"].shape[0] * out["output"].shape[1])
            r["overhead_percent_of_medians"] = round(
                100.0 * (sorted(r["on_ms"])[len(r["on_ms"]) // 2] / sorted(r["off_ms"])[len(r["off_ms"]) // 2] - 1.0), 2)
            rec["batches"][name] = r
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        if args.out is not None:
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text("\n".join(lines) + "\n")
        del model
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
