#!/usr/bin/env python
"""Kernel time of ``fs2hip_attn_prior`` against the ``fs2hip_attn_softmax`` launch that reads its result.

    python tools/bench_attn_prior.py [--launches 20] [--rounds 7] [--out FILE]

Geometries: (B, Tm, Ts) = (32, 648, 128), the benchmark's, and (64, 1291, 200), the GST configuration's.  Lengths: "full"
-- every utterance as long as the geometry, the most work the prior kernel can have -- and "ragged" -- mel lengths drawn
from the upper half of the extent, texts in proportion, one utterance at the maximum (padding rows are plain zero stores).
Variants: the prior's three forms (csrc/attn_prior.hip) -- every lgamma from a table of ``lgamma(j + 1)``, what ``scaling =
1`` takes by default; a table of the ``k``-only terms (``FS2_ATTN_PRIOR_TABLE=1``: what every other scaling takes); every
lgamma evaluated in place (``FS2_ATTN_PRIOR_TABLE=0``) -- and ``attn_softmax`` on a tensor of the same shape: it streams the
same ``B * Tm * Ts`` elements (two reads, two writes), so it is the yardstick for "a launch over this tensor".
Per variant: three warm-up launches, then HIP events around ``--launches`` back-to-back launches; the variants alternate
``--rounds`` times and the median round is reported (us per launch), with the fastest and slowest beside it.
Prints one JSON line per geometry and length distribution."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from fastspeech2_lightning_amd import hip as H  # noqa: E402

GEOMETRIES = [(32, 648, 128), (64, 1291, 200)]


def lengths(B, Tm, Ts, ragged, seed=1234):
    if not ragged:
        return torch.full((B,), Tm, dtype=torch.int32), torch.full((B,), Ts, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    mel = torch.randint(Tm // 2, Tm + 1, (B,), generator=g, dtype=torch.int32)
    mel[0] = Tm
    src = (mel.double() * Ts / Tm).round().clamp(1, Ts).to(torch.int32)
    return mel, src


def timed(fn, launches):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / launches * 1e3   # us per launch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = []
    for B, Tm, Ts in GEOMETRIES:
        for ragged in (False, True):
            mel, src = (t.cuda() for t in lengths(B, Tm, Ts, ragged))
            prior = torch.empty(B, Tm, Ts, device="cuda")
            logits = torch.randn(B, Tm, Ts, device="cuda")

            def form(value):
                def run():
                    if value is None:
                        os.environ.pop("FS2_ATTN_PRIOR_TABLE", None)
                    else:
                        os.environ["FS2_ATTN_PRIOR_TABLE"] = value
                    H.attn_prior(mel, src, Tm, Ts, out=prior)
                return run

            def softmax():
                H.attn_softmax(logits, prior, src)

            variants = {"attn_prior_int_table": form(None), "attn_prior_k_table": form("1"), "attn_prior_in_place": form("0"),
                        "attn_softmax": softmax}
            results = []
            for k in list(variants)[:3]:
                variants[k]()
                results.append(prior.clone())
            same = all(bool(torch.equal(results[0], r)) for r in results[1:])
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.launches))
            os.environ.pop("FS2_ATTN_PRIOR_TABLE", None)
            rec = {"B": B, "Tm": Tm, "Ts": Ts, "lengths": "ragged" if ragged else "full",
                   "valid_elements": int((mel.long() * src.long()).sum()), "elements": B * Tm * Ts,
                   "launches": args.launches, "rounds": args.rounds,
                   "forms_bit_identical": same}
            for k, v in times.items():
                v = sorted(v)
                rec[k + "_us"] = {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del prior, logits
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
