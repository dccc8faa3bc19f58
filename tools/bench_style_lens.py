#!/usr/bin/env python
"""Time and launch count of the GST style encoder's inference forward with and without lengths.

    python tools/bench_style_lens.py [--forwards 50] [--rounds 5] [--out FILE]

Geometries: B = 32 references padded to T_ref = 257 and 1 291 frames, 80 mel bins (random values, random weights: the
kernels' time does not depend on either).  Variants, all on the SAME padded tensor:
  * ``padded``      -- ``StyleEncoder.fwd(mel)``: the path without lengths (six convolutions, then one GEMM and one
                       ``gru_gate`` launch per GRU step, driven from Python);
  * ``lens_full``   -- ``StyleEncoder.fwd(mel, lens)`` with every length equal to T_ref (the masks write nothing, the
                       recurrence runs every step: the most work the length-aware path can have);
  * ``lens_ragged`` -- the same with lengths drawn from the upper half of the extent, one reference at the maximum.
Per variant: three warm-up forwards, then a host clock around ``--forwards`` forwards ending in a device synchronise (what
a caller sees: the forward is a chain of small launches, so the host's enqueue time is part of it) and HIP events around
the same window (the device's span).  The variants alternate ``--rounds`` times; median, fastest and slowest round are
reported in us per forward.  Launches are counted once per variant, outside the timed windows, as calls of C-ABI entry
points that take a stream.  Prints one JSON line per geometry."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from fastspeech2_lightning_amd import hip as H  # noqa: E402

GEOMETRIES = [(32, 257), (32, 1291)]


class _Counting:
    """The library with every launching entry point counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = H.SIGNATURES.get(name)
        if name.startswith("fs2hip_plan_") or (sig is not None and not sig.endswith("p")):
            return fn   # (a size query: no stream parameter, nothing is launched)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def count_launches(fn) -> dict:
    real = H.lib
    proxy = _Counting(H.real_lib())
    H.lib = lambda: proxy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        H.lib = real
    return dict(sorted(proxy.calls.items()))


def timed(fn, forwards):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(forwards):
        fn()
    end.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / forwards * 1e6
    return host, start.elapsed_time(end) / forwards * 1e3   # us per forward: host clock, device events


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--forwards", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from fastspeech2_lightning_amd.config import Stats
    from fastspeech2_lightning_amd.model import FastSpeech2
    from oracle import cases as C
    cfg, _, _ = C.build("e2e_gst_multispeaker_train")
    torch.manual_seed(0)
    model = FastSpeech2(cfg, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID).eval()
    H.set_precision("32-true")
    gst = model.gst
    lines = []
    for B, T in GEOMETRIES:
        g = torch.Generator().manual_seed(1234)
        ragged = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32)
        ragged[0] = T
        full = torch.full((B,), T, dtype=torch.int32)
        mel = torch.randn(B, T, 80, generator=g)
        for b, n in enumerate(ragged.tolist()):
            mel[b, n:] = 0.0   # zero padding, as collate makes it: the masks then change nothing and every variant reads one tensor
        mel, ragged, full = mel.cuda(), ragged.cuda(), full.cuda()
        variants = {"padded": lambda: gst.fwd(mel), "lens_full": lambda: gst.fwd(mel, full),
                    "lens_ragged": lambda: gst.fwd(mel, ragged)}
        steps = T
        for _ in range(6):
            steps = (steps - 1) // 2 + 1
        rec = {"B": B, "T_ref": T, "gru_steps": steps, "ragged_lens_min": int(ragged.min()), "forwards": args.forwards,
               "rounds": args.rounds}
        same = float((gst.fwd(mel)[0] - gst.fwd(mel, full)[0]).abs().max())
        rec["lens_full_minus_padded_max_abs"] = same
        for k, fn in variants.items():
            calls = count_launches(fn)
            rec[k + "_launches"] = sum(calls.values())
            rec[k + "_launches_by_entry_point"] = calls
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.forwards))
        for k, v in times.items():
            for i, clock in enumerate(("host", "device")):
                s = sorted(t[i] for t in v)
                rec[f"{k}_{clock}_us"] = {"median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
