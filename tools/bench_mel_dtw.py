#!/usr/bin/env python
"""What ``--compare-to`` costs: ``fs2l synthesize CKPT -f LIST -b 32`` (free synthesis) on the synthetic corpus of
``tools/bench_utterance_scores.py`` (256 utterances, 20-160 tokens), plain, with ``--exact-lengths`` (which the option forces
on) and with ``--compare-to CORPUS``, in alternating runs.

    python tools/bench_mel_dtw.py [--utterances 256] [--batch 32] [--runs 3] [--out FILE.md]

Every run is one process of the command (checkpoint load, the GEMM tile tuner's first-use timings and the file reads
included); the figure is the command's own ``seconds`` (the synthesis loop: file reads, collate, forward, the DTW kernels,
the packing kernel, the copy, the wait, the writers), the process's wall time beside it.  The model is untrained; its
duration predictor's bias is set so that free synthesis produces about the corpus' frames per token, i.e. cost matrices of
the size a trained model would give.  Prints one JSON line per run and, with ``--out``, writes the table as markdown.
"""
from __future__ import annotations

import argparse
import json
import math
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import torch  # noqa: E402
from bench_utterance_scores import write_corpus  # noqa: E402

from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_lengths  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    tmp = Path(tempfile.mkdtemp(prefix="fs2l_mel_dtw_"))
    corpus = tmp / "corpus"
    variants = [("plain", []), ("--exact-lengths", ["--exact-lengths"]), ("--compare-to", ["--compare-to", str(corpus)])]
    results = {name: [] for name, _ in variants}
    try:
        config = FastSpeech2Config(model=dict(learn_alignment=False), text=default_symbols(64))
        model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234)
        lengths = list(synthetic_lengths(args.utterances, seed=1234))
        per_token = sum(f for _, f in lengths) / sum(t for t, _ in lengths)
        sd = model.state_dict()
        sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([math.log(per_token + 1.0)])
        model.load_state_dict(sd)
        ckpt = tmp / "model.ckpt"
        model.save_checkpoint(ckpt, global_step=0)
        del model
        fl = write_corpus(corpus, config, args.utterances)
        for run in range(args.runs):
            for name, extra in variants:   # alternating: every round runs each variant once
                out = tmp / "out"
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, str(REPO / "fs2l"), "synthesize", str(ckpt), "-f", str(fl), "-o", str(out),
                       "-b", str(args.batch), *extra]
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return r.returncode
                rep = json.loads(r.stdout.strip().splitlines()[-1])
                rec = {"variant": name, "run": run, "seconds": rep["seconds"], "process_seconds": round(wall, 2),
                       "files": rep["files"], "frames": rep["frames"], "batches": rep["batches"]}
                dtw = out / "dtw-0.psv"
                if dtw.exists():
                    rows = dtw.read_text(encoding="utf8").splitlines()[1:]
                    cols = [ln.split("|") for ln in rows]
                    rec.update(dtw_rows=len(rows), path_cells=sum(int(c[5]) for c in cols),
                               ref_frames=sum(int(c[7]) for c in cols))
                results[name].append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out is not None:
        lines = ["| variant | loop seconds, run by run | median | process seconds, run by run |", "|---|---|---|---|"]
        for name, _ in variants:
            loop = [r["seconds"] for r in results[name]]
            wall = [r["process_seconds"] for r in results[name]]
            lines.append(f"| {name} | {', '.join(f'{s:.3f}' for s in loop)} | {statistics.median(loop):.3f} | "
                         f"{', '.join(f'{s:.2f}' for s in wall)} |")
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n", encoding="utf8")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
