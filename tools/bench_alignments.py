#!/usr/bin/env python
"""What ``--write-alignments`` costs: ``fs2l synthesize CKPT -f LIST -T DIR -b 32`` on the synthetic teacher-forcing corpus of
``tools/bench_utterance_scores.py`` (256 utterances, 20-160 tokens), with and without the flag, in alternating runs.

    python tools/bench_alignments.py [--utterances 256] [--batch 32] [--runs 3] [--parent DIR] [--out FILE.md]

Every run is one process of the command (checkpoint load, the GEMM tile tuner's first-use timings and the file reads
included); the figure is the command's own ``seconds`` (the synthesis loop: file reads, collate, forward, the packing
kernels, the copy, the wait, the writers), the process's wall time beside it.  ``--parent DIR``: a built checkout of the
commit before the flag existed; its ``fs2l`` runs the same command without the flag in the same alternation.  Prints one
JSON line per run and, with ``--out``, writes the table as markdown.
"""
from __future__ import annotations

import argparse
import json
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

from bench_utterance_scores import write_corpus  # noqa: E402

from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    tmp = Path(tempfile.mkdtemp(prefix="fs2l_alignments_"))
    variants = [("flag off", REPO, []), ("flag on", REPO, ["--write-alignments"])]
    if args.parent is not None:
        variants.insert(0, ("parent commit, no flag", args.parent.resolve(), []))
    results = {name: [] for name, _, _ in variants}
    try:
        config = FastSpeech2Config(model=dict(learn_alignment=False), text=default_symbols(64))   # durations are given
        model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234)
        ckpt = tmp / "model.ckpt"
        model.save_checkpoint(ckpt, global_step=0)
        del model
        fl = write_corpus(tmp / "corpus", config, args.utterances)
        for run in range(args.runs):
            for name, root, extra in variants:   # alternating: every round runs each variant once
                out = tmp / "out"
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, str(root / "fs2l"), "synthesize", str(ckpt), "-f", str(fl), "-T", str(tmp / "corpus"),
                       "-o", str(out), "-b", str(args.batch), *extra]
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return r.returncode
                rep = json.loads(r.stdout.strip().splitlines()[-1])
                rec = {"variant": name, "run": run, "seconds": rep["seconds"], "process_seconds": round(wall, 2),
                       "files": rep["files"], "alignment_files": rep.get("alignment_files"), "frames": rep["frames"],
                       "batches": rep["batches"]}
                results[name].append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out is not None:
        lines = ["| variant | loop seconds, run by run | median | process seconds, run by run |", "|---|---|---|---|"]
        for name, _, _ in variants:
            loop = [r["seconds"] for r in results[name]]
            wall = [r["process_seconds"] for r in results[name]]
            lines.append(f"| {name} | {', '.join(f'{s:.3f}' for s in loop)} | {statistics.median(loop):.3f} | "
                         f"{', '.join(f'{s:.2f}' for s in wall)} |")
        args.out.write_text("\n".join(lines) + "\n", encoding="utf8")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
