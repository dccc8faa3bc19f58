#!/usr/bin/env python
"""What ``--write-paths`` costs: ``fs2l synthesize CKPT -f LIST -b 32 --compare-to CORPUS`` with and without
``--write-paths`` on the synthetic corpus and checkpoint of ``tools/bench_mel_dtw.py`` (256 utterances, 20-160 tokens), in
alternating runs, and -- with ``--trace DIR`` -- one more run of each under ``rocprofv3 --kernel-trace --stats`` for the
kernel times (the DTW kernels with and without directions and the walk, separately).

    python tools/bench_dtw_path.py [--utterances 256] [--batch 32] [--runs 3] [--yardstick CHECKOUT] [--trace DIR] [--out FILE.md]

``--yardstick CHECKOUT``: another built checkout of this repository (the parent commit) whose ``fs2l synthesize
--compare-to`` takes part in the alternation as the yardstick.  Every run is one process of the command; the figure is the
command's own ``seconds`` (the synthesis loop, ended by a device synchronise), the process's wall time beside it.  The
traced runs are not timed: tracing slows the host.  Prints one JSON line per run and, with ``--out``, writes the tables as
markdown."""
from __future__ import annotations

import argparse
import csv
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

KERNELS = ("frame_dist_kernel", "dtw_kernel<false>", "dtw_kernel<true>", "dtw_kernel", "dtw_path_kernel", "pack_rows")


def kernel_rows(trace_dir: Path) -> list:
    """[(kernel name, calls, total ns, average ns)] of the DTW and row-packing kernels from a trace's ``kernel_stats`` csv,
    and one row for everything else."""
    files = sorted(trace_dir.rglob("*kernel_stats.csv"))
    if not files:
        raise SystemExit(f"bench_dtw_path: no kernel_stats csv under {trace_dir}")
    rows, rest = [], [0, 0]
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            name, calls, total = r["Name"], int(r["Calls"]), int(float(r["TotalDurationNs"]))
            if any(k in name for k in KERNELS):
                rows.append((name, calls, total, total / max(calls, 1)))
            else:
                rest = [rest[0] + calls, rest[1] + total]
    rows.sort()
    rows.append(("every other kernel", rest[0], rest[1], rest[1] / max(rest[0], 1)))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--yardstick", type=Path, default=None)
    ap.add_argument("--trace", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    tmp = Path(tempfile.mkdtemp(prefix="fs2l_dtw_path_"))
    corpus = tmp / "corpus"
    compare = ["--compare-to", str(corpus)]
    variants = [("--compare-to", REPO, compare), ("--compare-to --write-paths", REPO, compare + ["--write-paths"])]
    if args.yardstick is not None:
        variants.insert(0, ("--compare-to, yardstick checkout", args.yardstick.resolve(), compare))
    results = {name: [] for name, _, _ in variants}
    traces = {}
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

        def command(root, extra, out):
            return [sys.executable, str(root / "fs2l"), "synthesize", str(ckpt), "-f", str(fl), "-o", str(out),
                    "-b", str(args.batch), *extra]

        for run in range(args.runs):
            for name, root, extra in variants:   # alternating: every round runs each variant once
                out = tmp / "out"
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                r = subprocess.run(command(root, extra, out), capture_output=True, text=True, cwd=root)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return r.returncode
                rep = json.loads(r.stdout.strip().splitlines()[-1])
                rec = {"variant": name, "run": run, "seconds": rep["seconds"], "process_seconds": round(wall, 2),
                       "files": rep["files"], "frames": rep["frames"], "batches": rep["batches"],
                       "path_files": rep.get("path_files", 0),
                       "dtw_sha": _sha(out / "dtw-0.psv"), "spec_sha": _sha(out / "synthesized_spec")}
                results[name].append(rec)
                print(json.dumps(rec), flush=True)
        if args.trace is not None:
            for name, root, extra in variants:
                if root != REPO:
                    continue
                out = tmp / "out"
                shutil.rmtree(out, ignore_errors=True)
                d = args.trace / ("with_paths" if "--write-paths" in extra else "without_paths")
                shutil.rmtree(d, ignore_errors=True)
                d.mkdir(parents=True)
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--",
                       *command(root, extra, out)]
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return r.returncode
                traces[name] = kernel_rows(d)
                for row in traces[name]:
                    print(json.dumps({"variant": name, "kernel": row[0], "calls": row[1], "total_ms": round(row[2] / 1e6, 3),
                                      "average_us": round(row[3] / 1e3, 1)}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out is not None:
        lines = ["| variant | loop seconds, run by run | median | process seconds, run by run |", "|---|---|---|---|"]
        for name, _, _ in variants:
            loop = [r["seconds"] for r in results[name]]
            wall = [r["process_seconds"] for r in results[name]]
            lines.append(f"| {name} | {', '.join(f'{s:.3f}' for s in loop)} | {statistics.median(loop):.3f} | "
                         f"{', '.join(f'{s:.2f}' for s in wall)} |")
        for name, rows in traces.items():
            lines += ["", f"`{name}`, one traced run:", "", "| kernel | launches | total ms | average us |", "|---|---|---|---|"]
            lines += [f"| `{k}` | {calls} | {total / 1e6:.3f} | {avg / 1e3:.1f} |" for k, calls, total, avg in rows]
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n", encoding="utf8")
    return 0


def _sha(path: Path) -> str:
    """A short digest of a file, or of a directory's files in name order ("" when it does not exist): with
    ``FS2_GEMM_TUNE=0`` in the environment (no timing-dependent tile picks) equal digests say that two variants computed the
    same bytes."""
    import hashlib
    if not path.exists():
        return ""
    h = hashlib.sha256()
    for f in (sorted(path.iterdir()) if path.is_dir() else [path]):
        h.update(f.name.encode() + f.read_bytes())
    return h.hexdigest()[:12]


if __name__ == "__main__":
    raise SystemExit(main())
