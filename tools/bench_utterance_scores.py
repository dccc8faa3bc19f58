#!/usr/bin/env python
"""What batching buys when a corpus is scored: ``fs2l synthesize -T DIR --return-scores --scores-only`` at ``-b 1`` (how
the reference's scorer runs, fs2/prediction_writing_callback.py:138-211) against ``-b 32``.

    python tools/bench_utterance_scores.py [--utterances 256] [--batches 1 32] [--precision 32-true] [--out FILE.md]

Headline model configuration (durations given, no aligner) with random weights; a synthetic teacher-forcing corpus of
LJSpeech-like lengths (20-160 tokens, ~5 frames per token: ``synthetic_lengths``) with random mels and the durations that
add up to them, written to a temporary directory the way the preprocessor lays it out.  Every batch size is ONE run of the command in a process of its
own -- checkpoint load, the GEMM tile tuner's first-use timings and the file reads included, which is what a user waits
for; the command's own ``seconds`` (the synthesis loop alone) is reported beside the process's wall time.  Prints one JSON
line per run and, with ``--out``, writes the table as markdown.
"""
from __future__ import annotations

import argparse
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from fastspeech2_lightning_amd import data as D  # noqa: E402
from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_item, synthetic_lengths  # noqa: E402


def write_corpus(root: Path, config, n: int, seed: int = 1234) -> Path:
    audio = config.preprocessing.audio
    rows = []
    for u, (n_tok, n_frames) in enumerate(synthetic_lengths(n, seed=seed)):
        item = synthetic_item(n_tok, n_frames, n_symbols=64, n_mels=audio.n_mels, seed=seed + u)
        bn = f"utt{u:04d}"
        for kind, fn, t in (("spec", f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt", item["mel"].transpose(0, 1).contiguous()),
                            ("duration", "duration.pt", item["duration"])):
            p = D.feature_path(root, kind, bn, "default", "default", fn)
            p.parent.mkdir(parents=True, exist_ok=True)
            torch.save(t, p)
        toks = "/".join(f"s{int(i) - 1:02d}" for i in item["text"])
        rows.append("|".join([bn, "default", "default", f"synthetic utterance {u:04d}", toks]))
    fl = root / "filelist.psv"
    fl.write_text("basename|language|speaker|characters|character_tokens\n" + "\n".join(rows) + "\n", encoding="utf8")
    return fl


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--precision", default="32-true")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    tmp = Path(tempfile.mkdtemp(prefix="fs2l_scores_"))
    results = []
    try:
        config = FastSpeech2Config(model=dict(learn_alignment=False), text=default_symbols(64))   # durations are given
        model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234)
        ckpt = tmp / "model.ckpt"
        model.save_checkpoint(ckpt, global_step=0)
        del model
        fl = write_corpus(tmp / "corpus", config, args.utterances)
        for b in args.batches:
            out = tmp / f"out_b{b}"
            cmd = [sys.executable, str(REPO / "fs2l"), "synthesize", str(ckpt), "-f", str(fl), "-T", str(tmp / "corpus"),
                   "-o", str(out), "-b", str(b), "--precision", args.precision, "--return-scores", "--scores-only"]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                print(r.stderr[-2000:], file=sys.stderr)
                return r.returncode
            rep = json.loads(r.stdout.strip().splitlines()[-1])
            rows = (out / "scores-0.psv").read_text(encoding="utf8").splitlines()
            assert len(rows) == args.utterances + 1, len(rows)
            rec = {"batch_size": b, "utterances": rep["utterances"], "frames": rep["frames"], "batches": rep["batches"],
                   "loop_seconds": rep["seconds"], "loop_utterances_per_s": round(rep["utterances"] / rep["seconds"], 1),
                   "process_seconds": round(wall, 2), "process_utterances_per_s": round(rep["utterances"] / wall, 1),
                   "precision": args.precision}
            print(json.dumps(rec), flush=True)
            results.append(rec)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out is not None:
        lines = ["| -b | batches | loop seconds | utterances/s (loop) | process seconds | utterances/s (process) |",
                 "|---|---|---|---|---|---|"]
        lines += [f"| {r['batch_size']} | {r['batches']} | {r['loop_seconds']} | {r['loop_utterances_per_s']} | "
                  f"{r['process_seconds']} | {r['process_utterances_per_s']} |" for r in results]
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n", encoding="utf8")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
