#!/usr/bin/env python
"""Bulk synthesis throughput: the per-utterance read-back of ``predict_step`` + ``SpecWriter.write`` against the packed,
pipelined loop of ``synthesis.synthesize`` (what ``fs2l synthesize`` runs).

    python tools/bench_synthesize.py [--utterances 512] [--batch 32] [--rounds 3] [--precisions 32-true bf16-mixed] [--out FILE]

Headline model configuration, random weights with the duration predictor's bias set so that a token lasts ~5 frames,
synthetic texts of LJSpeech-like length (20-160 tokens).  In ONE process, after a warm-up pass of every path over every
batch shape (the GEMM tile tuner times each new shape once), the three paths alternate ``--rounds`` times:

  a  the per-batch loop a user had to write: ``collate -> predict_step -> SpecWriter.write``, input order
  b  ``synthesize(sort=False)``: the same batches through ``fs2hip_pack_spec`` + one asynchronous copy per batch
  c  ``synthesize(sort=True)``: batches sorted by token count (less padding; other batches, so other files)

Host clock around the whole loop, ending in a device synchronise; files go to the same temporary directory in all three.
Prints one JSON line per precision: utterances/s and mel-frames/s per path and round.
"""
from __future__ import annotations

import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from fastspeech2_lightning_amd import data as D  # noqa: E402
from fastspeech2_lightning_amd.config import FastSpeech2Config, InferenceControl, Stats  # noqa: E402
from fastspeech2_lightning_amd.synthetic import DEFAULT_STATS, default_symbols, synthetic_lengths  # noqa: E402


def entries(n: int, seed: int = 1234) -> list:
    g = torch.Generator().manual_seed(seed)
    out = []
    for u, (n_tok, _) in enumerate(synthetic_lengths(n, seed=seed)):
        toks = [f"s{int(i):02d}" for i in torch.randint(0, 63, (n_tok,), generator=g)]
        out.append({"basename": f"utt{u:04d}", "characters": f"synthetic utterance {u:04d}", "character_tokens": "/".join(toks),
                    "speaker": "default", "language": "default", "is_last_input_chunk": True, "duration_control": 1.0})
    return out


def path_a(model, ds, batch_size, out_dir):
    w = D.SpecWriter(out_dir, model.output_key, 0)
    frames = 0
    for idx in D.synthesis_batches(ds.token_counts, batch_size, sort=False):
        batch = D.collate([ds[i] for i in idx], learn_alignment=model.config.model.learn_alignment)
        out = model.predict_step(batch)
        w.write(out, batch)
        frames += int(model.variance_adaptor.host_totals.sum())
    return frames


def path_new(sort):
    def run(model, ds, batch_size, out_dir):
        from fastspeech2_lightning_amd.synthesis import synthesize
        w = D.PackedSpecWriter(out_dir, model.output_key, 0, n_mels=model.config.preprocessing.audio.n_mels)
        return synthesize(model, ds, batch_size, InferenceControl(), w, sort=sort)["frames"]
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precisions", nargs="+", default=["32-true", "bf16-mixed"])
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from fastspeech2_lightning_amd.model import FastSpeech2
    paths = {"a_predict_step_spec_writer": path_a, "b_packed_no_sort": path_new(False), "c_packed_sorted": path_new(True)}
    tmp = Path(tempfile.mkdtemp(prefix="fs2l_synth_"))
    lines = []
    try:
        for precision in args.precisions:
            config = FastSpeech2Config(text=default_symbols(64))
            model = FastSpeech2(config, Stats(**DEFAULT_STATS), lang2id={"default": 0}, speaker2id={"default": 0}, seed=1234,
                                precision=precision)
            sd = model.state_dict()
            sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([1.79])  # exp(1.79) - 1 ~ 5 frames a token
            model.load_state_dict(sd)
            model.eval()
            ds = D.SynthesisDataset(entries(args.utterances), config, model.lang2id, model.speaker2id)
            rec = {"precision": precision, "utterances": len(ds), "batch": args.batch, "rounds": args.rounds, "paths": {}}
            for name, fn in paths.items():   # warm-up: every path over every batch shape
                fn(model, ds, args.batch, tmp / "warm")
                torch.cuda.synchronize()
                rec["paths"][name] = {"seconds": [], "utterances_per_s": [], "mel_frames_per_s": []}
            for r in range(args.rounds):
                for name, fn in paths.items():
                    out_dir = tmp / f"{precision}_{name}_{r}"
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    frames = fn(model, ds, args.batch, out_dir)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    p = rec["paths"][name]
                    p["seconds"].append(round(dt, 4))
                    p["utterances_per_s"].append(round(len(ds) / dt, 1))
                    p["mel_frames_per_s"].append(round(frames / dt, 0))
                    p["frames"] = frames
                    shutil.rmtree(out_dir, ignore_errors=True)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            if args.out is not None:  # (written as the run goes: a later precision's trouble does not lose this one)
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(lines) + "\n")
            del model
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
