"""GPU: ``fs2l train --val-synthesis [--val-cepstra K] [--monitor KEY]`` on the synthetic project of tests/test_cli_cpu.py
(10 training and 3 validation utterances, batch 4: 3 steps per epoch).

Two runs of 6 steps that validate every 2 steps, one plain and one with the flags: the flags must not move a training step
by a bit (losses, learning rate, gradient norm ``==``; final weights equal tensor for tensor), every validation record of the
second carries the five free-synthesis metrics, ``data.validate`` on ``last.ckpt`` in this process reproduces the last record
exactly, and the frame counts behind it are those of ``fs2l synthesize --compare-to`` on the same checkpoint and filelist
(integers: exact lengths make an utterance's frame count independent of its batch).  ``best.ckpt`` follows ``--monitor``."""
import csv
import json

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests.test_cli_cpu import make_project

pytestmark = pytest.mark.gpu

NEW_KEYS = ("validation/mel_dtw", "validation/cep_dtw", "validation/frame_ratio", "validation/synth_scored",
            "validation/synth_empty")
FLAGS = ("--val-synthesis", "--val-cepstra", "13", "--monitor", "validation/mel_dtw")
_CACHE = {}


def _run(cfg, out, *extra):
    args = ["train", str(cfg), "--output-dir", str(out), "--log-every", "1", "--devices", "1", *extra]
    assert cli.main(args) == 0
    recs = [json.loads(line) for line in (out / "metrics.jsonl").read_text().splitlines()]
    train = {r["step"]: r for r in recs if "training/total_loss" in r}
    val = [r for r in recs if "validation/total_loss" in r]
    return train, val


def _runs(tmp_path_factory):
    """The two runs, once: (root, config, plain (train, val), flagged (train, val))."""
    if "runs" not in _CACHE:
        root = tmp_path_factory.mktemp("val_synthesis")
        cfg = make_project(root, n_train=10, n_val=3, write_features=True)
        plain = _run(cfg, root / "plain", "--max-steps", "6", "--val-every", "2")
        flagged = _run(cfg, root / "flagged", "--max-steps", "6", "--val-every", "2", *FLAGS)
        _CACHE["runs"] = (root, cfg, plain, flagged)
    return _CACHE["runs"]


def _ckpt(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_the_flags_do_not_move_a_training_step(tmp_path_factory):
    root, _, (plain, plain_val), (flagged, flagged_val) = _runs(tmp_path_factory)
    assert sorted(plain) == sorted(flagged) == [1, 2, 3, 4, 5, 6]
    for step in range(1, 7):
        for key in ("training/total_loss", "lr", "grad_norm"):
            assert plain[step][key] == flagged[step][key], (step, key, plain[step][key], flagged[step][key])
    a, b = _ckpt(root / "plain" / "checkpoints" / "last.ckpt"), _ckpt(root / "flagged" / "checkpoints" / "last.ckpt")
    assert list(a["state_dict"]) == list(b["state_dict"])
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    # the teacher-forced losses of the validations are the same numbers too, and a plain run's records and checkpoints
    # carry nothing new
    assert len(plain_val) == len(flagged_val) == 3
    for p, f in zip(plain_val, flagged_val):
        assert not set(NEW_KEYS) & set(p)
        assert {k: v for k, v in f.items() if k not in NEW_KEYS + ("time",)} == {k: v for k, v in p.items() if k != "time"}
    assert "fs2l_monitor" not in a and b["fs2l_monitor"] == "validation/mel_dtw"


def test_every_validation_record_carries_the_metrics(tmp_path_factory):
    _, _, _, (_, val) = _runs(tmp_path_factory)
    assert [v["step"] for v in val] == [2, 4, 6]
    for v in val:
        print({k: v[k] for k in NEW_KEYS})
        for k in NEW_KEYS:
            assert k in v and v[k] == v[k] and abs(v[k]) < float("inf"), (k, v)
        assert v["validation/synth_scored"] + v["validation/synth_empty"] == 3
        assert v["validation/frame_ratio"] >= 0
        if v["validation/synth_scored"] > 0:
            assert v["validation/mel_dtw"] > 0 and v["validation/cep_dtw"] > 0
            assert v["validation/cep_dtw"] <= v["validation/mel_dtw"] * (1 + 1e-5)
        else:
            assert v["validation/mel_dtw"] == 0.0 and v["validation/cep_dtw"] == 0.0 and v["validation/frame_ratio"] == 0.0


def test_validate_in_process_reproduces_the_last_record_and_synthesize_its_frames(tmp_path_factory, tmp_path):
    root, cfg, _, (_, val) = _runs(tmp_path_factory)
    last = root / "flagged" / "checkpoints" / "last.ckpt"
    args = cli.build_parser().parse_args(["train", str(cfg), "--output-dir", str(tmp_path / "again"), "--devices", "1",
                                          "--resume", str(last)])
    trainer = cli.Trainer(args, cli.plan(args), 0, 1, 0)
    trainer.metrics.close()
    opts = D.SynthesisValidation(cepstra=13)
    got = D.validate(trainer.model, trainer.batches(trainer.val_set, False, 0, 0), synthesis=opts)
    want = {k: v for k, v in val[-1].items() if k.startswith("validation/")}
    assert val[-1]["step"] == 6 and got == want, (got, want)
    assert list(got)[-5:] == list(NEW_KEYS)                                       # behind the losses, in the documented order
    without = D.validate(trainer.model, trainer.batches(trainer.val_set, False, 0, 0))
    assert without == {k: v for k, v in want.items() if k not in NEW_KEYS}
    assert trainer.model.training                                                 # left as it was found
    # the frame counts: those of the command on the same checkpoint and filelist
    out = tmp_path / "synth"
    pre = cfg.parent / "preprocessed"
    assert cli.main(["synthesize", str(last), "-f", str(pre / "validation_filelist.psv"), "--compare-to", str(pre),
                     "-o", str(out), "--scores-only", "--cepstra", "13"]) == 0
    with open(out / "dtw-6.psv", encoding="utf8", newline="") as f:
        rows = list(csv.DictReader(f, delimiter="|"))
    assert len(rows) == 3
    frames, ref_frames = sum(int(r["frames"]) for r in rows), sum(int(r["ref_frames"]) for r in rows)
    scored = sum(1 for r in rows if int(r["steps"]) > 0)
    print("sums of the pass", dict(zip(D.SYNTHESIS_SUMS, opts.sums)), "frames", frames, "ref_frames", ref_frames)
    assert opts.sums[4] == frames and opts.sums[5] == ref_frames and ref_frames > 0
    assert opts.sums[2] == scored == got["validation/synth_scored"] and opts.sums[3] == 3 - scored
    assert got["validation/frame_ratio"] == frames / ref_frames


def test_best_follows_the_monitor_and_starts_over_under_another(tmp_path_factory):
    root, cfg, _, (_, val) = _runs(tmp_path_factory)
    ckpts = root / "flagged" / "checkpoints"
    scored = [v for v in val if v["validation/synth_scored"] > 0]
    print([(v["step"], v["validation/mel_dtw"], v["validation/synth_scored"]) for v in val])
    if scored:
        best = min(scored, key=lambda v: (v["validation/mel_dtw"], v["step"]))   # strict <: the first of equals stays
        ck = _ckpt(ckpts / "best.ckpt")
        assert ck["global_step"] == best["step"] and ck["fs2l_best_monitor"] == best["validation/mel_dtw"]
        assert ck["fs2l_monitor"] == "validation/mel_dtw"
    else:
        assert not (ckpts / "best.ckpt").exists()        # a mean over no utterance never selects a checkpoint
    # resumed under the default monitor: best starts over, so the first validation of the resumed run becomes best
    train, val2 = _run(cfg, root / "flagged", "--max-steps", "8", "--val-every", "2")
    assert sorted(train)[-1] == 8
    ck = _ckpt(ckpts / "best.ckpt")
    resumed = [v for v in val2 if v["step"] > 6]
    assert [v["step"] for v in resumed] == [8] and not set(NEW_KEYS) & set(resumed[0])
    assert ck["global_step"] == 8 and ck["fs2l_best_monitor"] == resumed[0]["validation/total_loss"]
    assert "fs2l_monitor" not in ck
