"""CPU: the host side of ``fs2l synthesize --compare-to`` -- the numpy restatement of the DTW definition against an
exhaustive search, ``data.DtwWriter``'s order and fields, the command's refusals and what ``--dry-run`` reports, the
dataset's and ``synthesize``'s refusals, and the binding of the two entry points against the header."""
import csv
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from oracle import cases as C
from tests import dtw_references as R

REPO = Path(__file__).resolve().parent.parent


def _stub_checkpoint(path):
    """A checkpoint with everything but weights: what ``--dry-run`` reads."""
    cfg = C.small_config(learn_alignment=False)
    torch.save({"global_step": 3, "hyper_parameters": {"config": cfg.model_checkpoint_dump(), "stats": C.STATS,
                                                       "lang2id": dict(C.LANG2ID), "speaker2id": dict(C.SPEAKER2ID)}}, path)
    return path


@pytest.mark.parametrize("shape", R.all_shapes(4), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_reference_finds_the_cheapest_monotone_path(shape):
    """Every shape up to 4 x 4: the float64 recursion's total is the minimum over ALL monotone paths, and its step count is
    the length of one of the paths that reach it -- on real-valued costs (no ties) and on small integers (full of them)."""
    g = np.random.default_rng(100 * shape[0] + shape[1])
    for trial in range(12):
        cost = g.random(shape) if trial % 2 == 0 else g.integers(0, 3, shape).astype(np.float64)
        total, steps = R.dtw(cost)
        best, lengths = R.brute_force(cost)
        assert abs(total - best) <= 1e-12 * max(1.0, best), (cost, total, best)
        assert max(shape) <= steps <= shape[0] + shape[1] - 1
        if trial % 2 == 0:
            assert lengths == {steps}, (cost, steps, lengths)     # no ties: the cheapest path is unique
        else:
            assert steps in lengths, (cost, steps, lengths)


def test_the_tie_rule_by_hand():
    """All-equal costs: every cell ties, the diagonal is kept wherever it exists -> max(n, r) cells.  A cheaper row above
    beats the diagonal; up and left tying below the diagonal's cost: up is asked first and wins."""
    assert R.dtw(np.ones((3, 5))) == (5.0, 5)
    assert R.dtw(np.ones((5, 3))) == (5.0, 5)
    assert R.dtw(np.zeros((0, 4))) == (0.0, 0) and R.dtw(np.zeros((4, 0))) == (0.0, 0)
    # D = [[5, 6], [6, c + 5]]: diag 5 kept although up = left = 6
    assert R.dtw(np.array([[5.0, 1.0], [1.0, 2.0]])) == (7.0, 2)
    # D = [[1, 1], [1, .]]: diag 1, up 1, left 1 -> diagonal (2 cells); with diag 2 and up = left = 1: up, via (0, 1)
    total, steps = R.dtw(np.array([[2.0, -1.0], [-1.0, 0.0]]))
    assert (total, steps) == (1.0, 3)
    # the restatement in float32 repeats the kernel's rounding: a sum of three terms that float64 keeps apart
    c = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], dtype=np.float32)
    assert R.dtw(c, np.float32)[0] == np.float32(1.0) and R.dtw(c.astype(np.float64))[0] == 1.0 + 2.0 ** -23


def test_the_gpu_tests_inputs_leave_the_diagonal():
    """The batch tests/test_dtw_gpu.py runs: where both sequences are longer than one frame the cheapest path is longer than
    max(n, r), i.e. it takes up AND left moves beside the diagonal, in float32 and float64 alike; the float32 restatement
    stays inside the bounds the kernels are held to."""
    for idx, (n, r) in enumerate(R.LENGTHS):
        for channels in (80, 5):
            y, x = R.warped_pair(n, r, channels, idx)
            c32, c64 = R.frame_cost(y, x, np.float32), R.frame_cost(y, x)
            assert c32.dtype == np.float32 and c64.dtype == np.float64
            assert np.max(np.abs(c32 - c64) / c64) <= (channels + 3) * 2.0 ** -24
            (t32, s32), (t64, s64) = R.dtw(c32), R.dtw(c64)
            assert abs(float(t32) - t64) <= (n + r + channels) * 2.0 ** -23 * t64
            if min(n, r) > 1:
                assert s32 > max(n, r) and s64 > max(n, r), (n, r, s32, s64)
            else:
                assert s32 == s64 == max(n, r)


def _record(name, total, steps, frames=10, ref_frames=8):
    return dict(basename=name, speaker="spk0", language="l0", raw_text=f"text of {name}", total=total, steps=steps,
                frames=frames, ref_frames=ref_frames)


def test_dtw_writer_sorts_and_leaves_fields_empty(tmp_path):
    w = D.DtwWriter(tmp_path / "nested" / "dir", 41)
    assert w.path == tmp_path / "nested" / "dir" / "dtw-41.psv"
    w.add(3, _record("d", 6.0, 3))                        # 2.0, ties with b: input order keeps b first
    w.add(0, _record("a", 0.0, 0, frames=0))              # no path: empty mel_dtw, last
    w.add(4, _record("e", 10.0, 2, ref_frames=0))         # 5.0, but no frame ratio
    w.add(1, _record("b", 4.0, 2))                        # 2.0
    w.add(2, _record("c", 9.0, 3, frames=9, ref_frames=12))   # 3.0
    with pytest.raises(ValueError, match="twice"):
        w.add(1, _record("b", 4.0, 2))
    with pytest.raises(ValueError, match="steps"):
        w.add(9, dict(basename="x", total=1.0, frames=1, ref_frames=1))
    path = w.close()
    lines = path.read_text(encoding="utf8").splitlines()
    assert lines[0] == "|".join(D.DtwWriter.FIELDS) == (
        "basename|speaker|language|mel_dtw|total|steps|frames|ref_frames|frame_ratio|raw_text")
    assert [ln.split("|")[0] for ln in lines[1:]] == ["e", "c", "b", "d", "a"]
    with open(path, encoding="utf8", newline="") as f:
        rows = {r["basename"]: r for r in csv.DictReader(f, delimiter="|")}
    assert rows["a"]["mel_dtw"] == "" and rows["a"]["steps"] == "0" and rows["a"]["frame_ratio"] == "0.0"
    assert rows["e"]["frame_ratio"] == "" and rows["e"]["mel_dtw"] == "5.0" and rows["e"]["ref_frames"] == "0"
    assert rows["c"] == dict(basename="c", speaker="spk0", language="l0", mel_dtw="3.0", total="9.0", steps="3", frames="9",
                             ref_frames="12", frame_ratio="0.75", raw_text="text of c")
    # floats survive the file exactly
    w2 = D.DtwWriter(tmp_path, 0)
    x = float(torch.tensor(1 / 3, dtype=torch.float32))
    w2.add(0, _record("x", x, 7))
    with open(w2.close(), encoding="utf8", newline="") as f:
        row = list(csv.DictReader(f, delimiter="|"))[0]
    assert float(row["total"]) == x and float(row["mel_dtw"]) == x / 7


def test_the_command_refuses_what_cannot_be_compared(tmp_path, capsys):
    missing = tmp_path / "no_such.ckpt"      # never opened: the errors below are raised first
    with pytest.raises(SystemExit, match="teacher-forcing-directory"):
        cli.main(["synthesize", str(missing), "-f", "l.psv", "--compare-to", str(tmp_path), "-T", str(tmp_path)])
    with pytest.raises(SystemExit, match="basename"):
        cli.main(["synthesize", str(missing), "-t", "abc", "--compare-to", str(tmp_path)])
    with pytest.raises(SystemExit, match="--compare-to"):
        cli.main(["synthesize", str(missing), "-t", "abc", "--scores-only"])
    assert "Loading checkpoint" not in capsys.readouterr().err
    p = cli.build_parser()
    a = p.parse_args(["synthesize", "m.ckpt", "-f", "l.psv", "--compare-to", "dir", "--scores-only", "-b", "2"])
    assert a.compare_to == Path("dir") and a.scores_only and not a.return_scores
    assert p.parse_args(["synthesize", "m.ckpt", "-t", "abc"]).compare_to is None


def test_dry_run_lists_the_dtw_file(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    fl = tmp_path / "list.psv"
    fl.write_text("basename|language|speaker|characters\nu0|l0|spk0|abca\nu1|l0|spk0|ab\nu2|l0|spk0|bca\n", encoding="utf8")
    out = tmp_path / "out"
    argv = ["synthesize", str(ckpt), "-o", str(out), "-f", str(fl), "--dry-run"]
    assert cli.main(argv) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "dtw_file" not in plain and "compare_to" not in plain and plain["exact_lengths"] is False
    assert cli.main(argv + ["--compare-to", str(tmp_path / "corpus")]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["dtw_file"] == str(out / "dtw-3.psv") and rep["compare_to"] == str(tmp_path / "corpus")
    assert rep["exact_lengths"] is True                                       # a comparison forces exact lengths
    assert rep["files"] == plain["files"] and rep["batches"] == plain["batches"] and len(rep["files"]) == 3
    assert {k: v for k, v in rep.items() if k not in ("dtw_file", "compare_to", "exact_lengths")} == \
        {k: v for k, v in plain.items() if k != "exact_lengths"}
    assert cli.main(argv + ["--compare-to", str(tmp_path / "corpus"), "--scores-only"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["files"] == []
    assert not out.exists()                                                   # a dry run writes nothing


def test_the_dataset_attaches_the_recording(tmp_path):
    cfg = C.small_config(learn_alignment=False)
    audio = cfg.preprocessing.audio
    entries = [{"basename": "u0", "characters": "ab", "language": "l0", "speaker": "spk0"},
               {"basename": "u1", "characters": "abc", "language": "l0", "speaker": "spk0"}]
    with pytest.raises(ValueError, match="teacher_forcing_dir"):
        D.SynthesisDataset(entries, cfg, C.LANG2ID, C.SPEAKER2ID, teacher_forcing_dir=tmp_path, compare_dir=tmp_path)
    ds = D.SynthesisDataset(entries, cfg, C.LANG2ID, C.SPEAKER2ID, compare_dir=tmp_path)
    assert ds.compare_dir == tmp_path and not ds.teacher_forcing
    with pytest.raises(FileNotFoundError, match="'u0'"):
        ds[0]
    mels = [torch.randn(audio.n_mels, 7), torch.randn(audio.n_mels, 4)]
    for e, m in zip(entries, mels):
        p = D.feature_path(tmp_path, "spec", e["basename"], "spk0", "l0", f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt")
        p.parent.mkdir(exist_ok=True)
        torch.save(m, p)
    item = ds[0]
    assert torch.equal(item["compare_mel"], mels[0].T) and item["mel"] is None
    assert list(item)[:-1] == list(D.SynthesisDataset(entries, cfg, C.LANG2ID, C.SPEAKER2ID)[0])   # the usual keys, in order
    from fastspeech2_lightning_amd.synthesis import collate_items
    batch = collate_items([ds[0], ds[1]], learn_alignment=False)
    assert batch["compare_mel"].shape == (2, 7, audio.n_mels) and batch["compare_lens"].tolist() == [7, 4]
    assert batch["compare_lens"].dtype == torch.int32
    assert torch.equal(batch["compare_mel"][1, :4], mels[1].T) and not batch["compare_mel"][1, 4:].any()
    assert "compare_lens" not in collate_items([D.SynthesisDataset(entries, cfg, C.LANG2ID, C.SPEAKER2ID)[0]], False)


def test_the_new_arguments_and_the_binding():
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthesis import _Slot, synthesize
    assert inspect.signature(synthesize).parameters["compare"].default is None
    assert list(inspect.signature(FastSpeech2.mel_dtw).parameters) == ["self", "output", "ref", "ref_lens", "out"]
    assert list(inspect.signature(hip.frame_dist).parameters) == ["a", "a_lens", "b", "b_lens", "out"]
    assert list(inspect.signature(hip.dtw).parameters) == ["cost", "lens1", "lens2", "total", "steps"]
    assert hip.SIGNATURES["fs2hip_frame_dist"] == "pppppiiiip" and hip.SIGNATURES["fs2hip_dtw"] == "pppppiiip"
    text = (REPO / "include" / "fs2hip.h").read_text()
    assert int(re.search(r"#define FS2_DTW_MAX_T1 (\d+)", text).group(1)) == hip.DTW_MAX_T1
    assert int(re.search(r"#define FS2_FRAME_DIST_MAX_C (\d+)", text).group(1)) == hip.FRAME_DIST_MAX_C
    # both limits are what 64 KiB of LDS holds
    assert (64 * 64 + 2 * hip.DTW_MAX_T1) * 4 == 64 * 1024
    assert (16 * hip.FRAME_DIST_MAX_C + 64 * (hip.FRAME_DIST_MAX_C + 1)) * 4 <= 64 * 1024 < (16 * 205 + 64 * 206) * 4
    inc = (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    assert "fs2hip_frame_dist(" in inc and "fs2hip_dtw(" in inc
    # the header of a slot: without a comparison not one float more, with it 2 * B rounded up to 16 bytes at the end
    for B in (1, 2, 3, 4, 5):
        assert _Slot.header(B, False, 0, False) == _Slot.header(B) == _Slot.table(B)
        assert _Slot.header(B, False, 3, True) - _Slot.header(B, False, 3) == _Slot.dtw_table(B) >= 2 * B
        assert _Slot.dtw_table(B) % 4 == 0 and _Slot.dtw_table(B) < 2 * B + 4
