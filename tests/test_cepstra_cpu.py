"""CPU: the cepstral distance's host side -- the DCT table and the numpy restatement of ``fs2hip_cepstra``
(tests/cepstra_references.py), ``data.synthesis_metrics``, ``data.DtwWriter(..., cepstra=K)``, and the command lines of ``fs2l
synthesize --cepstra`` and ``fs2l train --val-synthesis / --val-cepstra / --monitor``.

Bounds.  The fp32 restatement against float64: a sum of C products accumulated in order has an absolute error of at most
C * 2^-24 * sum_m |x_m * table_km| (C - 1 additions and one product rounding per term, each at most 2^-24 relative to a
partial sum that the sum of absolute products bounds; second-order terms are below the slack of counting C and not C - 1
+ 1 roundings at full weight).  The table's rows are orthonormal to fp32 rounding: ``table @ table.T`` is the identity to
1e-6 (C entries of at most 2^-24 * sqrt(2 / C) relative error each).  A projection on orthonormal rows does not lengthen a
vector, so ``||cepstra(a) - cepstra(b)|| <= ||a - b||`` up to that rounding: every cepstral frame cost is at most the mel
cost, which is what lets the DTW tests' bounds carry over."""
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests import cepstra_references as R

REPO = Path(__file__).resolve().parent.parent
PAIRS = ((80, 13), (80, 64), (5, 4), (16, 13))


@pytest.mark.parametrize("channels,K", PAIRS)
def test_the_table_is_orthonormal_and_is_the_bindings(channels, K):
    from fastspeech2_lightning_amd import hip
    tab = R.table(channels, K)
    assert tab.dtype == np.float32 and tab.shape == (K, channels)
    gram = tab.astype(np.float64) @ tab.astype(np.float64).T
    assert np.max(np.abs(gram - np.eye(K))) <= 1e-6
    # c0 is dropped: every row sums to zero against a constant frame
    assert np.max(np.abs(tab.astype(np.float64).sum(axis=1))) <= 1e-5
    mine = hip.dct_table_host(channels, K)
    assert mine.dtype == torch.float32 and mine.numpy().tobytes() == tab.tobytes()


@pytest.mark.parametrize("channels,K", PAIRS)
def test_the_fp32_restatement_meets_the_summation_bound(channels, K):
    tab = R.table(channels, K)
    x = R.mel_like(200, channels, seed=channels + K)
    got, want = R.cepstra32(x, tab), R.cepstra64(x, tab)
    assert got.dtype == np.float32 and got.shape == (200, K)
    unit = 2.0 ** -24 * R.abs_product64(x, tab)
    used = np.max(np.abs(got.astype(np.float64) - want) / unit)
    print(f"C = {channels}, K = {K}: the restatement uses {used:.2f} of the {channels} units of the bound")
    assert used <= channels


@pytest.mark.parametrize("channels,K", PAIRS)
def test_the_projection_is_a_contraction(channels, K):
    tab = R.table(channels, K)
    a, b = R.mel_like(150, channels, seed=1), R.mel_like(150, channels, seed=2)
    ca, cb = R.cepstra64(a, tab), R.cepstra64(b, tab)
    lhs = np.linalg.norm(ca - cb, axis=1)
    rhs = np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=1)
    assert (lhs <= rhs * (1 + 1e-6)).all()
    assert (lhs < 0.9 * rhs).any()           # and it really drops something (c0 and the high coefficients)


def test_the_binding_and_the_header_agree():
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthesis import _Slot
    text = (REPO / "include" / "fs2hip.h").read_text()
    assert int(re.search(r"#define FS2_CEPSTRA_MAX_K (\d+)", text).group(1)) == hip.CEPSTRA_MAX_K == 64
    assert hip.SIGNATURES["fs2hip_cepstra"] == "ppppiiiip"
    assert list(inspect.signature(hip.cepstra).parameters) == ["x", "lens", "K", "out"]
    assert "fs2hip_cepstra(" in (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    # ``cepstra=K`` is a keyword-only option of both methods; their published parameter list is what it was
    for fn in (FastSpeech2.mel_dtw, FastSpeech2.mel_dtw_paths):
        assert list(inspect.signature(fn).parameters) == ["self", "output", "ref", "ref_lens", "out"]
        assert "cepstra" in inspect.signature(fn, follow_wrapped=False).parameters
        with pytest.raises(TypeError):
            fn(None, None, None, None, None, 13)                               # not positional
    assert inspect.signature(D.validate).parameters["synthesis"].default is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.cepstra(torch.zeros(1, 4, 8), torch.ones(1, dtype=torch.int32), 3)
    for bad in ((80, 0), (80, 65), (5, 5), (205, 13)):
        with pytest.raises(ValueError, match="dct_table"):
            hip.dct_table_host(*bad)
    # the slot header: 2 * B values as ever, 4 * B only with a cepstral distance
    for B in (1, 2, 3, 5):
        assert _Slot.dtw_table(B) == _Slot.dtw_table(B, False) == -(-2 * B // 4) * 4
        assert _Slot.dtw_table(B, True) == -(-4 * B // 4) * 4
        assert _Slot.header(B, False, 3, True, True) - _Slot.header(B, False, 3) == _Slot.dtw_table(B, True) >= 4 * B
        assert _Slot.header(B, False, 3, True, False) == _Slot.header(B, False, 3, True)


def test_synthesis_metrics_on_hand_made_arrays():
    m, sums = D.synthesis_metrics(total=[6.0, 0.0, 10.0, 9.0], steps=[3, 0, 4, 2], frames=[10, 0, 12, 8],
                                  ref_frames=[8, 5, 12, 10])
    assert m == {"validation/mel_dtw": (2.0 + 2.5 + 4.5) / 3, "validation/frame_ratio": 30 / 35,
                 "validation/synth_scored": 3, "validation/synth_empty": 1}
    assert list(m) == ["validation/mel_dtw", "validation/frame_ratio", "validation/synth_scored", "validation/synth_empty"]
    assert sums == [9.0, 0.0, 3.0, 1.0, 30.0, 35.0] and len(sums) == len(D.SYNTHESIS_SUMS) == 6
    m, sums = D.synthesis_metrics([6.0, 0.0, 10.0, 9.0], [3, 0, 4, 2], [10, 0, 12, 8], [8, 5, 12, 10],
                                  cep_total=[3.0, 0.0, 2.0, 1.0], cep_steps=[4, 0, 4, 2])
    assert m["validation/cep_dtw"] == (0.75 + 0.5 + 0.5) / 3 and m["validation/mel_dtw"] == 3.0
    assert list(m) == ["validation/mel_dtw", "validation/cep_dtw", "validation/frame_ratio", "validation/synth_scored",
                       "validation/synth_empty"]
    assert sums == [9.0, 1.75, 3.0, 1.0, 30.0, 35.0]
    # the sums of two ranks add up to the metrics of the whole set
    _, first = D.synthesis_metrics([6.0, 0.0], [3, 0], [10, 0], [8, 5], [3.0, 0.0], [4, 0])
    _, second = D.synthesis_metrics([10.0, 9.0], [4, 2], [12, 8], [12, 10], [2.0, 1.0], [4, 2])
    assert D.synthesis_metrics_from_sums([a + b for a, b in zip(first, second)], True) == m
    # every utterance empty: counted, nothing averaged, every value finite
    m, sums = D.synthesis_metrics([0.0, 0.0], [0, 0], [0, 0], [7, 9], [0.0, 0.0], [0, 0])
    assert m == {"validation/mel_dtw": 0.0, "validation/cep_dtw": 0.0, "validation/frame_ratio": 0.0,
                 "validation/synth_scored": 0, "validation/synth_empty": 2}
    assert sums == [0.0, 0.0, 0.0, 2.0, 0.0, 16.0]
    m, _ = D.synthesis_metrics([], [], [], [])
    assert m["validation/synth_scored"] == 0 and m["validation/frame_ratio"] == 0.0
    # float32 inputs are taken in float64
    t = np.array([1 / 3, 0.1], dtype=np.float32)
    m, _ = D.synthesis_metrics(t, np.array([3, 7], dtype=np.int32), [1, 1], [1, 1])
    assert m["validation/mel_dtw"] == (float(t[0]) / 3 + float(t[1]) / 7) / 2
    with pytest.raises(ValueError, match="length"):
        D.synthesis_metrics([1.0], [1, 2], [1], [1])
    with pytest.raises(ValueError, match="disagree"):
        D.synthesis_metrics([1.0], [1], [1], [1], [1.0], [0])


def _record(name, total, steps, frames=10, ref_frames=8, **more):
    return dict(basename=name, speaker="spk0", language="l0", raw_text=f"text of {name}", total=total, steps=steps,
                frames=frames, ref_frames=ref_frames, **more)


def test_dtw_writer_with_and_without_cepstra(tmp_path):
    plain = D.DtwWriter(tmp_path / "plain", 7)
    plain.add(1, _record("b", 4.0, 2))
    plain.add(0, _record("a", 0.0, 0, frames=0))
    plain.add(2, _record("c", 9.0, 3, frames=9, ref_frames=12))
    assert plain.cepstra is None and plain.fields == D.DtwWriter.FIELDS
    assert plain.close().read_bytes() == (
        b"basename|speaker|language|mel_dtw|total|steps|frames|ref_frames|frame_ratio|raw_text\n"
        b"c|spk0|l0|3.0|9.0|3|9|12|0.75|text of c\n"
        b"b|spk0|l0|2.0|4.0|2|10|8|1.25|text of b\n"
        b"a|spk0|l0||0.0|0|0|8|0.0|text of a\n")
    # records that carry cepstral values do not change a file that was not asked for them
    extra = D.DtwWriter(tmp_path / "extra", 7)
    extra.add(1, _record("b", 4.0, 2, cep_total=3.0, cep_steps=4))
    extra.add(0, _record("a", 0.0, 0, frames=0, cep_total=0.0, cep_steps=0))
    extra.add(2, _record("c", 9.0, 3, frames=9, ref_frames=12, cep_total=1.5, cep_steps=3))
    assert extra.close().read_bytes() == plain.path.read_bytes()
    cep = D.DtwWriter(tmp_path / "cep", 7, cepstra=13)
    assert cep.cepstra == 13 and D.DtwWriter.FIELDS == plain.fields          # the class attribute is what it was
    assert cep.fields == ("basename", "speaker", "language", "mel_dtw", "total", "steps", "cep_dtw", "cep_total", "cep_steps",
                          "frames", "ref_frames", "frame_ratio", "raw_text")
    cep.add(1, _record("b", 4.0, 2, cep_total=3.0, cep_steps=4))              # the smaller mel_dtw, the larger cep_dtw
    cep.add(0, _record("a", 0.0, 0, frames=0, cep_total=0.0, cep_steps=0))
    cep.add(2, _record("c", 9.0, 3, frames=9, ref_frames=12, cep_total=1.5, cep_steps=3))
    with pytest.raises(ValueError, match="cep_total"):
        cep.add(5, _record("x", 1.0, 1))
    assert cep.close().read_bytes() == (
        b"basename|speaker|language|mel_dtw|total|steps|cep_dtw|cep_total|cep_steps|frames|ref_frames|frame_ratio|raw_text\n"
        b"c|spk0|l0|3.0|9.0|3|0.5|1.5|3|9|12|0.75|text of c\n"                # sorted by mel_dtw, not by cep_dtw
        b"b|spk0|l0|2.0|4.0|2|0.75|3.0|4|10|8|1.25|text of b\n"
        b"a|spk0|l0||0.0|0||0.0|0|0|8|0.0|text of a\n")


def test_the_commands_refuse_what_cannot_work(tmp_path, capsys):
    missing = tmp_path / "no_such.ckpt"      # never opened: the error is raised first
    with pytest.raises(SystemExit, match="--cepstra goes with --compare-to"):
        cli.main(["synthesize", str(missing), "-f", "l.psv", "--cepstra", "13"])
    assert "Loading checkpoint" not in capsys.readouterr().err
    p = cli.build_parser()
    a = p.parse_args(["synthesize", "m.ckpt", "-f", "l.psv", "--compare-to", "dir", "--cepstra", "13"])
    assert a.cepstra == 13 and p.parse_args(["synthesize", "m.ckpt", "-t", "abc"]).cepstra is None
    t = p.parse_args(["train", "c.yaml"])
    assert t.monitor == "validation/total_loss" == cli.MONITOR and t.val_synthesis is False and t.val_cepstra is None
    from tests.test_cli_cpu import make_project
    cfg = make_project(tmp_path)
    with pytest.raises(SystemExit, match="--monitor validation/nonsense"):
        cli.main(["train", str(cfg), "--dry-run", "--monitor", "validation/nonsense"])
    with pytest.raises(SystemExit, match="needs --val-synthesis"):
        cli.main(["train", str(cfg), "--dry-run", "--monitor", "validation/mel_dtw"])
    with pytest.raises(SystemExit, match="--monitor validation/cep_dtw"):
        cli.main(["train", str(cfg), "--dry-run", "--val-synthesis", "--monitor", "validation/cep_dtw"])
    with pytest.raises(SystemExit, match="--monitor validation/attn_ctc_loss"):       # the model has no aligner
        cli.main(["train", str(cfg), "--dry-run", "--monitor", "validation/attn_ctc_loss"])
    with pytest.raises(SystemExit, match="--val-cepstra goes with --val-synthesis"):
        cli.main(["train", str(cfg), "--dry-run", "--val-cepstra", "13"])
    with pytest.raises(SystemExit, match="--val-cepstra 16"):                         # n_mels = 16: at most 15
        cli.main(["train", str(cfg), "--dry-run", "--val-synthesis", "--val-cepstra", "16"])
    with pytest.raises(SystemExit, match="max_length"):
        cli.main(["train", str(cfg), "--dry-run", "--val-synthesis", "-c", "model.max_length=7000"])
    capsys.readouterr()


def test_the_dry_run_prints_the_new_settings(tmp_path, capsys):
    from tests.test_cli_cpu import make_project
    cfg = make_project(tmp_path)
    assert cli.main(["train", str(cfg), "--dry-run"]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain["monitor"] == "validation/total_loss" and "val_synthesis" not in plain and "val_cepstra" not in plain
    assert cli.main(["train", str(cfg), "--dry-run", "--val-synthesis", "--val-cepstra", "13", "--monitor",
                     "validation/cep_dtw"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["monitor"] == "validation/cep_dtw" and rep["val_synthesis"] is True and rep["val_cepstra"] == 13
    assert {k: v for k, v in rep.items() if k not in ("monitor", "val_synthesis", "val_cepstra")} == \
        {k: v for k, v in plain.items() if k != "monitor"}
    assert list(plain) == [k for k in rep if k not in ("val_synthesis", "val_cepstra")]      # the old keys, in the old order
    assert cli.main(["train", str(cfg), "--dry-run", "--val-synthesis", "--monitor", "validation/mel_dtw"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["monitor"] == "validation/mel_dtw" and rep["val_synthesis"] is True and rep["val_cepstra"] is None
    assert cli.main(["train", str(cfg), "--dry-run", "--monitor", "validation/spec_loss"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["monitor"] == "validation/spec_loss"


def test_the_synthesize_dry_run_names_the_coefficients(tmp_path, capsys):
    from tests.test_dtw_cpu import _stub_checkpoint
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    fl = tmp_path / "list.psv"
    fl.write_text("basename|language|speaker|characters\nu0|l0|spk0|abca\nu1|l0|spk0|ab\n", encoding="utf8")
    argv = ["synthesize", str(ckpt), "-o", str(tmp_path / "out"), "-f", str(fl), "--dry-run", "--compare-to",
            str(tmp_path / "corpus")]
    assert cli.main(argv) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "cepstra" not in plain
    assert cli.main(argv + ["--cepstra", "13"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep.pop("cepstra") == 13 and rep == plain
    with pytest.raises(SystemExit, match="--cepstra 16"):       # the stub model has 16 mel bins
        cli.main(argv + ["--cepstra", "16"])
