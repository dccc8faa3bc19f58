"""CPU: the host side of per-utterance scoring -- ``data.coverage_scores`` against values worked out by hand,
``data.ScoreWriter``'s order and columns, the argument errors of ``fs2l synthesize --return-scores`` and what ``--dry-run``
reports, and the binding of ``fs2hip_utterance_losses`` against the header."""
import csv
import inspect
import json
import re
from pathlib import Path

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from oracle import cases as C

REPO = Path(__file__).resolve().parent.parent


def _stub_checkpoint(path):
    """A checkpoint with everything but weights: what ``--dry-run`` reads."""
    cfg = C.small_config(learn_alignment=False)
    torch.save({"global_step": 3, "hyper_parameters": {"config": cfg.model_checkpoint_dump(), "stats": C.STATS,
                                                       "lang2id": dict(C.LANG2ID), "speaker2id": dict(C.SPEAKER2ID)}}, path)
    return path


# Three entries over the tokens 1, 2, 3.  Token counts: 1 -> 4, 2 -> 3, 3 -> 2.  Trigrams of the framed entries:
#   <BOS> 1 2 3 1 <EOS>: (B,1,2) (1,2,3) (2,3,1) (3,1,E)
#   <BOS> 1 2 <EOS>:     (B,1,2) (1,2,E)
#   <BOS> 2 3 1 <EOS>:   (B,2,3) (2,3,1) (3,1,E)
# so (1,2,3) occurs once and (2,3,1) twice; an entry's own trigrams leave the boundary symbols out.
TOKENS = [[1, 2, 3, 1], [1, 2], [2, 3, 1]]
PHONE = [1 / 4 + 1 / 3 + 1 / 2 + 1 / 4, 1 / 4 + 1 / 3, 1 / 3 + 1 / 2 + 1 / 4]
TRIGRAM = [1 / 1 + 1 / 2, 0, 1 / 2]


def test_coverage_scores_by_hand():
    got = D.coverage_scores(TOKENS)
    assert [set(g) for g in got] == [{"phone_coverage_score", "trigram_coverage_score"}] * 3
    assert [g["phone_coverage_score"] for g in got] == pytest.approx(PHONE, rel=1e-12)
    assert [g["trigram_coverage_score"] for g in got] == pytest.approx(TRIGRAM, rel=1e-12)
    assert got[1]["trigram_coverage_score"] == 0                      # two tokens: no trigram of its own
    # the ids as SynthesisDataset.tokens holds them (int32 tensors), and strings, count the same way
    assert D.coverage_scores([torch.IntTensor(t) for t in TOKENS]) == got
    assert D.coverage_scores([[str(t) for t in ts] for ts in TOKENS]) == got
    # one entry of three distinct tokens: every count is 1, and its only inner trigram is the three of them
    assert D.coverage_scores([[1, 2, 3]]) == [{"phone_coverage_score": 3.0, "trigram_coverage_score": 1.0}]
    assert D.coverage_scores([]) == []
    assert "dropped" in D.coverage_scores.__doc__                     # unknown symbols: said where the reader looks


def _record(name, total, tri, **terms):
    return dict(basename=name, speaker="spk0", language="l0", raw_text=f"text of {name}", total=total,
                trigram_coverage_score=tri, phone_coverage_score=1.5, **terms)


def test_score_writer_sorts_and_orders_the_fields(tmp_path):
    w = D.ScoreWriter(tmp_path / "nested" / "dir", 41)
    assert w.path == tmp_path / "nested" / "dir" / "scores-41.psv"
    # delivered out of input order; b and c tie on the total (c has the smaller trigram score), d and e tie on both
    w.add(3, _record("d", 1.0, 0.5, duration=0.25, spec=0.5, postnet=0.25))
    w.add(0, _record("a", 2.0, 9.0, duration=1.0, spec=0.5, postnet=0.5, pitch=7.0))
    w.add(2, _record("c", 3.0, 0.1, duration=1.0, spec=1.0, postnet=1.0, attn_ctc=0.0, attn_bin=0.0))
    w.add(4, _record("e", 1.0, 0.5, duration=0.25, spec=0.5, postnet=0.25))
    w.add(1, _record("b", 3.0, 0.2, duration=1.0, spec=1.0, postnet=1.0))
    with pytest.raises(ValueError, match="twice"):
        w.add(1, _record("b", 3.0, 0.2))
    with pytest.raises(ValueError, match="total"):
        w.add(9, dict(basename="x", trigram_coverage_score=0.0))
    path = w.close()
    lines = path.read_text(encoding="utf8").splitlines()
    assert lines[0] == ("basename|speaker|language|total|trigram_coverage_score|duration|spec|postnet|attn_ctc|attn_bin|"
                        "raw_text|phone_coverage_score")
    assert [ln.split("|")[0] for ln in lines[1:]] == ["c", "b", "a", "d", "e"]
    with open(path, encoding="utf8", newline="") as f:
        rows = list(csv.DictReader(f, delimiter="|"))
    assert rows[0]["attn_ctc"] == "0.0" and rows[0]["attn_bin"] == "0.0"
    assert rows[1]["attn_ctc"] == "" and rows[1]["attn_bin"] == ""        # an absent term is an empty field
    assert "pitch" not in rows[2] and float(rows[2]["total"]) == 2.0       # not a column of the reference's file
    assert rows[2]["raw_text"] == "text of a" and float(rows[2]["phone_coverage_score"]) == 1.5
    assert float(rows[3]["spec"]) == 0.5
    # floats survive the file exactly
    w2 = D.ScoreWriter(tmp_path, 0)
    x = float(torch.tensor(1 / 3, dtype=torch.float32))
    w2.add(0, _record("x", x, 0.0, spec=x))
    with open(w2.close(), encoding="utf8", newline="") as f:
        assert float(list(csv.DictReader(f, delimiter="|"))[0]["total"]) == x


def test_argument_errors_come_before_the_checkpoint(tmp_path, capsys):
    missing = tmp_path / "no_such.ckpt"      # never opened: the errors below are raised first
    with pytest.raises(SystemExit, match="teacher-forcing-directory"):
        cli.main(["synthesize", str(missing), "-t", "abc", "--return-scores"])
    with pytest.raises(SystemExit, match="--return-scores"):
        cli.main(["synthesize", str(missing), "-t", "abc", "-T", str(tmp_path), "--scores-only"])
    assert "Loading checkpoint" not in capsys.readouterr().err
    a = cli.build_parser().parse_args(["synthesize", "m.ckpt", "-f", "l.psv", "-T", "dir", "--return-scores", "--scores-only"])
    assert a.return_scores and a.scores_only
    b = cli.build_parser().parse_args(["synthesize", "m.ckpt", "-t", "abc"])
    assert b.return_scores is False and b.scores_only is False


def test_dry_run_reports_the_scores(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    out = tmp_path / "out"
    argv = ["synthesize", str(ckpt), "-o", str(out), "-T", str(tmp_path / "corpus"), "-t", "abca", "-t", "ab", "-t", "bca",
            "--dry-run"]
    assert cli.main(argv) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain["return_scores"] is False and "scores_file" not in plain and plain["exact_lengths"] is False
    assert "trigram_coverage_score" not in plain["entries"][0] and len(plain["files"]) == 3
    assert cli.main(argv + ["--return-scores"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["return_scores"] is True and rep["exact_lengths"] is True       # scoring forces exact lengths
    assert rep["scores_file"] == str(out / "scores-3.psv")
    assert [e["phone_coverage_score"] for e in rep["entries"]] == pytest.approx(PHONE, rel=1e-12)
    assert [e["trigram_coverage_score"] for e in rep["entries"]] == pytest.approx(TRIGRAM, rel=1e-12)
    assert rep["files"] == plain["files"] and rep["batches"] == plain["batches"]
    assert cli.main(argv + ["--return-scores", "--scores-only"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["files"] == []
    assert not out.exists()                                                     # a dry run writes nothing


def test_synthesize_and_the_model_take_the_new_arguments():
    from fastspeech2_lightning_amd.model import LOSS_KEYS, FastSpeech2
    from fastspeech2_lightning_amd.synthesis import synthesize
    assert inspect.signature(synthesize).parameters["scores"].default is None
    p = inspect.signature(FastSpeech2.utterance_losses).parameters
    assert list(p)[:4] == ["self", "output", "batch", "current_epoch"] and p["current_epoch"].default == 0
    from fastspeech2_lightning_amd import hip
    assert hip.SCORE_COLUMNS == LOSS_KEYS + ("total",)
    assert inspect.signature(hip.attn_ctc_loss).parameters["nll_out"].default is None


def test_binding_matches_the_header_prototype():
    from fastspeech2_lightning_amd import hip
    assert "fs2hip_utterance_losses" in hip.EXPORTS
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fs2hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+fs2hip_utterance_losses\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/fs2hip.h does not declare fs2hip_utterance_losses"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const Fs2ScoreMember* members", "int n", "const float* soft", "const int* hard_idx",
                    "const int* mel_lens", "int Tm", "int Ts", "float bin_weight", "const float* nll", "float ctc_weight",
                    "float* scores", "int B", "void* stream"]
    assert hip.SIGNATURES["fs2hip_utterance_losses"] == "pipppiifpfpip"
    # the member struct: field for field what the header declares
    body = re.search(r"typedef struct \{([^{}]*)\} Fs2ScoreMember;", text).group(1)
    names = []
    for decl in body.split(";"):
        parts = decl.replace("*", " ").split(",")
        if decl.strip():
            names.append(parts[0].split()[-1])
            names += [x.strip() for x in parts[1:]]
    assert names == [f[0] for f in hip.ScoreMember._fields_]
    assert int(re.search(r"#define FS2_SCORE_MAX_MEMBERS (\d+)", text).group(1)) == hip.SCORE_MAX_MEMBERS
    assert int(re.search(r"#define FS2_SCORE_COLUMNS (\d+)", text).group(1)) == len(hip.SCORE_COLUMNS)
    inc = (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    assert "fs2hip_utterance_losses(" in inc
