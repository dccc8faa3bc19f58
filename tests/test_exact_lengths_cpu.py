"""CPU: the host side of exact-length inference -- ``fs2l synthesize --exact-lengths`` in the parser and in ``--dry-run``,
``synthesize``'s keyword, and the binding of ``fs2hip_zero_tail_rows`` against the header's prototype."""
import inspect
import json
import re
from pathlib import Path

import torch

from fastspeech2_lightning_amd import cli
from oracle import cases as C

REPO = Path(__file__).resolve().parent.parent


def _stub_checkpoint(path):
    """A checkpoint with everything but weights: what ``--dry-run`` reads."""
    cfg = C.small_config(learn_alignment=False)
    torch.save({"global_step": 3, "hyper_parameters": {"config": cfg.model_checkpoint_dump(), "stats": C.STATS,
                                                       "lang2id": dict(C.LANG2ID), "speaker2id": dict(C.SPEAKER2ID)}}, path)
    return path


def test_parser_accepts_exact_lengths():
    p = cli.build_parser()
    on = p.parse_args(["synthesize", "m.ckpt", "-t", "abc", "-b", "32", "--exact-lengths"])
    off = p.parse_args(["synthesize", "m.ckpt", "-t", "abc"])
    assert on.exact_lengths is True and off.exact_lengths is False
    sy = next(a for a in p._subparsers._group_actions[0].choices["synthesize"]._actions if a.dest == "exact_lengths")
    assert "alone" in sy.help and "-b" in sy.help and "sort" in sy.help


def test_dry_run_echoes_the_flag(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    argv = ["synthesize", str(ckpt), "-o", str(tmp_path / "out"), "-t", "abc", "-t", "ab", "--dry-run"]
    assert cli.main(argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["exact_lengths"] is False
    assert cli.main(argv + ["--exact-lengths"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["exact_lengths"] is True and rep["batches"] == [[0, 1]]   # (the batches do not depend on it)


def test_synthesize_takes_the_keyword_and_defaults_to_off():
    from fastspeech2_lightning_amd.synthesis import synthesize
    assert inspect.signature(synthesize).parameters["exact_lengths"].default is False


def test_binding_matches_the_header_prototype():
    from fastspeech2_lightning_amd import hip
    assert "fs2hip_zero_tail_rows" in hip.EXPORTS
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fs2hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+fs2hip_zero_tail_rows\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/fs2hip.h does not declare fs2hip_zero_tail_rows"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["void* x", "long long row_bytes", "const int* lens", "int B", "int T", "void* stream"]
    assert hip.SIGNATURES["fs2hip_zero_tail_rows"] == "pqpiip"   # pointer, int64, pointer, int, int, stream
    # a plan op like every entry point that takes a stream (the generated unpacking line is current: test_plan_cpu.py)
    inc = (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    assert "fs2hip_zero_tail_rows(" in inc
