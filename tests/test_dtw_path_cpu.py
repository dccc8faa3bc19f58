"""CPU: the restated warping path (tests/dtw_path_references.py) against exhaustive search, ``data.DtwPathWriter`` on
hand-made packed buffers, and the command line of ``fs2l synthesize --write-paths``."""
import csv
import inspect
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests import dtw_path_references as P
from tests import dtw_references as R

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ["_", "a", "b", "c", "d"]


@pytest.mark.parametrize("shape", R.all_shapes(4), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restated_path_is_a_cheapest_monotone_path(shape):
    """Every shape up to 4 x 4, on real-valued costs (the cheapest path is unique) and on small integers (full of ties): the
    path runs from (0, 0) to (n - 1, r - 1) by the three moves, its float64 cost is the minimum over ALL monotone paths,
    and ``total`` and ``steps`` are ``dtw_references.dtw``'s."""
    n, r = shape
    g = np.random.default_rng(100 * n + r)
    for trial in range(12):
        cost = g.random(shape) if trial % 2 == 0 else g.integers(0, 3, shape).astype(np.float64)
        total, steps, dirs = P.dtw_dirs(cost)
        assert (total, steps) == R.dtw(cost)
        assert dirs.shape == shape and dirs.dtype == np.uint8 and dirs[0, 0] == 0
        cells = P.path_cells(dirs)[::-1]
        assert cells[0] == (0, 0) and cells[-1] == (n - 1, r - 1) and len(cells) == steps
        for (i0, j0), (i1, j1) in zip(cells, cells[1:]):
            assert (i1 - i0, j1 - j0) in ((1, 1), (1, 0), (0, 1))
        best, paths = P.brute_force_paths(cost)
        walked = sum(cost[i, j] for i, j in cells)
        assert abs(walked - best) <= 1e-12 * max(1.0, best), (cost, walked, best)
        if trial % 2 == 0:
            assert paths == [cells]                       # no ties: THE cheapest path
        else:
            assert cells in paths
        first, last, fcost = P.walk(cost, dirs)
        assert first[0] == 0 and last[-1] == r - 1 and int((last - first + 1).sum()) == steps
        for i in range(n):
            row = [j for (k, j) in cells if k == i]
            assert (first[i], last[i]) == (min(row), max(row)) and row == list(range(min(row), max(row) + 1))


def test_the_walk_s_summation_order_and_the_tie_rule_by_hand():
    # all equal: the diagonal wherever it exists, then along the border
    _, steps, dirs = P.dtw_dirs(np.ones((2, 4)))
    assert steps == 4 and dirs.tolist() == [[0, 2, 2, 2], [1, 0, 0, 0]]
    assert P.path_cells(dirs) == [(1, 3), (0, 2), (0, 1), (0, 0)] and P.moves(dirs) == (1, 0, 2)
    first, last, fcost = P.walk(np.ones((2, 4)), dirs)
    assert (first.tolist(), last.tolist(), fcost.tolist()) == ([0, 3], [2, 3], [3.0, 1.0])
    # up and left tie below the diagonal's cost: up is asked first
    _, _, dirs = P.dtw_dirs(np.array([[2.0, -1.0], [-1.0, 0.0]]))
    assert dirs.tolist() == [[0, 2], [1, 1]]
    # one row holding 1, 2^-24, 2^-24, all on the path: from the LAST cell on the sum is (2^-24 + 2^-24) + 1 = 1 + 2^-23 in
    # fp32; in ascending j it would stay 1
    c = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], dtype=np.float32)
    _, _, dirs = P.dtw_dirs(c, np.float32)
    first, last, fcost = P.walk(c, dirs)
    assert (first.tolist(), last.tolist()) == ([0], [2])
    assert fcost[0] == np.float32(1.0 + 2.0 ** -23) and fcost.dtype == np.float32
    assert np.float32(np.float32(c[0, 0] + c[0, 1]) + c[0, 2]) == np.float32(1.0)
    # empty matrices
    assert P.dtw_dirs(np.zeros((0, 3)))[:2] == (0.0, 0) and P.path_cells(np.zeros((3, 0), dtype=np.uint8)) == []


def test_the_gpu_tests_paths_take_every_kind_of_move():
    """The facts tests/test_dtw_path_gpu.py relies on, on the float32 restatement of its C = 80 batch: ``total`` and ``steps``
    are ``dtw_references.dtw``'s, the cells add up to ``steps``, and the three longest utterances' paths hold diagonal, up and
    left moves."""
    counts = {}
    for idx, (n, r) in enumerate(R.LENGTHS):
        y, x = R.warped_pair(n, r, 80, idx)
        c32 = R.frame_cost(y, x, np.float32)
        total, steps, dirs = P.dtw_dirs(c32)
        want = R.dtw(c32)
        assert np.float32(total).tobytes() == np.float32(want[0]).tobytes() and steps == want[1]
        first, last, _ = P.walk(c32, dirs)
        assert int((last.astype(np.int64) - first + 1).sum()) == steps
        counts[(n, r)] = P.moves(dirs)
        assert sum(counts[(n, r)]) == steps - 1
    assert counts[(63, 64)] == (42, 20, 21) and counts[(65, 129)] == (62, 2, 66) and counts[(130, 200)] == (113, 16, 86)


# ---------------------------------------------------------------------------------------------------------------------
# DtwPathWriter on hand-made buffers
# ---------------------------------------------------------------------------------------------------------------------
def _pack(utterances):
    """[(duration, ref_first, ref_last, frame_cost)] -> (packed fp32 buffer, members): every member's rows back to back, the
    members one after the other, as ``hip.pack_rows`` leaves them (int32 rows as bit patterns)."""
    parts, members, at = [], {}, 0
    for k, name in enumerate(D.DtwPathWriter.MEMBERS):
        offsets = [0]
        for u in utterances:
            row = torch.tensor(u[k], dtype=torch.float32 if name == "frame_cost" else torch.int32)
            parts.append(row if name == "frame_cost" else row.view(torch.float32))
            offsets.append(offsets[-1] + row.numel())
        members[name] = (at, offsets)
        at += offsets[-1]
    return torch.cat(parts), members


def _batch(names, texts):
    return {"basename": names, "speaker": ["spk0"] * len(names), "language": ["l0"] * len(names),
            "raw_text": [f"text of {n}" for n in names], "text": [torch.tensor(t) for t in texts]}


# a 5-frame synthesis against 6 recorded frames; cells: (0,0) (1,1) (1,2) (2,2) (3,3) (4,4) (4,5) = 7
FIRST, LAST = [0, 1, 2, 3, 4], [0, 2, 2, 3, 5]
FCOST = [0.5, 1.25, 0.25, 2.0, 3.0]


def test_the_writer_cuts_the_path_into_tokens(tmp_path):
    w = D.DtwPathWriter(tmp_path / "out", 7, SYMBOLS)
    assert w.path == tmp_path / "out" / "dtw-tokens-7.psv"
    # tokens a b _ c: durations 2, 1, 0, 2 -- the third has no frames; the up move (1,2) -> (2,2) crosses the a | b boundary
    packed, members = _pack([([2, 1, 0, 2], FIRST, LAST, FCOST)])
    files = w.write_packed(packed, members, _batch(["u0"], [[1, 2, 0, 3, 4, 4]]), [0], [5], [6], [7.0], [7])
    assert files == [tmp_path / "out" / "dtw_path" / "u0--spk0--l0--ckpt=7--dtw-path.pt"]
    rec = torch.load(files[0], weights_only=True)
    assert sorted(rec) == sorted(["ref_first", "ref_last", "frame_cost", "frames", "ref_frames", "total", "steps", "text",
                                  "symbols", "duration", "token_cells", "token_cost", "token_ref_start", "token_ref_end",
                                  "basename", "speaker", "language", "raw_text"])
    assert rec["ref_first"].tolist() == FIRST and rec["ref_last"].tolist() == LAST and rec["frame_cost"].tolist() == FCOST
    assert rec["ref_first"].dtype == rec["ref_last"].dtype == torch.int32 and rec["frame_cost"].dtype == torch.float32
    assert (rec["frames"], rec["ref_frames"], rec["total"], rec["steps"]) == (5, 6, 7.0, 7)
    assert rec["text"].tolist() == [1, 2, 0, 3] and rec["symbols"] == ["a", "b", "_", "c"]      # the padded tail is cut
    assert rec["duration"].tolist() == [2, 1, 0, 2] and rec["duration"].dtype == torch.int32
    assert rec["token_cells"].tolist() == [3, 1, 0, 3] and int(rec["token_cells"].sum()) == rec["steps"]
    assert rec["token_cost"].tolist() == [1.75, 0.25, 0.0, 5.0] and rec["token_cost"].dtype == torch.float64
    assert rec["token_ref_start"].tolist() == [0, 2, 3, 3] and rec["token_ref_end"].tolist() == [3, 3, 3, 6]
    # a and b share recorded frame 2; the empty token sits where the next one starts
    assert rec["token_ref_end"][0] == rec["token_ref_start"][1] + 1
    assert (rec["basename"], rec["speaker"], rec["language"], rec["raw_text"]) == ("u0", "spk0", "l0", "text of u0")
    want = P.token_values([2, 1, 0, 2], FIRST, LAST, FCOST, 6)
    assert (rec["token_cells"].tolist(), rec["token_cost"].tolist(), rec["token_ref_start"].tolist(),
            rec["token_ref_end"].tolist()) == tuple(want)
    # trailing tokens without frames end at the recording's end
    tok = D.DtwPathWriter.tokens(torch.tensor([5, 0, 0]), torch.tensor(FIRST), torch.tensor(LAST), torch.tensor(FCOST), 6)
    assert tok["token_ref_start"].tolist() == [0, 6, 6] and tok["token_ref_end"].tolist() == [6, 6, 6]
    assert tok["token_cells"].tolist() == [7, 0, 0] and tok["token_cost"].tolist() == [math.fsum(FCOST), 0.0, 0.0]
    with pytest.raises(ValueError, match="twice"):
        w.write_packed(packed, members, _batch(["u0"], [[1, 2, 0, 3]]), [0], [5], [6], [7.0], [7])


def test_clipped_durations_add_up_to_the_frames(tmp_path):
    """The model's ``max_length`` cut the output to 5 frames where the durations add up to 8: the durations of the file are
    ``AlignmentWriter.clip``'s, and the tokens are cut from those."""
    w = D.DtwPathWriter(tmp_path, 0, SYMBOLS)
    packed, members = _pack([([2, 2, 3, 1], FIRST, LAST, FCOST)])
    rec = torch.load(w.write_packed(packed, members, _batch(["cut"], [[1, 2, 3, 4]]), [0], [5], [6], [7.0], [7])[0],
                     weights_only=True)
    assert rec["duration"].tolist() == D.AlignmentWriter.clip(torch.tensor([2, 2, 3, 1]), 5).tolist() == [2, 2, 1, 0]
    assert int(rec["duration"].sum()) == rec["frames"] == 5
    assert rec["token_cells"].tolist() == [3, 2, 2, 0] and rec["token_ref_end"].tolist() == [3, 4, 6, 6]
    assert rec["token_ref_start"].tolist() == [0, 2, 4, 6]
    with pytest.raises(ValueError, match="add up to 4"):
        w.write_packed(*_pack([([2, 2], FIRST, LAST, FCOST)]), _batch(["short"], [[1, 2]]), [1], [5], [6], [7.0], [7])


def test_every_consistency_check_raises(tmp_path):
    w = D.DtwPathWriter(tmp_path, 0, SYMBOLS)

    def write(first=FIRST, last=LAST, ref_frames=6, steps=7, frames=5, fcost=FCOST, pos=[0]):
        pos[0] += 1
        packed, members = _pack([([2, 1, 0, 2], first, last, fcost)])
        return w.write_packed(packed, members, _batch([f"u{pos[0]}"], [[1, 2, 0, 3]]), [pos[0]], [frames], [ref_frames], [7.0],
                              [steps])

    write()
    with pytest.raises(ValueError, match="from recorded frame 1"):
        write(first=[1, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="not from 0 to 6"):
        write(ref_frames=7)
    with pytest.raises(ValueError, match="not connected at frame 3"):
        write(first=[0, 1, 2, 4, 4], last=[0, 2, 2, 4, 5])                      # a recorded frame is skipped
    with pytest.raises(ValueError, match="not connected at frame 2"):
        write(first=[0, 1, 1, 3, 4], last=[0, 2, 2, 3, 5])                      # the path goes back
    with pytest.raises(ValueError, match="behind its last"):
        write(first=[0, 1, 3, 3, 4], last=[0, 2, 2, 3, 5])
    with pytest.raises(ValueError, match="7 cells where the recursion counted 8"):
        write(steps=8)
    with pytest.raises(ValueError, match="4 ref_last values for 5 frames"):
        write(last=[0, 2, 2, 3])
    with pytest.raises(ValueError, match="members must be"):
        w.write_packed(torch.zeros(4), {"duration": (0, [0, 1])}, _batch(["x"], [[1]]), [50], [1], [1], [1.0], [1])
    with pytest.raises(ValueError, match="2 totals for 1"):
        packed, members = _pack([([2, 1, 0, 2], FIRST, LAST, FCOST)])
        w.write_packed(packed, members, _batch(["x"], [[1, 2, 0, 3]]), [51], [5], [6], [7.0, 1.0], [7])
    with pytest.raises(ValueError, match="do not delimit"):
        packed, members = _pack([([2, 1, 0, 2], FIRST, LAST, FCOST)])
        members["frame_cost"] = (members["frame_cost"][0] + 1, members["frame_cost"][1])
        w.write_packed(packed, members, _batch(["x"], [[1, 2, 0, 3]]), [52], [5], [6], [7.0], [7])
    with pytest.raises(ValueError, match="symbol table"):
        D.DtwPathWriter(tmp_path, 0)
    assert sorted(w.records) == [1]                                             # nothing of a refused piece is kept


def test_the_token_table_is_sorted_worst_first(tmp_path):
    w = D.DtwPathWriter(tmp_path / "o", 41, SYMBOLS)
    one = ([1, 1], [0, 1], [0, 1], None)      # two frames on the diagonal of a 2 x 2 box: two cells

    def add(pos, name, fcost, total=None, frames=2, ref_frames=2, steps=2, first=(0, 1), last=(0, 1), dur=(1, 1)):
        packed, members = _pack([(list(dur), list(first), list(last), fcost)])
        w.write_packed(packed, members, _batch([name], [[1, 2]]), [pos], [frames], [ref_frames],
                       [sum(fcost) if total is None else total], [steps])

    add(3, "d", [1.0, 3.0])                   # mean 2, worst token 3: ratio 1.5 -- ties with b, input order keeps b first
    add(1, "b", [3.0, 1.0])                   # ratio 1.5, worst token 0
    add(2, "c", [0.5, 3.5])                   # mean 2, worst 3.5: ratio 1.75
    add(0, "a", [], frames=0, steps=0, first=(), last=(), dur=(0, 0), total=0.0)    # no path: last
    add(4, "e", [0.0, 0.0])                   # a mean of 0: no ratio
    add(5, "f", [2.0, 2.0])                   # equal tokens: the first, ratio 1
    path = w.close()
    assert path == tmp_path / "o" / "dtw-tokens-41.psv"
    lines = path.read_text(encoding="utf8").splitlines()
    assert lines[0] == "|".join(D.DtwPathWriter.FIELDS) == (
        "basename|speaker|language|token_index|symbol|token_frames|ref_start|ref_end|token_mel_dtw|mel_dtw|ratio|raw_text")
    assert [ln.split("|")[0] for ln in lines[1:]] == ["c", "b", "d", "f", "a", "e"]
    with open(path, encoding="utf8", newline="") as f:
        rows = {r["basename"]: r for r in csv.DictReader(f, delimiter="|")}
    assert rows["c"] == dict(basename="c", speaker="spk0", language="l0", token_index="1", symbol="b", token_frames="1",
                             ref_start="1", ref_end="2", token_mel_dtw="3.5", mel_dtw="2.0", ratio="1.75", raw_text="text of c")
    assert rows["b"]["token_index"] == "0" and rows["b"]["symbol"] == "a" and rows["d"]["token_index"] == "1"
    assert rows["f"]["token_index"] == "0" and rows["f"]["ratio"] == "1.0"
    assert rows["a"]["token_index"] == rows["a"]["mel_dtw"] == rows["a"]["ratio"] == rows["a"]["symbol"] == ""
    assert rows["e"]["ratio"] == "" and rows["e"]["mel_dtw"] == "0.0" and rows["e"]["token_mel_dtw"] == "0.0"
    # the file of an entry without a path: empty rows, tokens without cells at the recording's end
    rec = torch.load(w.filename("a", "spk0", "l0"), weights_only=True)
    assert rec["ref_first"].numel() == rec["frame_cost"].numel() == 0 and rec["steps"] == 0 and rec["frames"] == 0
    assert rec["token_cells"].tolist() == [0, 0] and rec["token_ref_start"].tolist() == [2, 2]
    del one


# ---------------------------------------------------------------------------------------------------------------------
# the command line, the signatures, the slot
# ---------------------------------------------------------------------------------------------------------------------
def test_write_paths_needs_compare_to(tmp_path, capsys):
    missing = tmp_path / "no_such.ckpt"      # never opened: the error is raised first
    with pytest.raises(SystemExit, match="--write-paths goes with --compare-to"):
        cli.main(["synthesize", str(missing), "-f", "l.psv", "--write-paths"])
    assert "Loading checkpoint" not in capsys.readouterr().err
    p = cli.build_parser()
    a = p.parse_args(["synthesize", "m.ckpt", "-f", "l.psv", "--compare-to", "dir", "--write-paths"])
    assert a.write_paths and a.compare_to == Path("dir")
    assert p.parse_args(["synthesize", "m.ckpt", "-f", "l.psv", "--compare-to", "dir"]).write_paths is False
    from fastspeech2_lightning_amd.synthesis import synthesize
    with pytest.raises(ValueError, match="goes with compare="):
        synthesize(None, None, 2, None, None, paths=D.DtwPathWriter(tmp_path, 0, SYMBOLS))


def test_dry_run_lists_the_path_files(tmp_path, capsys):
    from tests.test_dtw_cpu import _stub_checkpoint
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    fl = tmp_path / "list.psv"
    fl.write_text("basename|language|speaker|characters\nu0|l0|spk0|abca\nu1|l0|spk0|ab\n", encoding="utf8")
    out = tmp_path / "out"
    argv = ["synthesize", str(ckpt), "-o", str(out), "-f", str(fl), "--dry-run", "--compare-to", str(tmp_path / "corpus")]
    assert cli.main(argv) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "path_files" not in plain and "dtw_tokens_file" not in plain
    assert cli.main(argv + ["--write-paths"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["dtw_tokens_file"] == str(out / "dtw-tokens-3.psv")
    assert rep["path_files"] == [str(out / "dtw_path" / f"u{k}--spk0--l0--ckpt=3--dtw-path.pt") for k in (0, 1)]
    assert {k: v for k, v in rep.items() if k not in ("path_files", "dtw_tokens_file")} == plain
    assert not out.exists()


def test_the_new_arguments_the_binding_and_the_slot():
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.synthesis import _Slot, synthesize
    assert inspect.signature(synthesize).parameters["paths"].default is None
    # the existing calls keep their parameter lists; the path has calls of its own beside them
    assert list(inspect.signature(FastSpeech2.mel_dtw_paths).parameters) == list(inspect.signature(FastSpeech2.mel_dtw).parameters)
    assert list(inspect.signature(hip.dtw_dirs).parameters) == ["cost", "lens1", "lens2", "dirs", "total", "steps"]
    assert "dirs" not in inspect.signature(hip.dtw).parameters
    assert list(inspect.signature(hip.dtw_path).parameters) == ["cost", "dirs", "lens1", "lens2", "ref_first", "ref_last",
                                                                "frame_cost"]
    assert hip.SIGNATURES["fs2hip_dtw_dirs"] == "ppppppiiip" and hip.SIGNATURES["fs2hip_dtw_path"] == "pppppppiiip"
    text = (REPO / "include" / "fs2hip.h").read_text()
    assert int(re.search(r"#define FS2_DTW_PATH_MAX_T1 (\d+)", text).group(1)) == hip.DTW_PATH_MAX_T1
    # the limit is what 64 KiB of LDS holds beside the cost ring and the ring of codes
    assert 64 * 64 * 4 + 64 * 64 + 8 * hip.DTW_PATH_MAX_T1 == 64 * 1024
    inc = (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    assert "fs2hip_dtw_dirs(" in inc and "fs2hip_dtw_path(" in inc
    # the slot's header: four more offset tables in front of the DTW totals, which keep their place at its end
    for B in (1, 2, 3, 4, 5):
        assert _Slot.header(B, False, 3 + 4, True) - _Slot.header(B, False, 3, True) == 4 * _Slot.table(B)
        assert len(D.DtwPathWriter.MEMBERS) == 4
