"""GPU: ``fs2hip_dtw_dirs`` and ``fs2hip_dtw_path`` through the binding, against the numpy restatement of their definition
(tests/dtw_path_references.py).

The batch is that of tests/test_dtw_gpu.py (its cost matrices are computed once and shared): six utterances padded to
130 x 200 whose lengths cross the wavefront (63 / 64 / 65) and the strip boundary (128 / 129) and include single-row and
single-column recursions, at C = 80 and C = 5, NaN around every box.  Every output is pre-filled -- NaN, -1 or 0xFF -- so
that a byte written outside a box shows.

Everything here is an equality.  The recursion adds and compares only, so its totals, step counts and codes are those of
the fp32 numpy recursion on the same matrix; the path is a function of the codes; a frame's cost is an fp32 sum in a stated
order.  The second batch holds small integers, where nearly every choice is a tie and the diagonal-then-up-then-left rule
alone decides the path."""
import numpy as np
import pytest
import torch

from tests import dtw_path_references as P
from tests import dtw_references as R
from tests.test_dtw_gpu import N, RL, B, _batch, _lens

pytestmark = pytest.mark.gpu

FILL = 0xFF


@pytest.fixture(scope="module")
def hip():
    from fastspeech2_lightning_amd import hip as H
    return H


def _run_dirs(hip, cost, n, r):
    b, t1, t2 = cost.shape
    total = torch.full((b,), float("nan"), device="cuda")
    steps = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    dirs = torch.full((b, t1, t2), FILL, dtype=torch.uint8, device="cuda")
    t, s = hip.dtw_dirs(cost, _lens(n), _lens(r), dirs, total=total, steps=steps)
    assert t is total and s is steps
    torch.cuda.synchronize()
    return total.cpu().numpy(), steps.cpu().numpy(), dirs


def _run_path(hip, cost, dirs, n, r):
    b, t1, _ = cost.shape
    first = torch.full((b, t1), -1, dtype=torch.int32, device="cuda")
    last = torch.full((b, t1), -1, dtype=torch.int32, device="cuda")
    fcost = torch.full((b, t1), float("nan"), device="cuda")
    got = hip.dtw_path(cost, dirs, _lens(n), _lens(r), ref_first=first, ref_last=last, frame_cost=fcost)
    assert got[0] is first and got[1] is last and got[2] is fcost
    torch.cuda.synchronize()
    return first.cpu().numpy(), last.cpu().numpy(), fcost.cpu().numpy()


def _integer_cost():
    g = np.random.default_rng(17)
    cost = np.full((B, R.T1, R.T2), np.nan, dtype=np.float32)
    for u, (n, r) in enumerate(R.LENGTHS):
        cost[u, :n, :r] = g.integers(0, 3, size=(n, r)).astype(np.float32)
    return cost


_CACHE = {}


def _case(hip, kind):
    """One batch, run once through both kernels, with its numpy references: ``kind`` is 80 or 5 (the warped batch at that
    many channels, the kernel's own cost matrix) or "ties" (small-integer matrices handed in as ``cost``)."""
    if kind not in _CACHE:
        if kind == "ties":
            cost_np = _integer_cost()
            cost = torch.from_numpy(cost_np).cuda()
        else:
            d = _batch(hip, kind)
            cost, cost_np = d["cost"], d["cost_np"]
        total, steps, dirs = _run_dirs(hip, cost, N, RL)
        first, last, fcost = _run_path(hip, cost, dirs, N, RL)
        want = []
        for u, (n, r) in enumerate(R.LENGTHS):
            box = cost_np[u, :n, :r]
            t, s, codes = P.dtw_dirs(box, np.float32)
            want.append((t, s, codes) + P.walk(box, codes))
        _CACHE[kind] = dict(cost=cost, cost_np=cost_np, total=total, steps=steps, dirs=dirs, dirs_np=dirs.cpu().numpy(),
                            first=first, last=last, fcost=fcost, want=want)
    return _CACHE[kind]


KINDS = [80, 5, "ties"]


@pytest.mark.parametrize("kind", KINDS)
def test_totals_and_steps_are_those_of_dtw_without_dirs(hip, kind):
    d = _case(hip, kind)
    total = torch.full((B,), float("nan"), device="cuda")
    steps = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    hip.dtw(d["cost"], _lens(N), _lens(RL), total=total, steps=steps)
    torch.cuda.synchronize()
    assert total.cpu().numpy().tobytes() == d["total"].tobytes()
    assert steps.cpu().numpy().tobytes() == d["steps"].tobytes()
    for u, (n, r) in enumerate(R.LENGTHS):
        want_total, want_steps = R.dtw(d["cost_np"][u, :n, :r], np.float32)
        assert d["total"][u].tobytes() == np.float32(want_total).tobytes(), (u, d["total"][u], want_total)
        assert int(d["steps"][u]) == want_steps, (u, d["steps"][u], want_steps)
        # the restatement with directions is the same recursion
        assert np.float32(d["want"][u][0]).tobytes() == np.float32(want_total).tobytes() and d["want"][u][1] == want_steps


@pytest.mark.parametrize("kind", KINDS)
def test_codes_cell_for_cell_and_nothing_outside_the_boxes(hip, kind):
    d = _case(hip, kind)
    for u, (n, r) in enumerate(R.LENGTHS):
        got, want = d["dirs_np"][u, :n, :r], d["want"][u][2]
        wrong = np.argwhere(got != want)
        assert wrong.size == 0, (u, len(wrong), wrong[:5].tolist())
        assert got[0, 0] == 0
        outside = np.ones((R.T1, R.T2), dtype=bool)
        outside[:n, :r] = False
        assert (d["dirs_np"][u][outside] == FILL).all(), u
        print(f"{kind}, utterance {u} ({n} x {r}): diagonal / up / left moves on the path {P.moves(want)}")
    if kind == 80:
        # the warped pairs' paths take all three kinds of move (the facts the CPU restatement was run for)
        for u in (3, 4, 5):
            assert min(P.moves(d["want"][u][2])) > 0, (u, P.moves(d["want"][u][2]))


@pytest.mark.parametrize("kind", KINDS)
def test_the_walk_is_the_restated_backtrack(hip, kind):
    d = _case(hip, kind)
    for u, (n, r) in enumerate(R.LENGTHS):
        _, want_steps, _, first, last, fcost = d["want"][u]
        assert d["first"][u, :n].tolist() == first.tolist(), u
        assert d["last"][u, :n].tolist() == last.tolist(), u
        assert d["fcost"][u, :n].tobytes() == fcost.tobytes(), (u, d["fcost"][u, :n], fcost)
        assert (d["first"][u, n:] == -1).all() and (d["last"][u, n:] == -1).all() and np.isnan(d["fcost"][u, n:]).all(), u
        cells = int((d["last"][u, :n].astype(np.int64) - d["first"][u, :n] + 1).sum())
        assert cells == int(d["steps"][u]) == want_steps, (u, cells, d["steps"][u])
        assert d["first"][u, 0] == 0 and d["last"][u, n - 1] == r - 1


def test_empty_boxes_write_zero_and_nothing_else(hip):
    box = np.random.default_rng(23).random((3, 5, 5)).astype(np.float32)
    cost = torch.from_numpy(box).cuda()
    n, r = [0, 5, 3], [5, 0, 3]
    total, steps, dirs = _run_dirs(hip, cost, n, r)
    first, last, fcost = _run_path(hip, cost, dirs, n, r)
    dirs = dirs.cpu().numpy()
    assert total[:2].tolist() == [0.0, 0.0] and steps[:2].tolist() == [0, 0]
    assert (dirs[:2] == FILL).all()
    assert (first[:2] == -1).all() and (last[:2] == -1).all() and np.isnan(fcost[:2]).all()
    t, s, codes = P.dtw_dirs(box[2, :3, :3], np.float32)
    assert (total[2].tobytes(), int(steps[2])) == (np.float32(t).tobytes(), s)
    assert (dirs[2, :3, :3] == codes).all() and (dirs[2, 3:] == FILL).all() and (dirs[2, :, 3:] == FILL).all()
    wf, wl, wc = P.walk(box[2, :3, :3], codes)
    assert first[2, :3].tolist() == wf.tolist() and last[2, :3].tolist() == wl.tolist()
    assert fcost[2, :3].tobytes() == wc.tobytes()
    assert (first[2, 3:] == -1).all() and (last[2, 3:] == -1).all() and np.isnan(fcost[2, 3:]).all()


@pytest.mark.parametrize("kind", [80, "ties"])
def test_an_utterance_alone_gives_the_bytes_it_gives_in_the_batch(hip, kind):
    d = _case(hip, kind)
    for u, (n, r) in enumerate(R.LENGTHS):
        cost = torch.from_numpy(np.ascontiguousarray(d["cost_np"][u:u + 1, :n, :r])).cuda()      # B = 1, tight shapes
        total, steps, dirs = _run_dirs(hip, cost, [n], [r])
        first, last, fcost = _run_path(hip, cost, dirs, [n], [r])
        assert total[0].tobytes() == d["total"][u].tobytes() and int(steps[0]) == int(d["steps"][u]), u
        assert dirs.cpu().numpy()[0].tobytes() == np.ascontiguousarray(d["dirs_np"][u, :n, :r]).tobytes(), u
        assert first[0].tobytes() == np.ascontiguousarray(d["first"][u, :n]).tobytes(), u
        assert last[0].tobytes() == np.ascontiguousarray(d["last"][u, :n]).tobytes(), u
        assert fcost[0].tobytes() == np.ascontiguousarray(d["fcost"][u, :n]).tobytes(), u


def test_allocated_results_and_foreign_codes(hip):
    """``dtw_path`` allocates what it is not given; codes the recursion cannot have written do not lead out of the box."""
    box = np.random.default_rng(29).random((1, 7, 9)).astype(np.float32)
    cost = torch.from_numpy(box).cuda()
    _, _, dirs = _run_dirs(hip, cost, [7], [9])
    first, last, fcost = hip.dtw_path(cost, dirs, _lens([7]), _lens([9]))
    assert first.dtype == last.dtype == torch.int32 and fcost.dtype == torch.float32
    assert first.shape == last.shape == fcost.shape == (1, 7)
    want = P.walk(box[0], dirs.cpu().numpy()[0])
    assert first[0].tolist() == want[0].tolist() and last[0].tolist() == want[1].tolist()
    for code in (0, 1, 2, FILL):   # all diagonal / up / left / undefined: the walk follows the border to (0, 0)
        forced = torch.full_like(dirs, code)
        f, l, _ = _run_path(hip, cost, forced, [7], [9])
        assert f[0, 0] == 0 and l[0, 6] == 8 and (f[0] >= 0).all() and (l[0] <= 8).all() and (f[0] <= l[0]).all()
        assert ((f[0, 1:] - l[0, :-1] == 0) | (f[0, 1:] - l[0, :-1] == 1)).all()


def test_the_longest_geometry_the_limit_admits(hip):
    """T1 at the path variant's LDS limit (the launch's dynamic LDS is the full 64 KiB), two strips, 176 tiles of the walk."""
    n, r = hip.DTW_PATH_MAX_T1, 70
    box = np.random.default_rng(31).integers(0, 3, size=(n, r)).astype(np.float32)
    cost = torch.from_numpy(box[None]).cuda()
    total, steps, dirs = _run_dirs(hip, cost, [n], [r])
    want_total, want_steps, codes = _fast_dirs(box)
    assert (float(total[0]), int(steps[0])) == (want_total, want_steps)
    got = dirs.cpu().numpy()[0]
    assert (got == codes).all(), np.argwhere(got != codes)[:5].tolist()
    first, last, fcost = _run_path(hip, cost, dirs, [n], [r])
    wf, wl, wc = P.walk(box, codes)
    assert first[0].tolist() == wf.tolist() and last[0].tolist() == wl.tolist() and fcost[0].tobytes() == wc.tobytes()


def _fast_dirs(cost):
    """``P.dtw_dirs`` a row at a time in plain Python floats (exact for small integers)."""
    n, r = cost.shape
    inf = float("inf")
    codes = np.zeros((n, r), dtype=np.uint8)
    prevD, prevS = [inf] * r, [0] * r
    for i in range(n):
        row = cost[i].tolist()
        curD, curS, curC = [0.0] * r, [0] * r, [0] * r
        for j in range(r):
            if i == 0 and j == 0:
                curD[0], curS[0] = row[0], 1
                continue
            best, s, c = (prevD[j - 1], prevS[j - 1], 0) if j > 0 else (inf, 0, 0)
            if prevD[j] < best:
                best, s, c = prevD[j], prevS[j], 1
            if j > 0 and curD[j - 1] < best:
                best, s, c = curD[j - 1], curS[j - 1], 2
            curD[j], curS[j], curC[j] = row[j] + best, s + 1, c
        codes[i] = curC
        prevD, prevS = curD, curS
    return prevD[-1], prevS[-1], codes


def test_refusals(hip):
    f32 = dict(device="cuda", dtype=torch.float32)
    cost = torch.zeros(2, 4, 5, **f32)
    l2 = _lens([4, 4])
    dirs = torch.zeros(2, 4, 5, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=f"at most {hip.DTW_PATH_MAX_T1} rows"):
        tall = torch.zeros(1, hip.DTW_PATH_MAX_T1 + 1, 1, **f32)
        hip.dtw_dirs(tall, _lens([1]), _lens([1]), torch.zeros(1, hip.DTW_PATH_MAX_T1 + 1, 1, dtype=torch.uint8, device="cuda"))
    # without dirs the same geometry is inside dtw's own limit
    assert hip.DTW_PATH_MAX_T1 == 5632 < hip.DTW_MAX_T1
    hip.dtw(torch.zeros(1, hip.DTW_PATH_MAX_T1 + 1, 1, **f32), _lens([1]), _lens([1]))
    with pytest.raises(ValueError, match="dirs is"):
        hip.dtw_dirs(cost, l2, l2, dirs[:, :3].contiguous())
    with pytest.raises(TypeError):
        hip.dtw_dirs(cost, l2, l2, dirs.int())
    with pytest.raises(ValueError, match="dirs is"):
        hip.dtw_path(cost, dirs[:1], l2, l2)
    with pytest.raises(ValueError, match="ref_last is"):
        hip.dtw_path(cost, dirs, l2, l2, ref_last=torch.zeros(2, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        hip.dtw_path(cost, dirs, l2, l2, frame_cost=torch.zeros(2, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="lengths"):
        hip.dtw_path(cost, dirs, l2, _lens([1]))
    # the C entry points refuse the same before any launch
    lib = hip.real_lib()
    p = cost.data_ptr()
    assert lib.fs2hip_dtw_dirs(p, l2.data_ptr(), l2.data_ptr(), p, l2.data_ptr(), None, 2, 4, 5, None) == -22
    assert lib.fs2hip_dtw_dirs(p, l2.data_ptr(), l2.data_ptr(), p, l2.data_ptr(), dirs.data_ptr(), 2,
                               hip.DTW_PATH_MAX_T1 + 1, 5, None) == -22
    assert lib.fs2hip_dtw_path(p, None, l2.data_ptr(), l2.data_ptr(), p, p, p, 2, 4, 5, None) == -22
    assert lib.fs2hip_dtw_path(p, dirs.data_ptr(), l2.data_ptr(), l2.data_ptr(), p, p, p, 2, 0, 5, None) == -22
    torch.cuda.synchronize()
