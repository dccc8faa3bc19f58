"""GPU: ``fs2hip_frame_dist`` and ``fs2hip_dtw`` through the binding, against the numpy restatement of their definition
(tests/dtw_references.py).

One batch of six utterances padded to T1 = 130, T2 = 200: lengths that cross the wavefront (63 / 64 / 65) and the strip
boundary (128 / 129) and include single-row and single-column recursions.  The inputs are smooth curves sampled under two
time warps plus small noise, so the cheapest path takes up and left moves (tests/test_dtw_cpu.py checks that on the CPU).
Every padded row of both inputs is NaN and every output buffer is pre-filled with NaN / -1 by the tests themselves.

Bounds.  ``frame_dist`` against float64: relative error at most (C + 3) * 2^-24 -- a sum of C non-negative terms in fp32
plus the subtraction's, the square's and the root's roundings.  ``dtw`` on a given fp32 matrix: adds and compares only, so
bit-equal to the fp32 numpy recursion on that matrix.  End to end against float64: at most (n + r + C) * 2^-23 relative --
the sequential-sum bound over at most n + r path cells on top of the cost bound."""
import numpy as np
import pytest
import torch

from tests import dtw_references as R

pytestmark = pytest.mark.gpu

B = len(R.LENGTHS)
N = [n for n, _ in R.LENGTHS]
RL = [r for _, r in R.LENGTHS]


@pytest.fixture(scope="module")
def hip():
    from fastspeech2_lightning_amd import hip as H
    return H


def _pairs(channels):
    return [R.warped_pair(n, r, channels, idx) for idx, (n, r) in enumerate(R.LENGTHS)]


def _padded(seqs, T):
    out = np.full((len(seqs), T, seqs[0].shape[1]), np.nan, dtype=np.float32)
    for row, s in zip(out, seqs):
        row[:len(s)] = s
    return torch.from_numpy(out).cuda()


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


_CACHE = {}


def _batch(hip, channels):
    """The batch at ``channels``: the kernel's cost buffer (NaN outside the boxes), the float64 references, computed once."""
    if channels not in _CACHE:
        pairs = _pairs(channels)
        a, b = _padded([y for y, _ in pairs], R.T1), _padded([x for _, x in pairs], R.T2)
        cost = torch.full((B, R.T1, R.T2), float("nan"), device="cuda")
        got = hip.frame_dist(a, _lens(N), b, _lens(RL), out=cost)
        assert got is cost
        torch.cuda.synchronize()
        want = [R.frame_cost(y, x) for y, x in pairs]
        _CACHE[channels] = dict(pairs=pairs, cost=cost, cost_np=cost.cpu().numpy(), want=want,
                                dtw64=[R.dtw(w) for w in want])
    return _CACHE[channels]


def _run_dtw(hip, cost, n, r):
    total = torch.full((cost.shape[0],), float("nan"), device="cuda")
    steps = torch.full((cost.shape[0],), -1, dtype=torch.int32, device="cuda")
    t, s = hip.dtw(cost, _lens(n), _lens(r), total=total, steps=steps)
    assert t is total and s is steps
    torch.cuda.synchronize()
    return total.cpu().numpy(), steps.cpu().numpy()


@pytest.mark.parametrize("channels", [80, 5])
def test_frame_dist_against_float64(hip, channels):
    d = _batch(hip, channels)
    bound = (channels + 3) * 2.0 ** -24
    for u, (n, r) in enumerate(R.LENGTHS):
        got, want = d["cost_np"][u, :n, :r].astype(np.float64), d["want"][u]
        rel = np.max(np.abs(got - want) / want)
        print(f"C = {channels}, utterance {u} ({n} x {r}): relative error {rel:.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and rel <= bound, (u, rel, bound)
        # nothing outside the utterance's box was written
        outside = np.ones((R.T1, R.T2), dtype=bool)
        outside[:n, :r] = False
        assert np.isnan(d["cost_np"][u][outside]).all(), u


@pytest.mark.parametrize("channels", [80, 5])
def test_dtw_is_the_fp32_recursion_on_its_own_cost_matrix(hip, channels):
    d = _batch(hip, channels)
    total, steps = _run_dtw(hip, d["cost"], N, RL)
    for u, (n, r) in enumerate(R.LENGTHS):
        want_total, want_steps = R.dtw(d["cost_np"][u, :n, :r], np.float32)
        print(f"C = {channels}, utterance {u} ({n} x {r}): total {total[u]!r} / {want_total!r}, steps {steps[u]} / {want_steps}")
        assert total[u].tobytes() == np.float32(want_total).tobytes(), (u, total[u], want_total)
        assert int(steps[u]) == want_steps, (u, steps[u], want_steps)


@pytest.mark.parametrize("channels", [80, 5])
def test_end_to_end_against_float64(hip, channels):
    d = _batch(hip, channels)
    total, _ = _run_dtw(hip, d["cost"], N, RL)
    for u, (n, r) in enumerate(R.LENGTHS):
        want = d["dtw64"][u][0]
        bound = (n + r + channels) * 2.0 ** -23 * want
        print(f"C = {channels}, utterance {u} ({n} x {r}): |total - total64| {abs(float(total[u]) - want):.3e}, bound {bound:.3e}")
        assert abs(float(total[u]) - want) <= bound, (u, total[u], want)


def test_exact_ties_follow_the_stated_order(hip):
    """Small integers 0..2, 37 x 70 inside a padded 40 x 130 (NaN around): almost every cell ties, and a sum of at most 106
    small integers is exact in fp32 -- so the total is also the float64 one, and the step count says which tie won."""
    g = np.random.default_rng(5)
    box = g.integers(0, 3, size=(37, 70)).astype(np.float32)
    cost = np.full((1, 40, 130), np.nan, dtype=np.float32)
    cost[0, :37, :70] = box
    total, steps = _run_dtw(hip, torch.from_numpy(cost).cuda(), [37], [70])
    want_total, want_steps = R.dtw(box, np.float32)
    assert (float(total[0]), int(steps[0])) == (float(want_total), want_steps)
    total64, steps64 = R.dtw(box.astype(np.float64))
    assert (float(want_total), want_steps) == (float(total64), steps64) and steps64 > 70
    # the transposed problem swaps the roles of up and left: another path length unless the rule were symmetric
    total_t, steps_t = _run_dtw(hip, torch.from_numpy(np.ascontiguousarray(cost.transpose(0, 2, 1))).cuda(), [70], [37])
    want_t = R.dtw(np.ascontiguousarray(box.T), np.float32)
    assert (float(total_t[0]), int(steps_t[0])) == (float(want_t[0]), want_t[1]) and float(total_t[0]) == float(total[0])


def test_a_row_does_not_depend_on_its_batch(hip):
    d = _batch(hip, 80)
    total, steps = _run_dtw(hip, d["cost"], N, RL)
    for u, (n, r) in enumerate(R.LENGTHS):
        y, x = d["pairs"][u]
        a, b = torch.from_numpy(y[None]).cuda(), torch.from_numpy(x[None]).cuda()      # B = 1, tight shapes
        cost = hip.frame_dist(a, _lens([n]), b, _lens([r]))
        assert cost.shape == (1, n, r)
        assert cost.cpu().numpy().tobytes() == np.ascontiguousarray(d["cost_np"][u, :n, :r]).tobytes(), u
        t1, s1 = _run_dtw(hip, cost, [n], [r])
        assert t1[0].tobytes() == total[u].tobytes() and int(s1[0]) == int(steps[u]), (u, t1, total[u], s1, steps[u])


def test_empty_rows_and_clamped_lengths(hip):
    """n = 0 and r = 0 give (0, 0) without touching the matrix; lengths beyond the geometry are clamped to it."""
    box = np.random.default_rng(3).random((3, 6, 9)).astype(np.float32)
    cost = torch.from_numpy(box).cuda()
    total, steps = _run_dtw(hip, cost, [0, 4, 99], [5, 0, 99])
    assert total[:2].tolist() == [0.0, 0.0] and steps[:2].tolist() == [0, 0]
    want = R.dtw(box[2], np.float32)
    assert (total[2].tobytes(), int(steps[2])) == (np.float32(want[0]).tobytes(), want[1])
    nan_cost = torch.full((2, 4, 4), float("nan"), device="cuda")
    ones = torch.ones(2, 4, 3, device="cuda")
    hip.frame_dist(ones, _lens([0, -3]), ones, _lens([4, 4]), out=nan_cost)
    torch.cuda.synchronize()
    assert torch.isnan(nan_cost).all()


def test_refusals(hip):
    f32 = dict(device="cuda", dtype=torch.float32)
    a, b = torch.zeros(2, 4, 8, **f32), torch.zeros(2, 5, 8, **f32)
    l2 = _lens([4, 4])
    with pytest.raises(ValueError, match="frame_dist"):
        hip.frame_dist(a, l2, torch.zeros(2, 5, 7, **f32), l2)                       # channel counts differ
    with pytest.raises(ValueError, match="lengths"):
        hip.frame_dist(a, _lens([4]), b, l2)
    with pytest.raises(TypeError):
        hip.frame_dist(a, l2.long(), b, l2)
    with pytest.raises(ValueError, match="out is"):
        hip.frame_dist(a, l2, b, l2, out=torch.zeros(2, 4, 6, **f32))
    with pytest.raises(ValueError, match=f"at most {hip.FRAME_DIST_MAX_C} channels"):
        wide = torch.zeros(1, 2, hip.FRAME_DIST_MAX_C + 1, **f32)
        hip.frame_dist(wide, _lens([2]), wide, _lens([2]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.frame_dist(a.cpu(), l2, b, l2)
    cost = torch.zeros(2, 4, 5, **f32)
    with pytest.raises(ValueError, match=f"at most {hip.DTW_MAX_T1} rows"):
        hip.dtw(torch.zeros(1, hip.DTW_MAX_T1 + 1, 1, **f32), _lens([1]), _lens([1]))
    with pytest.raises(ValueError, match="lengths"):
        hip.dtw(cost, l2, _lens([1, 2, 3]))
    with pytest.raises(ValueError, match="entries"):
        hip.dtw(cost, l2, l2, total=torch.zeros(3, **f32))
    with pytest.raises(TypeError):
        hip.dtw(cost, l2, l2, steps=torch.zeros(2, **f32))
    with pytest.raises(ValueError, match="non-empty"):
        hip.dtw(torch.zeros(2, 4, **f32), l2, l2)
    # the C entry points refuse the same before any launch
    lib = hip.real_lib()
    assert lib.fs2hip_dtw(None, l2.data_ptr(), l2.data_ptr(), cost.data_ptr(), l2.data_ptr(), 2, 4, 5, None) == -22
    assert lib.fs2hip_dtw(cost.data_ptr(), l2.data_ptr(), l2.data_ptr(), cost.data_ptr(), l2.data_ptr(), 2,
                          hip.DTW_MAX_T1 + 1, 5, None) == -22
    assert lib.fs2hip_frame_dist(a.data_ptr(), l2.data_ptr(), b.data_ptr(), l2.data_ptr(), cost.data_ptr(), 2, 4, 5,
                                 hip.FRAME_DIST_MAX_C + 1, None) == -22


def test_the_longest_geometry_the_limit_admits(hip):
    """T1 at the LDS limit, three strips: the launch's dynamic LDS is the full 64 KiB."""
    n, r = hip.DTW_MAX_T1, 130
    box = np.random.default_rng(11).integers(0, 3, size=(n, r)).astype(np.float32)
    total, steps = _run_dtw(hip, torch.from_numpy(box[None]).cuda(), [n], [r])
    want = _fast_dtw(box)
    assert (float(total[0]), int(steps[0])) == want


def _fast_dtw(cost):
    """The same recursion, a row at a time where the order of evaluation allows it (the left dependence stays a loop over
    columns, in plain Python floats: exact for small integers)."""
    n, r = cost.shape
    inf = float("inf")
    prevD, prevS = [inf] * r, [0] * r
    for i in range(n):
        row = cost[i].tolist()
        curD, curS = [0.0] * r, [0] * r
        for j in range(r):
            if i == 0 and j == 0:
                curD[0], curS[0] = row[0], 1
                continue
            best, s = (prevD[j - 1], prevS[j - 1]) if j > 0 else (inf, 0)
            if prevD[j] < best:
                best, s = prevD[j], prevS[j]
            if j > 0 and curD[j - 1] < best:
                best, s = curD[j - 1], curS[j - 1]
            curD[j], curS[j] = row[j] + best, s + 1
        prevD, prevS = curD, curS
    return prevD[-1], prevS[-1]
