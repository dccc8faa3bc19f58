"""numpy restatement of the DTW definition (include/fs2hip.h: ``fs2hip_frame_dist``, ``fs2hip_dtw``), generic in dtype:
run in float32 it repeats the kernels' arithmetic operation by operation, in float64 it is the reference they are bounded
against.  Shared by tests/test_dtw_cpu.py, tests/test_dtw_gpu.py and tests/test_dtw_synthesize_gpu.py."""
import itertools

import numpy as np


def frame_cost(y, r, dtype=np.float64):
    """cost[i][j] = sqrt(sum_c (y[i][c] - r[j][c])^2): every operation in ``dtype``, c ascending from 0."""
    y, r = np.asarray(y, dtype=dtype), np.asarray(r, dtype=dtype)
    acc = np.zeros((y.shape[0], r.shape[0]), dtype=dtype)
    for c in range(y.shape[1]):
        d = (y[:, c, None] - r[None, :, c]).astype(dtype)
        acc = (acc + (d * d).astype(dtype)).astype(dtype)
    return np.sqrt(acc).astype(dtype)


def dtw(cost, dtype=None):
    """(total, steps) of the recursion on ``cost`` [n, r]: diagonal first, then up, then left, each taken only when
    strictly smaller; a predecessor that does not exist is +inf.  An empty matrix gives (0, 0)."""
    cost = np.asarray(cost, dtype=dtype)
    dt = cost.dtype.type
    n, r = cost.shape
    if n == 0 or r == 0:
        return dt(0), 0
    inf = dt(np.inf)
    D = np.full((n, r), inf, dtype=cost.dtype)
    S = np.zeros((n, r), dtype=np.int64)
    for i in range(n):
        for j in range(r):
            if i == 0 and j == 0:
                D[0, 0], S[0, 0] = cost[0, 0], 1
                continue
            best, steps = (D[i - 1, j - 1], S[i - 1, j - 1]) if i > 0 and j > 0 else (inf, 0)
            if i > 0 and D[i - 1, j] < best:
                best, steps = D[i - 1, j], S[i - 1, j]
            if j > 0 and D[i, j - 1] < best:
                best, steps = D[i, j - 1], S[i, j - 1]
            D[i, j] = dt(cost[i, j] + best)
            S[i, j] = steps + 1
    return D[n - 1, r - 1], int(S[n - 1, r - 1])


def brute_force(cost):
    """The cheapest monotone path from (0, 0) to (n - 1, r - 1) by trying them all: (total, the set of lengths of the
    paths that reach it).  Small matrices only."""
    cost = np.asarray(cost, dtype=np.float64)
    n, r = cost.shape
    best, lengths = np.inf, set()

    def walk(i, j, total, cells):
        nonlocal best, lengths
        total = total + cost[i, j]
        if i == n - 1 and j == r - 1:
            if total < best:
                best, lengths = total, {cells + 1}
            elif total == best:
                lengths.add(cells + 1)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < r:
                walk(i + di, j + dj, total, cells + 1)

    walk(0, 0, 0.0, 0)
    return best, lengths


def warped_pair(n, r, C, seed):
    """Two [*, C] float32 sequences for a DTW test: one set of smooth curves sampled under two different time warps plus
    small noise, so that the cheapest path really leaves the diagonal (i.i.d. noise never pays for an extra cell)."""
    g = np.random.default_rng(seed)
    freq = g.uniform(0.5, 3.0, size=C)
    phase = g.uniform(0, 2 * np.pi, size=C)

    def sample(m, power):
        t = (np.arange(m) / max(m - 1, 1)) ** power
        return np.sin(2 * np.pi * t[:, None] * freq[None, :] + phase[None, :]) + 0.02 * g.standard_normal((m, C))

    return sample(n, 1.0).astype(np.float32), sample(r, 2.5).astype(np.float32)


#: the (n, r) of tests/test_dtw_gpu.py's batch: across the wavefront (63 / 64 / 65) and the strip boundary (128 / 129),
#: single-row and single-column recursions
LENGTHS = ((1, 1), (1, 70), (70, 1), (63, 64), (65, 129), (130, 200))
T1, T2 = 130, 200


def all_shapes(limit=4):
    return list(itertools.product(range(1, limit + 1), repeat=2))
