"""numpy restatement of the warping path (include/fs2hip.h: ``fs2hip_dtw_dirs``, ``fs2hip_dtw_path``): the recursion of
``tests/dtw_references.dtw`` with the code of the chosen predecessor kept, and the backtrack through those codes with the
kernel's summation order.  Shared by tests/test_dtw_path_cpu.py, tests/test_dtw_path_gpu.py and
tests/test_dtw_path_synthesize_gpu.py."""
import math

import numpy as np

DIAG, UP, LEFT = 0, 1, 2


def dtw_dirs(cost, dtype=None):
    """(total, steps, dirs [n, r] uint8) of the recursion on ``cost`` [n, r]: ``dtw_references.dtw`` statement by
    statement, plus the predecessor taken at every cell -- 0 diagonal, 1 up ``(i-1, j)``, 2 left ``(i, j-1)``; cell (0, 0)
    gets 0.  An empty matrix gives (0, 0, an empty array)."""
    cost = np.asarray(cost, dtype=dtype)
    dt = cost.dtype.type
    n, r = cost.shape
    dirs = np.zeros((n, r), dtype=np.uint8)
    if n == 0 or r == 0:
        return dt(0), 0, dirs
    inf = dt(np.inf)
    D = np.full((n, r), inf, dtype=cost.dtype)
    S = np.zeros((n, r), dtype=np.int64)
    for i in range(n):
        for j in range(r):
            if i == 0 and j == 0:
                D[0, 0], S[0, 0] = cost[0, 0], 1
                continue
            best, steps, code = (D[i - 1, j - 1], S[i - 1, j - 1], DIAG) if i > 0 and j > 0 else (inf, 0, DIAG)
            if i > 0 and D[i - 1, j] < best:
                best, steps, code = D[i - 1, j], S[i - 1, j], UP
            if j > 0 and D[i, j - 1] < best:
                best, steps, code = D[i, j - 1], S[i, j - 1], LEFT
            D[i, j] = dt(cost[i, j] + best)
            S[i, j] = steps + 1
            dirs[i, j] = code
    return D[n - 1, r - 1], int(S[n - 1, r - 1]), dirs


def path_cells(dirs):
    """The cells of the path through ``dirs`` [n, r], from (n - 1, r - 1) back to (0, 0), in the walk's order."""
    n, r = dirs.shape
    if n == 0 or r == 0:
        return []
    i, j = n - 1, r - 1
    cells = [(i, j)]
    while (i, j) != (0, 0):
        code = int(dirs[i, j])
        if code == LEFT:
            j -= 1
        elif code == UP:
            i -= 1
        else:
            i, j = i - 1, j - 1
        assert i >= 0 and j >= 0, "the codes lead outside the matrix"
        cells.append((i, j))
    return cells


def walk(cost, dirs):
    """(ref_first [n] int32, ref_last [n] int32, frame_cost [n] float32) of the backtrack: per row the smallest and
    largest column on the path and the float32 sum of the row's path cells, started from ``cost[i, ref_last[i]]`` and
    added in the order the walk meets them (j descending)."""
    cost = np.asarray(cost, dtype=np.float32)
    n = cost.shape[0]
    first = np.zeros(n, dtype=np.int32)
    last = np.zeros(n, dtype=np.int32)
    total = np.zeros(n, dtype=np.float32)
    seen = set()
    for i, j in path_cells(dirs):
        if i not in seen:
            seen.add(i)
            last[i], total[i] = j, cost[i, j]
        else:
            total[i] = np.float32(total[i] + cost[i, j])
        first[i] = j
    return first, last, total


def moves(dirs):
    """(diagonal, up, left) move counts of the path through ``dirs``."""
    cells = path_cells(dirs)
    count = [0, 0, 0]
    for i, j in cells[:-1]:
        count[int(dirs[i, j])] += 1
    return tuple(count)


def brute_force_paths(cost):
    """Every cheapest monotone path from (0, 0) to (n - 1, r - 1), by trying them all, in float64: (the minimum, the list
    of paths that reach it, each a list of cells from (0, 0) on).  Small matrices only."""
    cost = np.asarray(cost, dtype=np.float64)
    n, r = cost.shape
    best, paths = np.inf, []

    def go(i, j, total, cells):
        nonlocal best, paths
        total = total + cost[i, j]
        cells = cells + [(i, j)]
        if i == n - 1 and j == r - 1:
            if total < best:
                best, paths = total, [cells]
            elif total == best:
                paths.append(cells)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < r:
                go(i + di, j + dj, total, cells)

    go(0, 0, 0.0, [])
    return best, paths


def token_values(duration, ref_first, ref_last, frame_cost, ref_frames):
    """What ``data.DtwPathWriter`` derives per token, restated with plain loops: (cells, cost float64, ref_start, ref_end)
    lists.  Token k owns frames [s_k, e_k) of the cumulative durations; a token without frames has 0 cells, 0 cost and
    start = end = the start of the next token that has frames (``ref_frames`` if there is none)."""
    ends = np.cumsum(np.asarray(duration, dtype=np.int64))
    starts = ends - np.asarray(duration, dtype=np.int64)
    K = len(ends)
    cells, cost, rs, re = [0] * K, [0.0] * K, [0] * K, [0] * K
    nxt = int(ref_frames)
    for k in range(K - 1, -1, -1):
        s, e = int(starts[k]), int(ends[k])
        if e > s:
            cells[k] = int(sum(int(ref_last[i]) - int(ref_first[i]) + 1 for i in range(s, e)))
            cost[k] = math.fsum(float(x) for x in frame_cost[s:e])   # (exactly rounded: no order to agree on)
            rs[k], re[k] = int(ref_first[s]), int(ref_last[e - 1]) + 1
            nxt = rs[k]
        else:
            rs[k] = re[k] = nxt
    return cells, cost, rs, re
