"""Python restatement of the rectangular linear sum assignment that csrc/assign.hip's `k_lsa`
implements: the shortest-augmenting-path method of Crouse, "On implementing 2D rectangular
assignment algorithms" (IEEE T-AES 52(4), 2016), in the form `scipy.optimize.linear_sum_assignment`
runs it -- float64 duals on the cost converted from fp32, the same scan order, the same tie rule --
so that `row_ind` / `col_ind` EQUAL scipy's (tests/test_assign.py), not just their total cost.

    lsa(cost) -> (row_ind, col_ind, status)

status: 0 solved; 1 a NaN or -inf entry; 2 infeasible (scipy raises ValueError on both; the
kernel writes the status and fills its outputs with -1, and so does this).
"""
import numpy as np

INF = float("inf")


def lsa(cost):
    cost = np.asarray(cost, dtype=np.float64)
    rows, cols = cost.shape
    n = min(rows, cols)
    fail = lambda st: (np.full(n, -1, np.int64), np.full(n, -1, np.int64), st)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    transposed = cols < rows
    c = cost.T if transposed else cost
    nr, nc = c.shape
    if np.isnan(c).any() or (c == -INF).any():
        return fail(1)
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col, path = [-1] * nr, [-1] * nc, [-1] * nc
    for cur in range(nr):
        shortest = [INF] * nc
        sr, sc = [], []
        remaining = [nc - 1 - it for it in range(nc)]
        num_remaining, min_val, i, sink = nc, 0.0, cur, -1
        while sink == -1:
            sr.append(i)
            lowest, index = INF, -1
            for it in range(num_remaining):
                j = remaining[it]
                r = min_val + float(c[i, j]) - u[i] - v[j]
                if r < shortest[j]:
                    path[j] = i
                    shortest[j] = r
                # among equal minima the last unassigned column in scan order wins, otherwise
                # the first column in scan order
                if shortest[j] < lowest or (shortest[j] == lowest and row4col[j] == -1):
                    lowest, index = shortest[j], it
            min_val = lowest
            if min_val == INF:
                return fail(2)
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            sc.append(j)
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for i in sr:
            if i != cur:
                u[i] += min_val - shortest[col4row[i]]
        for j in sc:
            v[j] -= min_val - shortest[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    col4row = np.asarray(col4row, np.int64)
    if not transposed:
        return np.arange(nr, dtype=np.int64), col4row, 0
    order = np.argsort(col4row)
    return col4row[order], order.astype(np.int64), 0


def problems(kind, rows, cols, rng):
    """A seeded fp32 cost matrix of one of the three kinds the tests run: "random", "ints"
    (entries in {0, 1, 2}: ties everywhere) and "dup" (duplicated columns and a duplicated row,
    as the triplet matcher produces for ground-truth triplets of one class pair)."""
    if kind == "ints":
        return rng.integers(0, 3, size=(rows, cols)).astype(np.float32)
    c = rng.standard_normal((rows, cols)).astype(np.float32)
    if kind == "dup":
        for _ in range(max(1, cols // 3)):
            a, b = rng.integers(0, cols, 2)
            c[:, a] = c[:, b]
        if rows > 1:
            a, b = rng.integers(0, rows, 2)
            c[a, :] = c[b, :]
    return c
