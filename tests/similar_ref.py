"""Float64 restatement of the similarity search (amar_nearest_f32) and the list checker of its tests.

score(j, i) = sum_c Q[j, c] T[i, c]                                      (dot)
            = that * inv_norm(Q[j]) * inv_norm(T[i])                     (cosine), inv_norm(x) = 1/sqrt(sum x^2), 0 for a zero row
so a zero row scores 0 against everything, never NaN.  Lists: score descending, table row ascending on ties, excluded rows
absent, padded with -1 / -inf.
"""
import numpy as np

U24 = 2.0 ** -24              # unit roundoff of float32


def inv_norm64(x):
    s = (np.asarray(x, dtype=np.float64) ** 2).sum(axis=1)
    return np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)


def nearest64(Q, T, metric):
    """The [m, n] score grid on float64."""
    if metric not in ('dot', 'cosine'):
        raise ValueError(metric)
    grid = np.asarray(Q, dtype=np.float64) @ np.asarray(T, dtype=np.float64).T
    if metric == 'cosine':
        grid = grid * inv_norm64(Q)[:, None] * inv_norm64(T)[None, :]
    return grid


def score_tolerance(Q, T, metric):
    """[m, n] bound on |f32 kernel score - float64 score|: (d + 8) 2^-24 ||q|| ||t||, the norms being 1 for cosine.  An f32 sum of d
    products is within d u sum|q_c t_c| <= d u ||q|| ||t|| (Cauchy-Schwarz) of the exact one; cosine adds the two inverse norms
    (a sum of d squares, a square root and a division each, taken relative to the norm) and the two products with them: 8 u is
    the room for those, rounded up."""
    d = np.asarray(Q).shape[1]
    if metric == 'cosine':
        return np.full((len(Q), len(T)), (d + 8) * U24)
    nq = np.sqrt((np.asarray(Q, dtype=np.float64) ** 2).sum(axis=1))
    nt = np.sqrt((np.asarray(T, dtype=np.float64) ** 2).sum(axis=1))
    return (d + 8) * U24 * nq[:, None] * nt[None, :]


def topk64(grid_row, excluded, k):
    """(rows [k] -1 padded, scores [k] -inf padded) of one query on float64 scores."""
    avail = np.array([i for i in range(len(grid_row)) if i not in excluded], dtype=np.int64)
    order = np.lexsort((avail, -grid_row[avail])) if len(avail) else np.zeros(0, dtype=np.int64)
    rows = np.full(k, -1, dtype=np.int64)
    scores = np.full(k, -np.inf)
    n = min(k, len(avail))
    rows[:n] = avail[order][:n]
    scores[:n] = grid_row[avail][order][:n]
    return rows, scores


def check_lists(queries, rows, scores, want64, excl, k, label, tol_grid=None, base=0):
    """The logic of tests/test_recommend_gpu.py:_check_lists with a per-pair score tolerance.  queries [m]: row of want64 for every
    list; rows [m, k]: table rows (+ base), -1 padded; excl: {list position -> set of excluded table rows}.  Asserts padding,
    no duplicate / excluded row, order, scores within tol_grid (default 1e-6) of float64; a list may differ from the float64
    ranking only where float64 gaps inside its first k + 1 ranks are within twice the observed score error.  Returns
    (number of lists that differ, largest score error)."""
    queries, rows, scores = np.asarray(queries), np.asarray(rows), np.asarray(scores)
    n = want64.shape[1]
    rows = np.where(rows >= 0, rows - base, -1)
    valid = rows >= 0
    picked = want64[queries[:, None], np.maximum(rows, 0)]
    bound = np.full(want64.shape, 1e-6) if tol_grid is None else tol_grid
    err_grid = np.abs(scores.astype(np.float64) - picked)
    assert np.all(err_grid[valid] <= bound[queries[:, None], np.maximum(rows, 0)][valid]), \
        "{}: scores {} from float64".format(label, float(err_grid[valid].max()))
    err = float(err_grid[valid].max()) if valid.any() else 0.0
    tol = 2 * err + 1e-12
    differing = 0
    for r, q in enumerate(queries.tolist()):
        ex = excl.get(r, set())
        avail = np.array([i for i in range(n) if i not in ex], dtype=np.int64)
        n_valid = min(k, len(avail))
        assert valid[r, :n_valid].all() and not valid[r, n_valid:].any(), "{}: list {} padding".format(label, r)
        assert np.all(np.isneginf(scores[r, n_valid:])), label
        got = rows[r, :n_valid]
        assert len(set(got.tolist())) == n_valid and not (set(got.tolist()) & ex), "{}: duplicate or excluded row".format(label)
        s = scores[r, :n_valid]
        assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (got[:-1] < got[1:]))), "{}: order".format(label)
        if n_valid == 0:
            continue
        sc = want64[q, avail]
        order = np.lexsort((avail, -sc))
        o_rows, o_s = avail[order], sc[order]
        assert np.abs(want64[q, got] - o_s[:n_valid]).max() <= tol, "{}: list {} differs beyond near-ties".format(label, r)
        gaps = -np.diff(o_s[:min(k + 1, len(o_s))])
        near = np.any((gaps > 0) & (gaps <= tol))
        if not near:
            assert np.array_equal(got, o_rows[:n_valid]), "{}: list {} without near-tie differs".format(label, r)
        elif not np.array_equal(got, o_rows[:n_valid]):
            differing += 1
    return differing, err


def nearest32(Q, T, metric, k, excl):
    """An f32 numpy evaluation of the same search (float32 products and norms, numpy's own summation order): what the seed check of
    the GPU test runs on the CPU.  Returns (rows [m, k], scores float32 [m, k])."""
    Q, T = np.asarray(Q, dtype=np.float32), np.asarray(T, dtype=np.float32)
    grid = Q @ T.T
    if metric == 'cosine':
        def inv(x):
            s = (x * x).sum(axis=1, dtype=np.float32)
            return np.where(s > 0, np.float32(1) / np.sqrt(np.where(s > 0, s, np.float32(1))), np.float32(0)).astype(np.float32)
        grid = (grid * inv(Q)[:, None]) * inv(T)[None, :]
    rows = np.full((len(Q), k), -1, dtype=np.int64)
    scores = np.full((len(Q), k), -np.inf, dtype=np.float32)
    for j in range(len(Q)):
        r, s = topk64(grid[j].astype(np.float64), excl.get(j, set()), k)
        rows[j], scores[j] = r, s.astype(np.float32)
    return rows, scores


def planted_case(n_rows, d, metric, seed, m=37):
    """The data of the kernel test: queries Q [m, d] (row m - 1 all zero), table T [n_rows, d] with two duplicates of row 1 and one
    all-zero row planted where the table is large enough, and the exclusion sets {query -> rows}: query 0 excludes every row,
    query 1 all but 3, the others a random segment."""
    rng = np.random.default_rng(seed)
    Q = rng.normal(0, 1, size=(m, d)).astype(np.float32)
    T = rng.normal(0, 1, size=(n_rows, d)).astype(np.float32)
    Q[m - 1] = 0
    if n_rows > 4:
        T[n_rows // 2] = T[1]
        T[n_rows - 1] = T[1]
        T[3] = 0
    excl = {0: set(range(n_rows)), 1: set(range(3, n_rows))}
    for j in range(2, m):
        excl[j] = set(rng.choice(n_rows, size=min(n_rows, int(rng.integers(0, 40))), replace=False).tolist())
    return Q, T, excl
