"""Float64 restatement of the diversified re-ranking (amar_rerank_mmr_f32, amar_list_diversity_f64), its tolerances and the cases of
its tests.

sim(a, b) = sum_c T[a, c] T[b, c]                                        (dot)
          = that * inv_norm(T[a]) * inv_norm(T[b])                       (cosine), inv_norm(x) = 1/sqrt(sum x^2), 0 for a zero row
rel_t     = (r_t - r_min) / (r_max - r_min) over the list's valid entries, 1 everywhere when r_max == r_min
step 0    : argmax rel_t;   step s >= 1: argmax over the valid unselected t of
v_t       = lam * rel_t - (1 - lam) * max_{u selected} sim(t, u),   ties to the smaller pool position;   v_0 = lam * rel
ILD       = mean over the pairs a < b of the list's valid items of 1 - sim(a, b), 0 below two items.

Tolerances.  tol_sim is similar_ref.score_tolerance: (d + 8) 2^-24 ||a|| ||b|| (the norms being 1 for cosine).
tol_v bounds |f32 v - float64 v| of one candidate given the same selected set:
    tol_v = (1 - lam) tol_sim + 8 * 2^-24 * (lam + (1 - lam) |sim|)
* rel is one subtraction, one subtraction and one division of f32 values: three roundings, each relative to a value of at most 1,
  so |rel32 - rel| <= 3u; times lam (the product's own rounding is the fourth u):            lam * 4u
* the penalty is the maximum of f32 sims, each within tol_sim of float64, so the maximum is too; times (1 - lam), itself
  rounded once (1 - lam in f32) and the product once:                                        (1 - lam) (tol_sim + 2u |sim|)
* the final subtraction rounds once, relative to |v| <= lam + (1 - lam) |sim|:               u (lam + (1 - lam) |sim|)
Summed: (1 - lam) tol_sim + u (5 lam + 3 (1 - lam) |sim|) <= the bound above (8u leaves room for lam itself being rounded to f32).
|sim| is taken as the largest |sim| of the candidate against the selected set.
"""
import numpy as np

from tests import similar_ref

U24 = similar_ref.U24
M_LISTS = 37
N_ROWS = 300
FULL_LISTS = 8
# (full lists, longest other list) where the default (FULL_LISTS, P) cannot meet the cap under any of 80 seeds: at P = 64, d = 512 the
# cosine's tol_sim is largest against the similarities' range, and a list of n candidates meets about n^2 / 2 gaps
LIST_LENGTHS_AT = {(64, 512, 'cosine'): (3, 24)}
MAX_NEAR_TIE_LISTS = 3           # MAX_NEAR_TIE_QUERIES of tests/test_similar_gpu.py

GRID_P = (1, 2, 5, 16, 17, 33, 64)
GRID_D = (4, 20, 48, 132, 512)
GRID_LAMBDA = (0.0, 0.3, 1.0)
GRID_METRIC = ('dot', 'cosine')


def grid_ks(P):
    return sorted({1, min(10, P), P})


def sim(T, metric):
    """The [n, n] similarity grid of the rows of T on float64."""
    return similar_ref.nearest64(T, T, metric)


def sim_tolerance(T, metric):
    return similar_ref.score_tolerance(T, T, metric)


def v_tolerance(lam, tol_sim, abs_sim):
    return (1.0 - lam) * tol_sim + 8 * U24 * (lam + (1.0 - lam) * abs_sim)


def rel64(scores):
    s = np.asarray(scores, dtype=np.float64)
    if len(s) == 0:
        return s
    lo, hi = s.min(), s.max()
    return (s - lo) / (hi - lo) if hi > lo else np.ones_like(s)


def step_values(rel, grid, items, selected, lam):
    """v of every pool position given the selected positions (in order): (v [n], |sim| bound [n], tol_sim index helper)."""
    if not selected:
        return lam * rel, np.zeros(len(rel))
    pen_all = grid[np.ix_(items, items[selected])]
    pen = pen_all.max(axis=1)
    return lam * rel - (1.0 - lam) * pen, np.abs(pen_all).max(axis=1)


def mmr64(pool_items, pool_scores, grid, lam, k):
    """Float64 greedy of one list.  pool_items [P] (-1 padded, valid prefix), grid = sim(T, metric).  Returns (positions chosen
    [n], items [k] -1 padded, scores [k] -inf padded, v [k] -inf padded, gaps [n]: v of the pick minus v of the runner-up, inf when
    there is none)."""
    pool_items = np.asarray(pool_items, dtype=np.int64)
    scores = np.asarray(pool_scores, dtype=np.float64)
    n_valid = int((pool_items >= 0).sum())
    items = pool_items[:n_valid]
    rel = rel64(scores[:n_valid])
    chosen, vs, gaps = [], [], []
    for s in range(min(k, n_valid)):
        v, _ = step_values(rel, grid, items, chosen, lam)
        key = rel if s == 0 else v
        free = np.array([t for t in range(n_valid) if t not in chosen], dtype=np.int64)
        order = free[np.lexsort((free, -key[free]))]
        chosen.append(int(order[0]))
        vs.append(float(v[order[0]]))
        gaps.append(float(key[order[0]] - key[order[1]]) if len(order) > 1 else np.inf)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s = np.full(k, -np.inf)
    out_v = np.full(k, -np.inf)
    out_i[:len(chosen)] = items[chosen]
    out_s[:len(chosen)] = scores[chosen]
    out_v[:len(chosen)] = vs
    return chosen, out_i, out_s, out_v, np.asarray(gaps)


def ild64(items, grid):
    """ILD of one list of rows (-1 entries skipped) on the float64 grid, and the number of valid items."""
    items = np.asarray(items, dtype=np.int64)
    items = items[items >= 0]
    n = len(items)
    if n < 2:
        return 0.0, n
    g = grid[np.ix_(items, items)]
    return float((1.0 - g[np.triu_indices(n, 1)]).mean()), n


# Seeds, chosen once: per case the smallest salt at which the float64 reference alone has at most MAX_NEAR_TIE_LISTS lists with a
# near-tie, for every trade-off of the grid at k = P (tests/test_diversify_cpu.py asserts it; nothing is reseeded at run time).
SEED_SALT = {(64, 4, 'cosine'): 1, (64, 48, 'cosine'): 1, (64, 512, 'cosine'): 1}


def case_seed(P, d, metric):
    return 7919 * P + 101 * d + (1 if metric == 'cosine' else 0) + 1000003 * SEED_SALT.get((P, d, metric), 0)


def planted_case(P, d, metric, m=M_LISTS, n_rows=N_ROWS):
    """The data of the kernel grid: T [n_rows, d] with row 3 all zero and rows 1, 150 identical; pools [m, P] of distinct rows with
    unsorted scores.  List 0 has no valid entry, list 1 a single one, list 2 min(P, 3) (fewer than k where k is larger), list 3 holds
    the zero row and both identical rows where P allows, the last FULL_LISTS are full, the others a random valid prefix (a list of n
    candidates meets about n^2 / 2 gaps, so full lists alone would put the float64 reference past the near-tie cap at P = 64, d = 512)."""
    rng = np.random.default_rng(case_seed(P, d, metric))
    # item vectors as a recommender learns them: a few latent directions plus noise, so that similarities spread over the whole
    # range (for independent normal rows they crowd within 1 / sqrt(d) of zero and f32 cannot tell the candidates apart)
    rank = min(d, 3)
    T = (rng.normal(0, 1, size=(n_rows, rank)) @ rng.normal(0, 1, size=(rank, d)) / np.sqrt(rank)
         + 0.05 * rng.normal(0, 1, size=(n_rows, d))).astype(np.float32)
    T[3] = 0
    T[150] = T[1]
    pool = np.full((m, P), -1, dtype=np.int32)
    scores = rng.normal(0, 1, size=(m, P)).astype(np.float32)
    for j in range(m):
        full, longest = LIST_LENGTHS_AT.get((P, d, metric), (FULL_LISTS, P))
        n = P if j >= m - full else int(rng.integers(1, min(P, longest) + 1))
        n = {0: 0, 1: 1, 2: min(P, 3)}.get(j, n)
        rows = rng.choice(n_rows, size=n, replace=False)
        if j == 3:
            plant = [3, 1, 150]
            rest = [r for r in rng.permutation(n_rows).tolist() if r not in plant]
            rows = np.array((rest[:1] + plant + rest[1:])[:P] if P > 3 else plant[:P], dtype=np.int64)
            n = len(rows)
        pool[j, :n] = rows
    return T, pool, scores


def exact_case(P=24, d=8, m=M_LISTS, n_rows=40, seed=3):
    """Small-integer vectors and dyadic scores: with metric 'dot' and a dyadic lam every v is exact in float32, ties abound."""
    rng = np.random.default_rng(seed)
    T = rng.integers(-2, 3, size=(n_rows, d)).astype(np.float32)
    pool = np.full((m, P), -1, dtype=np.int32)
    scores = np.zeros((m, P), dtype=np.float32)
    for j in range(m):
        n = int(rng.integers(1, P + 1))
        pool[j, :n] = rng.choice(n_rows, size=n, replace=False)
        # scores in {0, 1/4, ..., 1} with both ends present: rel is the score itself
        s = rng.integers(0, 5, size=n).astype(np.float32) / 4
        if n >= 2:
            s[rng.integers(0, n)] = 0.0
            s[(int(np.argmin(s)) + 1) % n] = 1.0
        scores[j, :n] = s
    return T, pool, scores


def greedy_with_near_tie(pool_row, score_row, grid, tol, lam, k):
    """(float64 items [k], near): near = at some float64 step s >= 1 another candidate c stands within tol_v(pick) + tol_v(c)
    (each candidate's own tol_v, at most 2 tol_v) below the pick without tying it: a list that an f32 evaluation may order
    differently.  Step 0 compares the scores themselves and an exact tie goes to the position: neither counts."""
    chosen, out_items, _, _, _ = mmr64(pool_row, score_row, grid, lam, k)
    n_valid = int((np.asarray(pool_row) >= 0).sum())
    items = np.asarray(pool_row[:n_valid], dtype=np.int64)
    rel = rel64(np.asarray(score_row, dtype=np.float64)[:n_valid])
    for s in range(1, len(chosen)):
        v, abs_sim = step_values(rel, grid, items, chosen[:s], lam)
        tol_v = v_tolerance(lam, tol[np.ix_(items, items[chosen[:s]])].max(axis=1), abs_sim)
        free = np.array([c for c in range(n_valid) if c not in chosen[:s + 1]], dtype=np.int64)
        gap = v[chosen[s]] - v[free]
        if np.any((gap > 0) & (gap <= tol_v[chosen[s]] + tol_v[free])):
            return out_items, True
    return out_items, False


def near_tie_lists(T, pool, scores, metric, lam, k):
    """How many lists of a case the float64 reference itself cannot settle (greedy_with_near_tie)."""
    grid, tol = sim(T, metric), sim_tolerance(T, metric)
    return sum(greedy_with_near_tie(pool[j], scores[j], grid, tol, lam, k)[1] for j in range(len(pool)))


def check_steps(pool, scores, got_items, got_mmr, grid, tol, lam, k, label):
    """Every step of every list, given the device's own prefix: the pick is a valid unselected candidate whose float64 v is within
    tol_v(pick) + tol_v(best) <= 2 tol_v of the float64 maximum (step 0: the best score itself, the smaller position on a tie), and
    out_mmr is within tol_v of the pick's float64 v; the padding is -1 / -inf.  Returns the largest |out_mmr - v| / tol_v seen."""
    worst = 0.0
    for j in range(len(pool)):
        n_valid = int((pool[j] >= 0).sum())
        items = pool[j, :n_valid].astype(np.int64)
        rel = rel64(scores[j, :n_valid])
        where = {int(r): t for t, r in enumerate(items.tolist())}
        chosen = []
        for s in range(k):
            if s >= n_valid:
                assert got_items[j, s] == -1 and np.isneginf(got_mmr[j, s]), '{}: list {} step {} padding'.format(label, j, s)
                continue
            t = where.get(int(got_items[j, s]))
            assert t is not None and t not in chosen, '{}: list {} step {} picks {}'.format(label, j, s, got_items[j, s])
            v, abs_sim = step_values(rel, grid, items, chosen, lam)
            tol_sim = tol[np.ix_(items, items[chosen])].max(axis=1) if chosen else np.zeros(n_valid)
            tol_v = v_tolerance(lam, tol_sim, abs_sim)
            free = np.array([c for c in range(n_valid) if c not in chosen], dtype=np.int64)
            if s == 0:
                best = free[np.lexsort((free, -scores[j, free].astype(np.float64)))][0]
                assert t == best, '{}: list {} step 0 picks position {} not {}'.format(label, j, t, best)
            else:
                best = free[np.argmax(v[free])]
                assert v[best] - v[t] <= tol_v[t] + tol_v[best], '{}: list {} step {}: v {} against the best {}'.format(
                    label, j, s, v[t], v[best])
            err = abs(float(got_mmr[j, s]) - v[t])
            assert err <= tol_v[t], '{}: list {} step {}: out_mmr off by {} (tol {})'.format(label, j, s, err, tol_v[t])
            worst = max(worst, err / tol_v[t] if tol_v[t] > 0 else 0.0)
            chosen.append(t)
    return worst
