"""Float64 restatement of the calibrated re-ranking (amar_rerank_calibrated_f32, amar_list_calibration_f64), its tolerances and the
cases of its tests.

Categories: a CSR over items, p(g|i) = 1/len_i on row i, an empty row = a neutral item.
psum(g)   = sum over the user's liked items with a row, item ascending, of 1/len_i;   p = psum / support     (float32 loops: `target32`)
n(g)      = sum over the chosen items with a row, selection order, of 1/len_i;        q = n / |S+|           (float32 loop:  `add_row32`)
C(p, S)   = sum over p(g) > 0 of p(g) log(p(g) / ((1 - a) q(g) + a p(g)))
step s    : argmax over the valid unselected t of v_t = lam * rel_t - (1 - lam) * C(p, S + {t}), ties to the smaller position; the
            raw scores decide when 1 - lam is 0 or the user has no target.

The contract fixes p, n and n + 1/len_t as float32 values, and a, 1 - a, lam, 1 - lam as the float32 argument and one float32
subtraction, so both sides start from the same numbers: the restatement evaluates C and v on float64 FROM those float32 values.

Tolerances, u = 2^-24.  The kernel's term of one cell is  p * logf(p / fmaf(1 - a, x / N, a * p)):
* x / N and a * p round once each (relative u), the fmaf once more: its two addends are positive, so the denominator is within 2u;
  p / den rounds once: the argument of the logarithm is within 3u, and so is its logarithm (|log(1 + e)| <= e (1 + e));
* logf is within 1 ulp of the logarithm of its argument (HIP documentation, "HIP math API", table of single-precision functions:
  logf, maximum error 1 ulp; the library is built without fast-math, so this is the function the kernel calls), and an ulp of y is at
  most 2u |y|;
* the product with p rounds once: u p |l|.
  e_term = 3u p (1 + |l|),  l the float64 logarithm.
Sums: a lane adds ceil(G / 64) terms in turn and the butterfly six partial sums, so a term passes through at most
d = ceil(G / 64) + 5 additions, each within u of its result: d u sum |term|.  A candidate with r cells of p > 0 adds r differences
(each subtraction within u (|new| + |old|), their sum within (r - 1) u sum (|new| + |old|)) and the result to the base sum (u |C|):
  tol_C(t) = [ sum_g e_term(n, N + 1) + sum_row (e_term(new) + e_term(old)) + u (d sum_g |term| + r sum_row (|new| + |old|) + |C_t|) ] (1 + 2^-20)
and, for a neutral candidate, [ sum_g e_term(n, N) + u d sum_g |term| ] (1 + 2^-20); the last factor holds the second-order terms.
v: rel is two subtractions and a division of values of at most 1 (3u), lam * rel rounds once (lam 4u); (1 - lam) * C32 carries
(1 - lam) tol_C and one rounding, the final subtraction another, relative to |v| <= lam + (1 - lam) C:
  tol_v(t) = (1 - lam) tol_C(t) + u (5 lam + 2 (1 - lam) C_t).
Neither is fitted to kernel output; tests/test_calibrate_gpu.py prints the worst observed error / tolerance.
"""
import numpy as np

U24 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
M_LISTS = 37
N_ITEMS = 300
N_USERS = M_LISTS                     # users == NULL needs one list per user
FULL_LISTS = 8
MAX_NEAR_TIE_LISTS = 3                # tests/diversify_ref.py
POOL_BUDGET = 4096                    # include/amar_hip.h: AMAR_CALIBRATE_POOL_BUDGET

GRID_P = (1, 2, 17, 64)
GRID_G = (1, 3, 64, 65, 1024)
GRID_LAMBDA = (0.0, 0.5, 1.0)
GRID_ALPHA = (0.01, 0.5)
LIKED_LENGTHS = (0, 1, 63, 64, 65, 200)
DENSE_CASES = ((64, 128), (17, 1024))       # dense rows: a full pool passes the staging budget


def dense_settings(P):
    """(trade_off, smoothing, k) of the dense cases: with nearly every category in every row the candidates differ by their scores
    alone, so trade_off = 0 would leave float64 itself nothing to order them by; at trade_off = 1 the scores decide and
    out_kl still goes through the rows read from memory."""
    return [(0.5, 0.01, min(10, P)), (0.5, 0.5, P), (1.0, 0.01, P)]
F32 = np.float32


def grid_ks(P):
    return sorted({P, max(1, min(10, P - 1))})


# ---- the float32 loops of the contract -------------------------------------------------------------------------------------------
def row_of(cats, i):
    ptr, ids = cats[0], cats[1]
    return ids[ptr[i]:ptr[i + 1]] if 0 <= i < len(ptr) - 1 else ids[:0]


def add_row32(acc, row):
    """acc[g] += 1/len for g in row, one float32 addition per cell (the cells of a row are distinct)."""
    if len(row):
        acc[row] = acc[row] + F32(1.0) / F32(len(row))
    return len(row) > 0


def target32(liked_items, cats, G):
    """(p float32 [G], support): psum in liked order, then one division per cell; zeros without a target."""
    psum, support = np.zeros(G, dtype=F32), 0
    for i in liked_items:
        support += int(add_row32(psum, row_of(cats, int(i))))
    return (psum / F32(support) if support else psum), support


# ---- float64 on the float32 state ---------------------------------------------------------------------------------------------------
def consts(lam, alpha):
    lam32, a32 = F32(lam), F32(alpha)
    return float(lam32), float(F32(1.0) - lam32), float(a32), float(F32(1.0) - a32)


def terms64(p, x, N, a, oma):
    """(term, |log|) of cells with p > 0 on float64 from float32 p and x."""
    p, x = p.astype(np.float64), x.astype(np.float64)
    q = x / N if N > 0 else np.zeros_like(x)
    l = np.log(p / (oma * q + a * p))
    return p * l, np.abs(l)


def e_term(p, abs_l):
    return 3.0 * U24 * p.astype(np.float64) * (1.0 + abs_l)


def c64(p, n, cnt, a, oma):
    has = p > 0
    return float(terms64(p[has], n[has], float(cnt), a, oma)[0].sum())


def rel64(scores):
    s = np.asarray(scores, dtype=np.float64)
    if len(s) == 0:
        return s
    lo, hi = s.min(), s.max()
    return (s - lo) / (hi - lo) if hi > lo else np.ones_like(s)


def step_values(p, n, cnt, rows, free, rel, lam, alpha, has_target):
    """For every pool position of `free`: (v, C, tol_v, tol_C) on float64 given the list's float32 sums n and |S+| = cnt."""
    lam_, oml, a, oma = consts(lam, alpha)
    P = len(rows)
    v, C, tol_v, tol_C = (np.full(P, -np.inf), np.zeros(P), np.zeros(P), np.zeros(P))
    if not has_target:
        for t in free:
            v[t], tol_v[t] = lam_ * rel[t], 5 * U24 * lam_
        return v, C, tol_v, tol_C
    has = np.nonzero(p > 0)[0]
    d = (len(p) + 63) // 64 + 5
    t0, l0 = terms64(p[has], n[has], float(cnt), a, oma)
    t1, l1 = terms64(p[has], n[has], float(cnt + 1), a, oma)
    base0, base1 = float(t0.sum()), float(t1.sum())
    tol0 = (float(e_term(p[has], l0).sum()) + U24 * d * float(np.abs(t0).sum())) * SLACK
    e1, abs1 = float(e_term(p[has], l1).sum()), float(np.abs(t1).sum())
    for t in free:
        row = rows[t]
        if len(row) == 0:
            C[t], tol_C[t] = base0, tol0
        else:
            cells = row[p[row] > 0]
            w = F32(1.0) / F32(len(row))
            new, ln = terms64(p[cells], n[cells] + w, float(cnt + 1), a, oma)
            old, lo = terms64(p[cells], n[cells], float(cnt + 1), a, oma)
            C[t] = base1 + float((new - old).sum())
            mag = float((np.abs(new) + np.abs(old)).sum())
            tol_C[t] = (e1 + float((e_term(p[cells], ln) + e_term(p[cells], lo)).sum())
                        + U24 * (d * abs1 + len(cells) * mag + abs(C[t]))) * SLACK
        v[t] = lam_ * rel[t] - oml * C[t]
        tol_v[t] = oml * tol_C[t] + U24 * (5 * lam_ + 2 * oml * abs(C[t]))
    return v, C, tol_v, tol_C


def _signature(p, n, rows, scores, lam, t):
    """What the kernel's arithmetic for candidate t reads, in the order it reads it: two candidates with the same signature get the
    same float32 bits (and the same float64 value), so the position settles them on both sides."""
    cells = rows[t][p[rows[t]] > 0]
    return (len(rows[t]), p[cells].tobytes(), n[cells].tobytes(), F32(scores[t]).tobytes() if F32(lam) != 0 else b'')


def greedy64(pool_row, score_row, liked_items, cats, G, lam, alpha, k, n_items=N_ITEMS):
    """Float64 greedy of one list.  Returns (items [k] -1 padded, scores [k] -inf padded, v [k], kl [k] -inf padded, near): near = at
    some step another candidate stands within tol_v(pick) + tol_v(c) of the pick without sharing its `_signature`: a list that a
    float32 evaluation may order differently."""
    pool_row = np.asarray(pool_row, dtype=np.int64)
    valid = [t for t in range(len(pool_row)) if 0 <= pool_row[t] < n_items]
    p, support = target32(liked_items, cats, G)
    has_target = support > 0
    rows = [row_of(cats, int(i)) if has_target and 0 <= i < n_items else cats[1][:0] for i in pool_row]
    scores = np.asarray(score_row, dtype=np.float64)
    rel = np.zeros(len(pool_row))
    rel[valid] = rel64(scores[valid])
    by_score = consts(lam, alpha)[1] == 0.0 or not has_target
    n, cnt, chosen, near = np.zeros(G, dtype=F32), 0, [], False
    out_i, out_s = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf)
    out_v, out_kl = np.full(k, -np.inf), np.full(k, -np.inf)
    for s in range(min(k, len(valid))):
        free = [t for t in valid if t not in chosen]
        v, C, tol_v, _ = step_values(p, n, cnt, rows, free, rel, lam, alpha, has_target)
        key = scores if by_score else v
        free = np.asarray(free, dtype=np.int64)
        best = int(free[np.lexsort((free, -key[free]))][0])
        if not by_score and not near:
            close = [c for c in free if c != best and v[best] - v[c] <= tol_v[best] + tol_v[c]]
            sig = _signature(p, n, rows, score_row, lam, best) if close else None
            near = any(_signature(p, n, rows, score_row, lam, c) != sig for c in close)
        chosen.append(best)
        out_i[s], out_s[s], out_v[s], out_kl[s] = pool_row[best], scores[best], v[best], C[best]
        cnt += int(add_row32(n, rows[best]))
    return out_i, out_s, out_v, out_kl, near


def check_steps(pool, scores, users, liked, cats, G, got_items, got_value, got_kl, lam, alpha, k, label, n_items=N_ITEMS):
    """Every step of every list, given the device's own prefix: the pick is a valid unselected candidate whose float64 v is within
    tol_v(pick) + tol_v(best) of the float64 maximum (the best score itself, the smaller position on a tie, where the scores decide),
    out_value is within tol_v and out_kl within tol_C of the pick's float64 values; the padding is -1 / -inf.  Returns the largest
    error / tolerance seen (out_value, out_kl)."""
    worst_v = worst_c = 0.0
    by_lam = consts(lam, alpha)[1] == 0.0
    for j in range(len(pool)):
        u = int(users[j])
        ok = 0 <= u < len(liked[0]) - 1
        valid = [t for t in range(pool.shape[1]) if ok and 0 <= pool[j, t] < n_items]
        p, support = target32(liked[1][liked[0][u]:liked[0][u + 1]] if ok else [], cats, G)
        has_target = support > 0
        rows = [row_of(cats, int(i)) if has_target and 0 <= i < n_items else cats[1][:0] for i in pool[j]]
        rel = np.zeros(pool.shape[1])
        rel[valid] = rel64(scores[j, valid])
        where = {int(pool[j, t]): t for t in valid}
        n, cnt, chosen = np.zeros(G, dtype=F32), 0, []
        for s in range(k):
            if s >= len(valid):
                assert got_items[j, s] == -1 and np.isneginf(got_value[j, s]) and np.isneginf(got_kl[j, s]), '{}: list {} step {} padding'.format(label, j, s)
                continue
            t = where.get(int(got_items[j, s]))
            assert t is not None and t not in chosen, '{}: list {} step {} picks {}'.format(label, j, s, got_items[j, s])
            free = [c for c in valid if c not in chosen]
            v, C, tol_v, tol_C = step_values(p, n, cnt, rows, free, rel, lam, alpha, has_target)
            free = np.asarray(free, dtype=np.int64)
            if by_lam or not has_target:
                best = free[np.lexsort((free, -scores[j, free].astype(np.float64)))][0]
                assert t == best, '{}: list {} step {} picks position {} not {}'.format(label, j, s, t, best)
            else:
                best = free[np.argmax(v[free])]
                assert v[best] - v[t] <= tol_v[t] + tol_v[best], '{}: list {} step {}: v {} against the best {}'.format(label, j, s, v[t], v[best])
            err_v, err_c = abs(float(got_value[j, s]) - v[t]), abs(float(got_kl[j, s]) - C[t])
            assert err_v <= tol_v[t], '{}: list {} step {}: out_value off by {} (tol {})'.format(label, j, s, err_v, tol_v[t])
            assert err_c <= tol_C[t], '{}: list {} step {}: out_kl off by {} (tol {})'.format(label, j, s, err_c, tol_C[t])
            worst_v = max(worst_v, err_v / tol_v[t] if tol_v[t] > 0 else 0.0)
            worst_c = max(worst_c, err_c / tol_C[t] if tol_C[t] > 0 else 0.0)
            chosen.append(t)
            cnt += int(add_row32(n, rows[t]))
    return worst_v, worst_c


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# Seeds, chosen once: per case the smallest salt at which the float64 reference alone has at most MAX_NEAR_TIE_LISTS lists with a
# near-tie for every trade-off and smoothing of the grid at k = P (tests/test_calibrate_cpu.py asserts it; nothing is reseeded at run time).
SEED_SALT = {(17, 3, False): 1, (17, 65, False): 1, (17, 1024, False): 1, (64, 3, False): 2, (64, 64, False): 5, (64, 65, False): 1,
             (64, 1024, False): 4}
# (full lists, longest other list) at trade_off = 0 where the default (FULL_LISTS, P) cannot meet the cap under any of 12 seeds: a
# list of n candidates meets about n^2 / 2 gaps, and with many categories the steps stand closest together when the scores do not
# count.  Where they count (trade_off > 0) these cells run with the default lengths too (`grid_case`).
LIST_LENGTHS_AT = {(17, 1024): (3, 10), (64, 65): (3, 24), (64, 1024): (3, 16)}


SEED_SALT_FULL = {}                   # the same cells with full-length lists, used where the scores count (trade_off > 0)


def case_seed(P, G, dense, short=True):
    salt = SEED_SALT.get((P, G, dense), 0) if short else SEED_SALT_FULL.get((P, G), 0)
    return 7919 * P + 101 * G + (1 if dense else 0) + 1000003 * salt + (500009 if not short else 0)


def planted_case(P, G, dense=False, m=M_LISTS, n_items=N_ITEMS, short=True):
    """The data of the kernel grid: (cats = (ptr, ids, max_row), liked = (ptr, items), pool [m, P], scores [m, P], users [m]).
    Category rows: item 0 empty, item 1 one category, item 2 all G, about one item in six neutral, the others 1..min(G, 6) categories
    drawn with Zipf weights
    (`dense`: G - 2..G, so that a pool's rows pass the LDS staging budget).  Liked lists: user u has LIKED_LENGTHS[u % 6] items; user
    8 likes neutral items only, as does user 7 (a single one).  Pools of distinct items with unsorted scores: list 0 has no valid
    entry, list 1 a single one, list 2 holes between its entries, list 3 holds items 0, 1, 2 where P allows, the last FULL_LISTS
    are full, the others a random valid prefix (`short`: the lengths of LIST_LENGTHS_AT where the cell has an entry)."""
    short = short and (P, G) in LIST_LENGTHS_AT and not dense
    rng = np.random.default_rng(case_seed(P, G, dense, short or (P, G) not in LIST_LENGTHS_AT or dense))
    longest = max(1, min(G - 1, 6))                                     # item 2 alone holds every category: it moves q as a neutral item does
    lens = np.where(rng.random(n_items) < 1.0 / 6, 0,
                    rng.integers(max(1, G - 2), G + 1, size=n_items) if dense else rng.integers(1, longest + 1, size=n_items))
    lens[:3] = (0, 1, G)
    ptr = np.zeros(n_items + 1, dtype=np.int32)
    np.cumsum(lens, out=ptr[1:])
    # popular and rare categories, as genres are: a target with distinct cells (equal ones make candidates that float64 cannot order)
    weight = 1.0 / np.arange(1, G + 1)
    ids = np.concatenate([np.sort(rng.choice(G, size=l, replace=False, p=weight / weight.sum())) for l in lens]).astype(np.int32)
    neutral = np.nonzero(lens == 0)[0]
    l_ptr, l_items = np.zeros(N_USERS + 1, dtype=np.int32), []
    for u in range(N_USERS):
        items = np.sort(rng.choice(n_items, size=LIKED_LENGTHS[u % len(LIKED_LENGTHS)], replace=False))
        if u == 8:
            items = neutral
        if u == 7:
            items = neutral[:1]
        l_items.append(items)
        l_ptr[u + 1] = l_ptr[u] + len(items)
    l_items = np.concatenate(l_items).astype(np.int32)
    pool = np.full((m, P), -1, dtype=np.int32)
    scores = rng.normal(0, 1, size=(m, P)).astype(np.float32)
    for j in range(m):
        full, longest_list = LIST_LENGTHS_AT[(P, G)] if short else (FULL_LISTS, P)
        nv = P if j >= m - full else int(rng.integers(1, min(P, longest_list) + 1))
        nv = {0: 0, 1: 1}.get(j, nv)
        # with one category a neutral candidate and one with the category move q alike: lists 3 and 4 alone mix them there
        rows = rng.choice(n_items if G > 1 or j == 4 else np.nonzero(lens > 0)[0], size=nv, replace=False)
        if j == 3:
            rest = [r for r in rng.permutation(n_items).tolist() if r not in (0, 1, 2)]
            rows = np.array((rest[:1] + [0, 1, 2] + rest[1:])[:P] if P > 3 else [0, 1, 2][:P], dtype=np.int64)
        if j == 2:
            at = np.sort(rng.choice(P, size=min(P, max(1, len(rows) // 2)), replace=False))
            pool[j, at] = rows[:len(at)]
        else:
            pool[j, :len(rows)] = rows
    return (ptr, ids, int(lens.max())), (l_ptr, l_items), pool, scores, np.arange(m, dtype=np.int32) % N_USERS


def grid_case(P, G, lam):
    """The case of one grid cell at one trade-off: the shortened lists of LIST_LENGTHS_AT at trade_off = 0 only."""
    return planted_case(P, G, short=lam == 0)


def liked_of(liked, u):
    return liked[1][liked[0][u]:liked[0][u + 1]]


def near_tie_lists(case, G, lam, alpha, k):
    """How many lists of a case the float64 reference itself cannot settle (greedy64's near)."""
    cats, liked, pool, scores, users = case
    return sum(greedy64(pool[j], scores[j], liked_of(liked, int(users[j])), cats, G, lam, alpha, k)[4] for j in range(len(pool)))


def two_genre_case():
    """Hand-worked: genres 0 and 1; items 0..9 are genre 0 (drama), 10..19 genre 1 (comedy), 20..23 neutral.  User 0 likes seven
    dramas and three comedies; user 1 likes neutral items only; user 2 nothing."""
    ptr = np.concatenate([np.arange(21), [20, 20, 20, 20]]).astype(np.int32)
    ids = np.array([0] * 10 + [1] * 10, dtype=np.int32)
    liked_ptr = np.array([0, 10, 12, 12], dtype=np.int32)
    liked_items = np.array([0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 20, 21], dtype=np.int32)
    return (ptr, ids, 1), (liked_ptr, liked_items)
