"""Float64 restatement of the explanations (amar_explain_f32), its tolerances and the cases of its tests.

For target i of user u, with sim as in tests/similar_ref.py (dot, or cosine with a zero row scoring 0):
evidence   : the items j of liked(u), j != i, by sim(i, j) descending, item row ascending on ties; the first E.
properties : every p of props(i) with support(p) = |{j in liked(u), j != i, p in props(j)}| > 0, by
             score(p) = w_p * sum_j max(sim(i, j), 0) descending, property index ascending on ties; the first Q.

Tolerances.  tol_sim is similar_ref.score_tolerance: (d + 8) 2^-24 ||a|| ||b|| (the norms being 1 for cosine); the derivation is
the one tests/diversify_ref.py reuses.  max(., 0) does not widen it.  A property score is an f32 sum of n_j such terms, each within
tol_sim of float64, and one product with w_p (a float32 value that the reference reads as it is):
    tol_p = w_p * sum_j tol_sim(i, j) + (n_j + 2) 2^-24 |score|
(n_j - 1 additions and the product round once each, relative to at most the partial sums <= |score| / w_p: all terms are >= 0).

Near-ties.  Entry r of a ranking is a near-tie when its float64 gap to a neighbour in the ranking, at or across the cut
(ranks r - 1 and r + 1, the latter also when r + 1 is the first rank cut off), is within the sum of the two entries' tolerances
("2 tol").  Exactly equal float64 values are not near-ties where the float32 values are certain to be equal too: two similarities
that are both exactly 0 (a zero row), two property scores whose terms are all sign-certain (|sim| > tol_sim or sim == 0) — equal
scores then come from the same liked items and the same weight, or are both 0.
"""
import numpy as np

from tests import similar_ref

U24 = similar_ref.U24
M_LISTS, N_USERS, N_ITEMS, N_PROPS = 37, 23, 320, 3000
ZERO_ROW = 7
LIKED_LADDER = (0, 1, 15, 16, 17, 63, 64, 65, 200)
TARGET_ROWS = (0, 1, 40, 256)
NEAR_TIE_CAP = 0.02

GRID_D = (4, 20, 64, 132)
GRID_K = (1, 10, 17, 64)
GRID_EQ = ((1, 0), (3, 3), (16, 16))
GRID_METRIC = ('dot', 'cosine')
# seed per (d, K, metric) where the default seed leaves the float64 reference itself above the near-tie cap
SEED = 11
SEED_AT = {}


def case_seed(d, K, metric):
    return SEED_AT.get((d, K, metric), SEED)


def idf(df, n_items):
    df = np.asarray(df, dtype=np.float64)
    return np.where(df > 0, np.log(float(n_items) / np.maximum(df, 1.0)), 0.0).astype(np.float32)


def sim_grid(T, metric):
    return similar_ref.nearest64(T, T, metric)


def sim_tolerance(T, metric):
    return similar_ref.score_tolerance(T, T, metric)


def _flags(values, tols, certain, n_cut):
    """Near-tie flags of the first n_cut entries of a ranking (values descending)."""
    n = len(values)
    flag = np.zeros(min(n_cut, n), dtype=bool)
    for r in range(min(n_cut, n - 1)):
        gap = values[r] - values[r + 1]
        if gap <= tols[r] + tols[r + 1] and not (gap == 0 and certain[r] and certain[r + 1]):
            flag[r] = True
            if r + 1 < len(flag):
                flag[r + 1] = True
    return flag


def explain_target(i, liked, grid, tol_grid, prop_rows, weight, E, Q):
    """One (user, item) pair on float64.  liked: the user's item rows, ascending; prop_rows: list of property index arrays per item
    or None.  Returns a dict: ev_items / ev_sims (whole ranking), ev_flag [min(E, n)], and with properties prop_ids / prop_scores /
    prop_support (whole ranking of the supported ones), prop_tol, prop_flag [min(Q, n)], plus score_of / support_of / tol_of: dicts
    over every property of the target."""
    out = {}
    js = np.asarray([j for j in liked if j != i], dtype=np.int64)
    s = grid[i, js] if len(js) else np.zeros(0)
    order = np.lexsort((js, -s)) if len(js) else np.zeros(0, dtype=np.int64)
    out['ev_items'], out['ev_sims'] = js[order], s[order]
    tol = tol_grid[i, js][order] if len(js) else np.zeros(0)
    out['ev_flag'] = _flags(out['ev_sims'], tol, out['ev_sims'] == 0, E)
    if prop_rows is None:
        return out
    mine = np.asarray(prop_rows[i], dtype=np.int64)
    score_of, support_of, tol_of, certain_of = {}, {}, {}, {}
    if len(mine) and len(js):
        member = np.zeros((len(js), len(mine)), dtype=bool)
        for a, j in enumerate(js):
            member[a] = np.isin(mine, prop_rows[j], assume_unique=True)
        pos = np.maximum(s, 0.0)
        tj = tol_grid[i, js]
        sure = (np.abs(s) > tj) | (s == 0)
        support = member.sum(0)
        w = weight[mine].astype(np.float64)
        score = w * (member * pos[:, None]).sum(0)
        tolp = w * (member * tj[:, None]).sum(0) + (support + 2) * U24 * np.abs(score)
        cert = (member <= sure[:, None]).all(0)
        for a, p in enumerate(mine):
            score_of[int(p)], support_of[int(p)], tol_of[int(p)], certain_of[int(p)] = score[a], int(support[a]), tolp[a], bool(cert[a])
    else:
        for p in mine:
            score_of[int(p)], support_of[int(p)], tol_of[int(p)], certain_of[int(p)] = 0.0, 0, 0.0, True
    have = np.asarray([p for p in mine if support_of[int(p)] > 0], dtype=np.int64)
    sc = np.asarray([score_of[int(p)] for p in have])
    order = np.lexsort((have, -sc)) if len(have) else np.zeros(0, dtype=np.int64)
    out['prop_ids'], out['prop_scores'] = have[order], sc[order]
    out['prop_support'] = np.asarray([support_of[int(p)] for p in have[order]], dtype=np.int64)
    out['prop_tol'] = np.asarray([tol_of[int(p)] for p in have[order]])
    out['prop_flag'] = _flags(out['prop_scores'], out['prop_tol'], np.asarray([certain_of[int(p)] for p in have[order]], dtype=bool), Q)
    out['score_of'], out['support_of'], out['tol_of'] = score_of, support_of, tol_of
    return out


def explain_list(targets, liked, grid, tol_grid, prop_rows, weight, E, Q):
    """explain_target for every entry of one list (None for a -1 entry)."""
    return [None if i < 0 else explain_target(int(i), liked, grid, tol_grid, prop_rows, weight, E, Q) for i in targets]


def padded(ref, E, Q):
    """The [E] / [Q] arrays the kernel writes for one target: (evidence, sims, props, scores, support), float64 values."""
    ev, es = np.full(E, -1, dtype=np.int64), np.full(E, -np.inf)
    pr, ps, pc = np.full(Q, -1, dtype=np.int64), np.full(Q, -np.inf), np.zeros(Q, dtype=np.int64)
    if ref is not None:
        n = min(E, len(ref['ev_items']))
        ev[:n], es[:n] = ref['ev_items'][:n], ref['ev_sims'][:n]
        if 'prop_ids' in ref:
            n = min(Q, len(ref['prop_ids']))
            pr[:n], ps[:n], pc[:n] = ref['prop_ids'][:n], ref['prop_scores'][:n], ref['prop_support'][:n]
    return ev, es, pr, ps, pc


def near_tie_rate(refs, E, Q):
    """(flagged, entries) over the written (list, target, rank) entries of a case: refs is a list (per list) of explain_list results."""
    flagged = entries = 0
    for per_list in refs:
        for ref in per_list:
            if ref is None:
                continue
            flagged += int(ref['ev_flag'][:E].sum())
            entries += min(E, len(ref['ev_items']))
            if 'prop_ids' in ref and Q:
                flagged += int(ref['prop_flag'][:Q].sum())
                entries += min(Q, len(ref['prop_ids']))
    return flagged, entries


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if len(rows) and ptr[-1] else np.zeros(0, dtype=np.int64)
    return ptr.astype(np.int32), flat.astype(np.int32)


def kernel_case(d, K, metric, seed=None):
    """The data of the kernel grid: T [N_ITEMS, d] float32 with one zero row, 23 users whose liked lists walk LIKED_LADDER, 37
    lists of K targets (some inside their user's liked list, -1 entries inside and at the end of some), property rows of
    TARGET_ROWS entries for the first half of the items, 0..30 for the rest and 300 for four of them, IDF weights."""
    seed = case_seed(d, K, metric) if seed is None else seed
    rng = np.random.default_rng([seed, d, K, int(metric == 'cosine')])
    T = rng.standard_normal((N_ITEMS, d)).astype(np.float32)
    T[ZERO_ROW] = 0.0
    liked = []
    for u in range(N_USERS):
        n = LIKED_LADDER[u % len(LIKED_LADDER)]
        row = np.sort(rng.choice(N_ITEMS, size=n, replace=False)).astype(np.int64)
        if n == 200 and ZERO_ROW not in row:
            row = np.sort(np.concatenate([row[row != row[0]][:n - 1], [ZERO_ROW]]))
        liked.append(row)
    prop_rows = []
    for i in range(N_ITEMS):
        n = TARGET_ROWS[i % 4] if i < N_ITEMS // 2 else (300 if i >= N_ITEMS - 4 else int(rng.integers(0, 31)))
        prop_rows.append(np.sort(rng.choice(N_PROPS, size=n, replace=False)).astype(np.int64))
    df = np.bincount(np.concatenate(prop_rows), minlength=N_PROPS)
    users = np.concatenate([np.arange(N_USERS), rng.integers(0, N_USERS, size=M_LISTS - N_USERS)]).astype(np.int64)
    users = users[rng.permutation(M_LISTS)]
    lists = np.full((M_LISTS, K), -1, dtype=np.int64)
    for j in range(M_LISTS):
        row = rng.choice(N_ITEMS, size=K, replace=False)
        own = liked[users[j]]
        for t in range(min(K, 3, len(own))):                         # targets inside the user's liked list
            cand = own[(5 * t + j) % len(own)]
            if cand not in row:
                row[(2 * t) % K] = cand
        if j == 0:
            row[K - 1] = ZERO_ROW if ZERO_ROW not in row else row[K - 1]
        lists[j] = row
        if K > 1 and j % 3 == 0:
            lists[j, K - 1 - (j % min(K - 1, 5)):] = -1              # padding at the end
        if K > 2 and j % 4 == 1:
            lists[j, K // 2] = -1                                    # and inside
    return {'T': T, 'liked': liked, 'prop_rows': prop_rows, 'weight': idf(df, N_ITEMS), 'users': users, 'lists': lists,
            'max_prop_row': max(len(r) for r in prop_rows)}


def case_reference(case, metric, E, Q):
    grid, tol = sim_grid(case['T'], metric), sim_tolerance(case['T'], metric)
    return [explain_list(case['lists'][j], case['liked'][case['users'][j]], grid, tol, case['prop_rows'], case['weight'], E, Q)
            for j in range(len(case['lists']))]


def exact_case(seed=5):
    """Small-integer vectors under dot and dyadic weights: every similarity and score is exact in float32, with many ties."""
    rng = np.random.default_rng(seed)
    n_items, n_users, n_props, d, K = 60, 9, 24, 8, 12
    T = rng.integers(-2, 3, size=(n_items, d)).astype(np.float32)
    T[3] = 0.0
    T[11] = T[10]
    liked = [np.sort(rng.choice(n_items, size=int(n), replace=False)).astype(np.int64) for n in rng.integers(0, 40, size=n_users)]
    prop_rows = [np.sort(rng.choice(n_props, size=int(rng.integers(0, 9)), replace=False)).astype(np.int64) for _ in range(n_items)]
    weight = (2.0 ** rng.integers(-2, 2, size=n_props)).astype(np.float32)
    users = rng.integers(0, n_users, size=20).astype(np.int64)
    lists = np.stack([rng.choice(n_items, size=K, replace=False) for _ in users]).astype(np.int64)
    lists[::4, K - 2:] = -1
    return {'T': T, 'liked': liked, 'prop_rows': prop_rows, 'weight': weight, 'users': users, 'lists': lists,
            'max_prop_row': max(len(r) for r in prop_rows)}
