"""Numpy restatement of recommendation among candidates (amar_recommend_among_f32, recommend.py:recommend_among): from a score
matrix, exclusion sets and a candidate set — one for every user, or one per listed user — the lists in the order of rank_better
(score descending, item row ascending), -1 / -inf padded.  And `items_with_properties`, restated by plain loops over sets.
Plain numpy and Python sets; no library code."""
import numpy as np


def topk_among(S, users, excl, cand, k, per_user=False):
    """(items int64 [m, k], scores float32 [m, k]) for the listed `users` (rows of S): the k best item rows of the user's candidate
    set that are not in excl[user].  `cand`: an iterable of item rows (every user) or, with per_user=True, one such iterable per
    LISTED user.  `excl`: per user a set of item rows (None: nothing is excluded)."""
    users = list(users)
    items = np.full((len(users), k), -1, dtype=np.int64)
    scores = np.full((len(users), k), -np.inf, dtype=np.float32)
    for j, u in enumerate(users):
        mine = set(int(c) for c in (cand[j] if per_user else cand))
        if excl is not None:
            mine -= set(excl[u])
        rows = sorted(mine, key=lambda r: (-float(S[u, r]), r))[:k]
        items[j, :len(rows)] = rows
        scores[j, :len(rows)] = [S[u, r] for r in rows]
    return items, scores


def filter_lists(items, scores, keep, k):
    """A complete ranking per row (items [m, K] best first, -1 padded) struck down to the entries in keep[j] (a set per row, or one
    set for all rows) and cut to k: what recommend_among must return when `items` is every user's full ranking."""
    m = len(items)
    out_i = np.full((m, k), -1, dtype=np.int64)
    out_s = np.full((m, k), -np.inf, dtype=np.float32)
    for j in range(m):
        mine = keep[j] if isinstance(keep, list) else keep
        at = [p for p in range(items.shape[1]) if items[j, p] >= 0 and int(items[j, p]) in mine][:k]
        out_i[j, :len(at)] = items[j, at]
        out_s[j, :len(at)] = scores[j, at]
    return out_i, out_s


def item_properties(n_items, links):
    """links: (item row, property index) pairs -> a list of n_items sets."""
    has = [set() for _ in range(n_items)]
    for i, p in links:
        has[int(i)].add(int(p))
    return has


def items_with_properties(has, any_of=None, all_of=None, none_of=None):
    """Item rows (ascending) whose property set has at least one of any_of, every one of all_of and none of none_of; None = no
    constraint."""
    out = []
    for i, mine in enumerate(has):
        ok = True
        if any_of is not None:
            ok = ok and any(p in mine for p in any_of)
        if all_of is not None:
            ok = ok and all(p in mine for p in all_of)
        if none_of is not None:
            ok = ok and not any(p in mine for p in none_of)
        if ok:
            out.append(i)
    return out
