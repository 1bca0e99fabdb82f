"""Numpy reference of exact full-catalogue positions (amar_rank_of_f32) and of the cut-off-free metrics that follow from them
(amar_rank_of_metrics_f64), from a dense score matrix: direct counting for the kernel's four outputs, sort-then-count for the
metrics.  Plain numpy; no library code."""
import numpy as np


def candidates(n_items, excluded):
    keep = np.ones(n_items, dtype=bool)
    if excluded is not None and len(excluded):
        keep[np.asarray(sorted(excluded), dtype=np.int64)] = False
    return keep


def counts(row, excluded, targets):
    """(scores float32, greater, eq_before, eq_after int64) of the item rows `targets` for one user: `row` = its float32 score of
    every item, the candidates = the items outside `excluded`, the target itself never counted."""
    row = np.asarray(row, dtype=np.float32)
    keep = candidates(len(row), excluded)
    items = np.arange(len(row))
    out = np.zeros((3, len(targets)), dtype=np.int64)
    for e, t in enumerate(targets):
        others = keep & (items != t)
        out[0, e] = np.sum(others & (row > row[t]))
        out[1, e] = np.sum(others & (row == row[t]) & (items < t))
        out[2, e] = np.sum(others & (row == row[t]) & (items > t))
    return row[np.asarray(targets, dtype=np.int64)], out[0], out[1], out[2]


def rank_of(S, users, excluded_by_user, targets):
    """The flat outputs of a call: entry j = (users[j], targets[j]); `excluded_by_user[u]` = the excluded rows of user u (None:
    nobody excludes anything).  Returns (scores, greater, eq_before, eq_after), one value per target in entry order."""
    parts = [counts(S[u], None if excluded_by_user is None else excluded_by_user[u], sorted(t)) for u, t in zip(users, targets)]
    if not parts:
        return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return tuple(np.concatenate([p[c] for p in parts]) for c in range(4))


def positions(row, excluded):
    """{item row: 1-based position} of every candidate in the order of recommend(): score descending, item row ascending."""
    row = np.asarray(row, dtype=np.float32)
    keep = candidates(len(row), excluded)
    order = [i for i in np.lexsort((np.arange(len(row)), -row.astype(np.float64))) if keep[i]]
    return {int(i): p + 1 for p, i in enumerate(order)}


def metrics(row, excluded, relevant):
    """(auc, rr, ap, valid) of one user by the definitions: the candidates sorted as recommend() sorts them, the targets
    R' = relevant \\ excluded; rr = 1 / the first target's position; ap = the mean over the targets of precision at their position;
    auc = the share of (target, non-target candidate) pairs the target wins, a tie counting 1/2.  valid False (and zeros) when there
    is no target or no non-target candidate."""
    row = np.asarray(row, dtype=np.float32)
    pos = positions(row, excluded)
    rel = sorted(set(int(i) for i in relevant) & set(pos))
    neg = sorted(set(pos) - set(rel))
    if not rel or not neg:
        return 0.0, 0.0, 0.0, False
    ranks = sorted(pos[t] for t in rel)
    ap = 0.0
    for t in rel:                                             # in target (item row) order
        ap += sum(1 for r in ranks if r <= pos[t]) / float(pos[t])
    neg_scores = row[np.asarray(neg, dtype=np.int64)]
    wins = 0.0
    for t in rel:
        wins += float(np.sum(row[t] > neg_scores)) + 0.5 * float(np.sum(row[t] == neg_scores))
    return wins / (float(len(rel)) * float(len(neg))), 1.0 / float(ranks[0]), ap / float(len(rel)), True
