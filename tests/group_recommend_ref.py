"""numpy float32 reference of group recommendation (amar_recommend_group_f32, recommend_group): given the members' scores S
[n_users, n_items] (float32, the bits the single-user ranking returns), the aggregate of a group and its top-k list."""
import numpy as np


def aggregate(S, members, strategy):
    """The group's aggregate score of every item, float32 [n_items]: 'mean' adds the members' rows in ascending member order and
    divides by the group size (float32 throughout), 'min' / 'max' reduce elementwise."""
    members = sorted(int(u) for u in members)
    rows = np.asarray(S, dtype=np.float32)[members]
    if strategy == 'mean':
        acc = rows[0]
        for t in range(1, len(members)):
            acc = acc + rows[t]
        return (acc / np.float32(len(members))).astype(np.float32)
    if strategy == 'min':
        return np.minimum.reduce(rows, axis=0)
    if strategy == 'max':
        return np.maximum.reduce(rows, axis=0)
    raise ValueError(strategy)


def group_topk(S, members, excluded, k, strategy, min_score=None):
    """(items int64 [k] padded with -1, scores float32 [k] padded with -inf) of one group: aggregate descending, item ascending on
    ties, over the items that are neither in `excluded` nor vetoed (any member's score below min_score)."""
    S = np.asarray(S, dtype=np.float32)
    items, scores = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf, dtype=np.float32)
    if len(members) == 0:
        return items, scores
    agg = aggregate(S, members, strategy)
    ok = np.ones(S.shape[1], dtype=bool)
    if min_score is not None:
        ok &= S[sorted(int(u) for u in members)].min(0) >= np.float32(min_score)
    if len(excluded):
        ok[np.asarray(sorted(excluded), dtype=np.int64)] = False
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -agg[cand]))][:k]
    items[:len(order)], scores[:len(order)] = order, agg[order]
    return items, scores


def groups_topk(S, groups, excluded, k, strategy, min_score=None):
    """group_topk for every group: (items int64 [g, k], scores float32 [g, k]); excluded: one collection of items per group."""
    out = [group_topk(S, m, e, k, strategy, min_score) for m, e in zip(groups, excluded)]
    return (np.stack([o[0] for o in out]) if out else np.zeros((0, k), dtype=np.int64),
            np.stack([o[1] for o in out]) if out else np.zeros((0, k), dtype=np.float32))
