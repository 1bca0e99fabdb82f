"""Reference of cursor paging (amar_recommend_after_f32, amar_topk_segmented_after_f32): plain numpy, no library code.

The rankers' order is score descending, then item ascending: a strict total order over distinct items, so a position in a ranking
is a pair (score, item) whether or not that pair is in the ranking.  `next_page` returns the k best entries strictly after one."""
import numpy as np

START = (np.float32(np.inf), -1)              # before every pair
END = (np.float32(-np.inf), -1)               # the padding of an exhausted list: after every pair


def after(score, item, cursor):
    """Whether (score, item) comes strictly after `cursor` = (score, item); arrays broadcast.  A NaN cursor score: nothing does."""
    cs, ci = np.float32(cursor[0]), int(cursor[1])
    score = np.asarray(score, dtype=np.float32)
    return (score < cs) | ((score == cs) & (np.asarray(item) > ci))


def next_page(scores, k, cursor=START, items=None, excluded=()):
    """scores float32 [n] of the items `items` (0..n-1 when None; distinct), `excluded` item values that must not be returned.
    Returns (items int64 [k], -1 padded; scores float32 [k], -inf padded): the k best, by (score descending, item ascending), of
    the unexcluded entries strictly after `cursor`."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    items = np.arange(len(scores), dtype=np.int64) if items is None else np.asarray(items, dtype=np.int64).reshape(-1)
    keep = after(scores, items, cursor)
    if len(excluded):
        keep &= ~np.isin(items, np.fromiter(excluded, dtype=np.int64))
    it, sc = items[keep], scores[keep]
    order = np.lexsort((it, -sc.astype(np.float64)))[:k]
    out_i, out_s = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf, dtype=np.float32)
    out_i[:len(order)], out_s[:len(order)] = it[order], sc[order]
    return out_i, out_s


def pages(score_rows, k, cursors, excluded=None):
    """`next_page` per row: score_rows [m, n], cursors = (items [m], scores [m]) as the entry points take them, excluded = one set per
    row or None.  Returns (items int64 [m, k], scores float32 [m, k])."""
    out = [next_page(row, k, (cursors[1][j], cursors[0][j]), excluded=() if excluded is None else excluded[j])
           for j, row in enumerate(score_rows)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
