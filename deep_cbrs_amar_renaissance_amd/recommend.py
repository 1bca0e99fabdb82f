"""Full-catalogue top-k recommendation: "the k best items for these users, among everything they have not seen".

Every scoring model exposes ``recommend(trainset, k=10, users=None, exclude_seen=True)``; this module holds the shared part.

Two routes, chosen by the head alone (no user-facing switch):

* fused: heads with a split plan (models/basic.py:_split_plan — every Basic* GNN model, BasicRS with a classifier of at
  least one hidden layer).  The towers are computed once per call in split form (b1 folded into the item table) and ONE
  ``amar_recommend_f32`` launch (two with item slices) scores every (user, item) pair and keeps each user's top-k on chip;
  nothing of size |U| x |I| reaches memory.
* pairs (`_recommend_pairs`): every other head (the hybrids, BasicRS without classifier hidden layers).  Per user chunk the
  unexcluded pair list is built on the device, scored by the model's hoisted pair scoring (``score_towers``) and ranked by
  ``amar_topk_segmented_f32``.  The tests also use it as the in-library yardstick of the fused route.

Both return ``(users int64 [m], items int64 [m, k], scores float32 [m, k])``: items are node ids (table row + |U|, the
convention of ``predict()`` inputs and ``top_k_arrays``), rows ordered by score descending then item id ascending, users with
fewer than k unexcluded items padded with -1 / -inf.

Inside ``device_lists()`` both routes stop before that conversion and return ``(users int64 [m] on the host, items int32 [m, k] item
ROWS on the device, scores float32 [m, k] on the device)``: ``evaluate_ranking`` scores the lists where they are
(``amar_rank_metrics_f64``), which is what lets ``fit(validation_ranking=...)`` validate every epoch.
"""
import contextlib
import weakref

import numpy as np
import torch

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd.engine import default_device

K_MAX = 64
PAIRS_PER_CHUNK = 1 << 24            # pair route: pairs scored per chunk of users (16 Mi: 64 MB of scores + 128 MB of ids)


def check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K_MAX:
        raise ValueError("k must be an integer in [1, {}] (got {!r})".format(K_MAX, k))
    return int(k)


def check_users(users, n_users):
    """Host int64 user indices in 0..n_users-1 (all users when None), in the caller's order."""
    if users is None:
        return np.arange(n_users, dtype=np.int64)
    u = users.detach().cpu().numpy() if isinstance(users, torch.Tensor) else np.asarray(users)
    u = u.reshape(-1)
    if u.size and not np.issubdtype(u.dtype, np.integer):
        raise ValueError("users must be integer indices")
    u = u.astype(np.int64)
    if u.size and (u.min() < 0 or u.max() >= n_users):
        raise ValueError("user indices must lie in [0, {}) (got {}..{})".format(n_users, int(u.min()), int(u.max())))
    return u


def exclusion_csr(ratings, n_users, n_items):
    """Training pairs as a CSR over users: (ptr int64 [n_users+1], items int64) with item ROWS 0..n_items-1, sorted and de-duplicated
    per user.  Every pair of `ratings` is excluded, whatever its label."""
    r = np.asarray(ratings)
    if r.size == 0:
        return np.zeros(n_users + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    u = r[:, 0].astype(np.int64)
    i = r[:, 1].astype(np.int64) - n_users
    if u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items:
        raise ValueError("ratings hold pairs outside the trainset's users / items")
    key = np.unique(u * n_items + i)                     # sorted by (user, item), duplicates gone
    uu, ii = key // n_items, key % n_items
    ptr = np.zeros(n_users + 1, dtype=np.int64)
    np.cumsum(np.bincount(uu, minlength=n_users), out=ptr[1:])
    return ptr, ii


# Exclusion CSRs on the device, built once per ratings array (held weakly: a dropped trainset frees its entry).
_EXCL_CACHE = {}


def _exclusion_device(trainset, n_users, n_items, exclude_seen):
    if not exclude_seen:
        return None
    ratings = trainset.ratings
    dev = default_device()
    key = (id(ratings), n_users, n_items, str(dev))
    hit = _EXCL_CACHE.get(key)
    if hit is not None and hit[0]() is ratings and hit[1] == np.shape(ratings):
        return hit[2]
    ptr, items = exclusion_csr(ratings, n_users, n_items)
    entry = (torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev))
    try:
        ref = weakref.ref(ratings)
        weakref.finalize(ratings, _EXCL_CACHE.pop, key, None)
    except TypeError:                                    # not weakly referenceable: keep the array alive with its entry
        ref = (lambda obj: (lambda: obj))(ratings)
    _EXCL_CACHE[key] = (ref, np.shape(ratings), entry)
    return entry


def _sizes(trainset):
    return len(trainset.users), len(trainset.items)


def _empty(k):
    return np.zeros(0, dtype=np.int64), np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)


_ON_DEVICE = False


@contextlib.contextmanager
def device_lists():
    """Internal: while active, `fused` and `pairs` return their device tensors (item rows, scores) instead of host node ids."""
    global _ON_DEVICE
    saved, _ON_DEVICE = _ON_DEVICE, True
    try:
        yield
    finally:
        _ON_DEVICE = saved


def evaluate_ranking(model, trainset, test_ratings, ks, users=None, exclude_seen=True):
    """model.recommend at k = max(ks) with the lists kept on the device, then utilities.metrics.full_ranking_metrics_device: the
    dict of `full_ranking_metrics(*model.recommend(...)[:2], test_ratings, ks)` without the lists (or a Python loop) on the host."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics, full_ranking_metrics_device
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("evaluate_ranking needs at least one k")
    n_users, n_items = _sizes(trainset)
    with device_lists():
        u, items, _ = model.recommend(trainset, k=check_k(max(ks)), users=users, exclude_seen=exclude_seen)
    if len(u) == 0:
        return full_ranking_metrics(u, items, test_ratings, ks)
    return full_ranking_metrics_device(None if users is None else u, items.contiguous(), test_ratings, ks, n_users, n_items)


def _finish(users, items, scores, n_users):
    if _ON_DEVICE:
        return users, items, scores
    items = items.cpu().numpy().astype(np.int64)
    items = np.where(items >= 0, items + n_users, -1)
    return users, items, scores.cpu().numpy().astype(np.float32)


def fused(towers, plan, trainset, k, users, exclude_seen):
    """One amar_recommend_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in)."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    tu, ti = towers[0], towers[1]
    excl = _exclusion_device(trainset, n_users, n_items, exclude_seen)
    blob, dims, acts = plan['rest']
    u_dev = None if users is None else torch.from_numpy(u.astype(np.int32)).to(tu.device)
    items, scores = capi.recommend(tu, ti, blob, dims, acts, plan['in_act'], k, users=u_dev,
                                   excl_ptr=excl[0] if excl else None, excl_items=excl[1] if excl else None)
    return _finish(u, items, scores, n_users)


def pairs(score_fn, trainset, k, users, exclude_seen, device=None):
    """Pair route: per user chunk, the unexcluded (user, item) list built on the device, scored by `score_fn(u_ids, i_ids)` (int32 rows
    of the user / item tower tables -> [P, 1] scores) and ranked by amar_topk_segmented_f32."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    dev = device or default_device()
    excl = _exclusion_device(trainset, n_users, n_items, exclude_seen)
    chunk = max(1, PAIRS_PER_CHUNK // max(1, n_items))
    out_i, out_s = [], []
    for lo in range(0, len(u), chunk):
        uc = torch.from_numpy(u[lo:lo + chunk]).to(dev)
        c = int(uc.numel())
        keep = torch.ones((c, n_items), dtype=torch.bool, device=dev)
        if excl is not None:
            ptr = excl[0].to(torch.int64)
            beg, cnt = ptr[uc], ptr[uc + 1] - ptr[uc]
            total = int(cnt.sum())
            if total:
                rows = torch.repeat_interleave(torch.arange(c, device=dev), cnt)
                first = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
                pos = torch.repeat_interleave(beg, cnt) + torch.arange(total, device=dev) - first
                keep[rows, excl[1].to(torch.int64)[pos]] = False
        r, i = keep.nonzero(as_tuple=True)                       # row-major: users in chunk order, items ascending
        seg = torch.zeros(c + 1, dtype=torch.int64, device=dev)
        torch.cumsum(keep.sum(1), 0, out=seg[1:])
        u_ids = uc[r].to(torch.int32).contiguous()
        i_ids = i.to(torch.int32).contiguous()
        if i_ids.numel():
            scores = score_fn(u_ids, i_ids).reshape(-1).contiguous()
        else:
            scores = torch.zeros(1, dtype=torch.float32, device=dev)
            i_ids = torch.zeros(1, dtype=torch.int32, device=dev)
        items, sc = capi.topk_segmented(seg.to(torch.int32), i_ids, scores, k)
        out_i.append(items)
        out_s.append(sc)
    return _finish(u, torch.cat(out_i), torch.cat(out_s), n_users)
