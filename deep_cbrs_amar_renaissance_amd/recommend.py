"""Full-catalogue top-k recommendation: "the k best items for these users, among everything they have not seen".

Every scoring model exposes ``recommend(trainset, k=10, users=None, exclude_seen=True)``; this module holds the shared part.

Two routes, chosen by the head alone (no user-facing switch):

* fused: heads with a split plan (models/basic.py:_split_plan — every Basic* GNN model, BasicRS with a classifier of at
  least one hidden layer).  The towers are computed once per call in split form (b1 folded into the item table) and ONE
  ``amar_recommend_f32`` launch (two with item slices) scores every (user, item) pair and keeps each user's top-k on chip;
  nothing of size |U| x |I| reaches memory.
  A head ranks fused only where the kernel has room for it: the rest stack, an item tile and the kernel's own state must fit
  160 KB of LDS (``capi.rank_route`` / ``capi.rank_fits``, asked per kernel: ``amar_recommend_f32``, ``amar_recommend_group_f32`` and
  ``amar_rank_of_f32`` have different sums, so 128 -> 128 -> 64 -> 1 is fused in ``recommend()`` and ranked by pairs in ``rank_items()``).
* pairs (`_recommend_pairs`): every other head (the hybrids, BasicRS without classifier hidden layers, a rest stack the kernel has no
  room for such as 128 -> 128 -> 128 -> 1: whatever ``predict()`` scores is ranked, nothing raises).  Per user chunk the
  unexcluded pair list is built on the device, scored by the model's hoisted pair scoring (``score_towers``) and ranked by
  ``amar_topk_segmented_f32``.  The tests also use it as the in-library yardstick of the fused route.

Both return ``(users int64 [m], items int64 [m, k], scores float32 [m, k])``: items are node ids (table row + |U|, the
convention of ``predict()`` inputs and ``top_k_arrays``), rows ordered by score descending then item id ascending, users with
fewer than k unexcluded items padded with -1 / -inf.

Inside ``device_lists()`` both routes stop before that conversion and return ``(users int64 [m] on the host, items int32 [m, k] item
ROWS on the device, scores float32 [m, k] on the device)``: ``evaluate_ranking`` scores the lists where they are
(``amar_rank_metrics_f64``), which is what lets ``fit(validation_ranking=...)`` validate every epoch.

The second half of the module is similarity search over the vectors the models learn: ``nearest`` (one ``amar_nearest_f32`` call, dot
or cosine, nothing of size m x n in memory) and ``SimilarSearch``, the mixin that gives every scoring model ``user_embeddings`` /
``item_embeddings``, ``similar_items``, ``similar_users`` and ``recommend_like``.

The third part is what a list looks like as a whole: ``rerank_mmr`` (one ``amar_rerank_mmr_f32`` launch re-ranks device pools by
Maximal Marginal Relevance; nothing of size m x P x P in memory), the mixin's ``recommend_diverse`` / ``list_diversity``, and the
opt-in ``diversity=`` of ``evaluate_ranking`` (intra-list diversity and catalogue coverage beside the accuracy metrics).

The fourth part answers "why this item for this user?": ``liked_csr`` and ``item_property_csr`` read the liked items and the
item-property links off the trainset, ``explain_lists`` joins them with the item vectors in one ``amar_explain_f32`` launch (nothing
of size m x K x L in memory) and the mixin's ``explain`` runs it on ``recommend(k)``'s device lists or on the caller's items.

The fifth part answers "what should WE watch?": ``group_csr`` / ``group_exclusion_csr`` turn groups of users into the CSRs of
``amar_recommend_group_f32``, ``group_fused`` is that one launch over the split towers (every member's score of every item combined
by the mean, the minimum or the maximum, with an optional veto, and selected on chip: nothing of size members x |I| in memory),
``group_pairs`` the same arithmetic over pair-route scores for the heads without a fused kernel, and the mixin's
``recommend_group`` picks between them exactly as ``recommend()`` does.

The sixth part keeps a list in proportion to its user's tastes: ``item_category_csr`` turns the item-property links (or a membership
matrix) into the categories of ``amar_rerank_calibrated_f32``, ``rerank_calibrated`` is that one launch over device pools (the user's
and the list's category distributions stay in LDS: nothing of size m x P x G in memory), the mixin's ``recommend_calibrated`` /
``list_calibration`` run it and its float64 metric (``amar_list_calibration_f64``), and ``evaluate_ranking`` takes ``calibration=``.

The seventh part turns the question round: "where does THIS item stand for this user?".  ``rank_of_fused`` is one
``amar_rank_of_f32`` launch over the split towers (every pair of the catalogue scored by the rankers' own score routine and counted
against the targets' scores on chip: nothing of size |U| x |I| in memory), ``rank_of_pairs`` the same counts from pair-route scores
per user chunk for the heads without a fused kernel, the mixin's ``rank_items`` answers per (user, item) pair, and
``evaluate_ranking`` takes ``rank_metrics=`` (AUC, MRR, MAP from the exact ranks of every held-out item: ``amar_rank_of_metrics_f64``).

The eighth part narrows the catalogue: "the best k among THESE items".  ``check_candidates`` reads a candidate set (node ids, a mask,
or one set per listed user), ``items_with_properties`` builds one from the graph's item-property links, ``among_fused`` is one
``amar_recommend_among_f32`` launch over the split towers (|U| x |C| pairs scored, the candidates' rows gathered into the item tile),
``pairs(keep_items=...)`` the pair route over the kept pairs, and the mixin's ``recommend_among`` picks between them.

The ninth part pages: "the best k AFTER this position of the user's ranking".  The order is a strict total order, so a position is a
pair (score, item); ``check_after`` reads the cursors, ``after_fused`` is one ``amar_recommend_after_f32`` launch (``fused`` with one
more compare per pair), ``pairs(after=...)`` the pair route from a cursor (``amar_topk_segmented_after_f32``), ``deep_fused`` /
``deep_pairs`` chain ceil(k / K_MAX) pages into lists of up to ``DEEP_K_MAX`` = 1024, and the mixin's ``recommend_after`` /
``recommend_deep`` pick between them as ``recommend()`` does.

The tenth part gives every user its own candidates: "the best k of THIS user's list".  ``check_candidate_lists`` reads one list per
listed user (sequences, or an [m, P] array / device tensor of node ids padded with -1), ``device_candidate_csr`` sorts and compacts a
device tensor where it is, ``lists_fused`` is one ``amar_recommend_lists_f32`` launch over the split towers (sum |C_u| pairs scored,
every wave walking its own user's list: nothing of size |U| x |I| anywhere), the mixin's ``recommend_from`` picks between it and
``pairs(keep_items=CSR)``, and ``evaluate_ranking_sampled`` is its in-library consumer: the 1 + N sampled-negatives protocol.
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


def check_ids(ids, lo, hi, what, not_integer="{what} must be integer node ids", out_of_range="{what} must lie in [{lo}, {hi}) (got {min}..{max})"):
    """Host int64 node ids in [lo, hi) (all of them when None), in the caller's order."""
    if ids is None:
        return np.arange(lo, hi, dtype=np.int64)
    a = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    a = a.reshape(-1)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(not_integer.format(what=what))
    a = a.astype(np.int64)
    if a.size and (a.min() < lo or a.max() >= hi):
        raise ValueError(out_of_range.format(what=what, lo=lo, hi=hi, min=int(a.min()), max=int(a.max())))
    return a


def check_users(users, n_users):
    """Host int64 user indices in 0..n_users-1 (all users when None), in the caller's order."""
    return check_ids(users, 0, n_users, 'users', "{what} must be integer indices", "user indices must lie in [{lo}, {hi}) (got {min}..{max})")


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


def liked_csr(ratings, n_users, n_items):
    """Label-1 training pairs as a CSR over users: (ptr int64 [n_users+1], items int64) with item ROWS 0..n_items-1, sorted and
    de-duplicated per user; the checks of `exclusion_csr`."""
    r = np.asarray(ratings)
    if r.size:
        r = r[r[:, 2] == 1]
    return exclusion_csr(r, n_users, n_items)


def item_property_csr(trainset):
    """The item-property links a trainset's graph already holds, as a CSR over items: (ptr int64 [|I|+1], props int64 property
    indices 0..|P|-1 sorted and de-duplicated per item, df int64 [|P|]: the distinct items of every property, max_row: the longest
    row), or None when the graph has no properties.  One adjacency larger than |U| + |I| ('unary-uip'): item rows |U|..|U|+|I|-1,
    columns >= |U|+|I|; a pair of adjacencies ('unary-kg'): the item-property one, items at rows 0..|I|-1.  Duplicate (item,
    property) links collapse to one."""
    n_users, n_items = _sizes(trainset)
    adj = getattr(trainset, 'adj_matrix', None)
    if isinstance(adj, (tuple, list)):
        if len(adj) < 2 or not hasattr(adj[1], 'tocoo'):                # (user-item, item-property[, user-property])
            return None
        coo, row0, col0 = adj[1].tocoo(), 0, n_items
    elif hasattr(adj, 'tocoo') and adj.shape[0] > n_users + n_items:
        coo, row0, col0 = adj.tocoo(), n_users, n_users + n_items
    else:
        return None
    n_props = int(coo.shape[0]) - col0
    if n_props <= 0:
        return None
    row, col = coo.row.astype(np.int64), coo.col.astype(np.int64)
    keep = (row >= row0) & (row < row0 + n_items) & (col >= col0)
    key = np.unique((row[keep] - row0) * n_props + (col[keep] - col0))
    it, pr = key // n_props, key % n_props
    ptr = np.zeros(n_items + 1, dtype=np.int64)
    np.cumsum(np.bincount(it, minlength=n_items), out=ptr[1:])
    return ptr, pr, np.bincount(pr, minlength=n_props).astype(np.int64), int(np.diff(ptr).max()) if n_items else 0


def property_weights(df, n_items, kind='idf'):
    """Float32 weights of the properties: 'idf' = log(|I| / df_p) computed in float64 (0 for a property nobody has), 'none' = 1."""
    if kind == 'none':
        return np.ones(len(df), dtype=np.float32)
    if kind != 'idf':
        raise ValueError("property_weight must be 'idf' or 'none' (got {!r})".format(kind))
    df = np.asarray(df, dtype=np.float64)
    return np.where(df > 0, np.log(float(n_items) / np.maximum(df, 1.0)), 0.0).astype(np.float32)


def _is_matrix(x):
    return hasattr(x, 'tocoo') or (isinstance(x, np.ndarray) and x.ndim == 2)


def item_category_csr(trainset, categories=None):
    """The categories calibration works in, as a CSR over item rows: (ptr int64 [|I|+1], ids int64 category numbers 0..G-1 sorted and
    de-duplicated per item, category_props int64 [G]: the property index of every category, max_row: the longest row).
    categories=None: the min(|P|, MAX_G) properties of `item_property_csr` with the largest document frequency (only df > 0 counts;
    ties to the smaller property index), numbered in ascending property index.  An int N: the N most frequent ones.  A sequence of
    property indices (unique, in range, at most MAX_G of them): those, numbered in ascending property index.  A scipy-sparse or dense
    0/1 membership matrix [|I|, G] (G <= MAX_G; category_props is then 0..G-1) serves trainsets without a property graph.
    ValueError for anything else, and for a trainset that has no properties when no matrix is given."""
    n_users, n_items = _sizes(trainset)
    max_g = capi.CALIBRATE_MAX_G
    if categories is not None and _is_matrix(categories):
        if tuple(categories.shape) != (n_items, categories.shape[1]) or not 1 <= categories.shape[1] <= max_g:
            raise ValueError("a category matrix must be [{} items, 1..{} categories] (got {})".format(n_items, max_g, tuple(categories.shape)))
        if hasattr(categories, 'tocoo'):
            coo = categories.tocoo()
            keep = np.asarray(coo.data) != 0
            it, g = coo.row[keep].astype(np.int64), coo.col[keep].astype(np.int64)
        else:
            it, g = (a.astype(np.int64) for a in np.nonzero(np.asarray(categories)))
        G = int(categories.shape[1])
        key = np.unique(it * G + g)
        props = np.arange(G, dtype=np.int64)
    else:
        csr = item_property_csr(trainset)
        if csr is None:
            raise ValueError("the trainset has no item properties: pass `categories` as an [items, categories] membership matrix")
        ptr, pr, df, _ = csr
        n_props = len(df)
        if categories is None or (isinstance(categories, (int, np.integer)) and not isinstance(categories, bool)):
            want = max_g if categories is None else int(categories)
            if not 1 <= want <= max_g:
                raise ValueError("categories must be an integer in [1, {}] (got {!r})".format(max_g, categories))
            order = np.lexsort((np.arange(n_props), -df))                # df descending, property index ascending
            props = np.sort(order[:want][df[order[:want]] > 0]).astype(np.int64)
        else:
            try:
                props = list(categories)
            except TypeError:
                props = None
            if props is None or np.ndim(props) != 1:                      # a nested list is no matrix: an ndarray or a scipy matrix is
                raise ValueError("categories must be None, an integer, a sequence of property indices or a membership matrix")
            try:
                props = check_ids(props, 0, n_props, 'categories')
            except TypeError:
                raise ValueError("categories must be None, an integer, a sequence of property indices or a membership matrix")
            if len(props) > max_g or len(np.unique(props)) != len(props):
                raise ValueError("categories must be at most {} distinct property indices".format(max_g))
            props = np.sort(props)
        if len(props) == 0:
            raise ValueError("no property is linked to any item: there is no category to calibrate on")
        G = len(props)
        number = np.full(n_props, -1, dtype=np.int64)
        number[props] = np.arange(G)
        it = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(ptr))
        g = number[pr]
        key = (it * G + g)[g >= 0]                                        # already sorted by (item, category): props ascending
    ptr = np.zeros(n_items + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // G, minlength=n_items), out=ptr[1:])
    return ptr, key % G, props, int(np.diff(ptr).max()) if n_items else 0


# Exclusion, liked and property CSRs on the device, built once per ratings array / graph (held weakly where the object allows it: a
# dropped trainset frees its entries).  The key is the object's identity: an array or graph mutated in place is not noticed, and the
# finalizer of a dead object whose id was reused may drop the new object's entry, which only costs a rebuild.
_EXCL_CACHE, _LIKED_CACHE, _PROP_CACHE, _CAT_CACHE = {}, {}, {}, {}


def _device_cached(cache, obj, key, build):
    hit = cache.get(key)
    if hit is not None and hit[0]() is obj:
        return hit[1]
    entry = build()
    try:
        ref = weakref.ref(obj)
        weakref.finalize(obj, cache.pop, key, None)
    except TypeError:                                    # not weakly referenceable: keep the object alive with its entry
        ref = (lambda o: (lambda: o))(obj)
    cache[key] = (ref, entry)
    return entry


def _exclusion_device(trainset, n_users, n_items, exclude_seen):
    if not exclude_seen:
        return None
    ratings, dev = trainset.ratings, default_device()

    def build():
        ptr, items = exclusion_csr(ratings, n_users, n_items)
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev)
    return _device_cached(_EXCL_CACHE, ratings, (id(ratings), np.shape(ratings), n_users, n_items, str(dev)), build)


def _liked_device(trainset, n_users, n_items):
    ratings, dev = trainset.ratings, default_device()

    def build():
        ptr, items = liked_csr(ratings, n_users, n_items)
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev)
    return _device_cached(_LIKED_CACHE, ratings, (id(ratings), np.shape(ratings), n_users, n_items, str(dev)), build)


def _props_device(trainset, n_items, kind):
    """(prop_ptr, prop_ids, weights) on the device and the longest row, or None for a trainset without properties."""
    adj, dev = getattr(trainset, 'adj_matrix', None), default_device()
    if adj is None:
        return None

    def build():
        csr = item_property_csr(trainset)
        if csr is None:
            return None
        ptr, ids, df, max_row = csr
        w = torch.from_numpy(property_weights(df, n_items, kind)).to(dev)
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(ids.astype(np.int32)).to(dev), w, max_row
    return _device_cached(_PROP_CACHE, adj, (id(adj), n_items, kind, str(dev)), build)


def _cats_device(trainset, n_items, categories):
    """(cat_ptr, cat_ids) on the device, the number of categories and the longest row, cached per graph (or per membership matrix)
    and category choice; the ValueErrors of `item_category_csr`."""
    dev = default_device()
    if categories is not None and _is_matrix(categories):
        obj, choice = categories, 'matrix'
    else:
        obj = getattr(trainset, 'adj_matrix', None)
        choice = categories
        if not (categories is None or (isinstance(categories, (int, np.integer)) and not isinstance(categories, bool))):
            try:
                choice = repr(list(categories))                           # [1.0] is not [1]: a hit must not skip the checks
            except TypeError:
                choice, obj = None, None                                  # not a sequence: item_category_csr says so
    if obj is None:
        item_category_csr(trainset, categories)                           # raises: nothing to hold an entry for
        raise ValueError("the trainset has no graph to take categories from")

    def build():
        ptr, ids, props, max_row = item_category_csr(trainset, categories)
        return torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(ids.astype(np.int32)).to(dev), len(props), max_row
    return _device_cached(_CAT_CACHE, obj, (id(obj), n_items, choice, str(dev)), build)


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


def evaluate_ranking(model, trainset, test_ratings, ks, users=None, exclude_seen=True, diversity=None, calibration=None, rank_metrics=None):
    """model.recommend at k = max(ks) with the lists kept on the device, then utilities.metrics.full_ranking_metrics_device: the
    dict of `full_ranking_metrics(*model.recommend(...)[:2], test_ratings, ks)` without the lists (or a Python loop) on the host.
    diversity={'metric': 'cosine' | 'dot', 'space': ...} (both optional) adds, for every k, 'ild_at_<k>' (the float64 mean, over the
    lists with at least two items in their first k ranks, of the intra-list diversity of those ranks in the model's item `space`:
    amar_list_diversity_f64) and 'item_coverage_at_<k>' (the distinct items in the first k ranks of all lists over |I|).
    calibration={'smoothing': 0.01, 'categories': None} (both optional) adds 'miscalibration_at_<k>': the float64 mean, over the users
    that have a target, of C(p, the first k ranks) (amar_list_calibration_f64; categories as in `item_category_csr`), 0 when no user
    has one.
    rank_metrics=('auc', 'mrr', 'map') (any subset) adds those keys — the cut-off-free measures from the exact rank of every
    held-out item (`heldout_rank_metrics`; utilities.metrics.full_ranking_rank_metrics has the definitions) — and
    'rank_metrics_users' = (evaluated, skipped); `ks` may then be empty."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import check_rank_metrics, full_ranking_metrics, full_ranking_metrics_device
    ks = [int(k) for k in ks]
    if rank_metrics is not None:
        rank_metrics = check_rank_metrics(rank_metrics)
        if not ks:
            if diversity is not None or calibration is not None:
                raise ValueError("diversity and calibration are measured at cutoffs: evaluate_ranking needs at least one k for them")
            return heldout_rank_metrics(model, trainset, test_ratings, users, exclude_seen, rank_metrics)
        out = evaluate_ranking(model, trainset, test_ratings, ks, users=users, exclude_seen=exclude_seen, diversity=diversity,
                               calibration=calibration)
        out.update(heldout_rank_metrics(model, trainset, test_ratings, users, exclude_seen, rank_metrics))
        return out
    if not ks:
        raise ValueError("evaluate_ranking needs at least one k")
    if diversity is not None:
        unknown = set(diversity) - {'metric', 'space'}
        if unknown:
            raise ValueError("diversity takes the keys 'metric' and 'space' (got {})".format(sorted(unknown)))
        check_metric(diversity.get('metric', 'cosine'))
    if calibration is not None:
        unknown = set(calibration) - {'smoothing', 'categories'}
        if unknown:
            raise ValueError("calibration takes the keys 'smoothing' and 'categories' (got {})".format(sorted(unknown)))
        check_smoothing(calibration.get('smoothing', 0.01))
    n_users, n_items = _sizes(trainset)
    cats = _cats_device(trainset, n_items, calibration.get('categories')) if calibration is not None else None
    with device_lists():
        u, items, _ = model.recommend(trainset, k=check_k(max(ks)), users=users, exclude_seen=exclude_seen)
    if len(u) == 0:
        out = full_ranking_metrics(u, items, test_ratings, ks)
        if diversity is not None:
            for k in ks:
                out['ild_at_{}'.format(k)], out['item_coverage_at_{}'.format(k)] = 0.0, 0.0
        if calibration is not None:
            for k in ks:
                out['miscalibration_at_{}'.format(k)] = 0.0
        return out
    items = items.contiguous()
    out = full_ranking_metrics_device(None if users is None else u, items, test_ratings, ks, n_users, n_items)
    if diversity is not None:
        table = model._item_embeddings(trainset, diversity.get('space'))
        out.update(diversity_metrics(items, table, ks, diversity.get('metric', 'cosine'), n_items))
    if calibration is not None:
        u_dev = None if users is None else torch.from_numpy(u.astype(np.int32)).to(items.device)
        out.update(calibration_metrics(items, u_dev, _liked_device(trainset, n_users, n_items), cats, ks, calibration.get('smoothing', 0.01)))
    return out


def calibration_metrics(lists, users, liked, cats, ks, smoothing=0.01):
    """{'miscalibration_at_<k>'} of device lists (int32 [m, K] item rows, -1 padded) of `users` (int32 [m] on the device, None = the
    identity): C per list from amar_list_calibration_f64 (`liked` = the liked CSR on the device, `cats` = `_cats_device`), averaged
    in float64 over the users that have a target (0 when none has)."""
    kl, _, support = capi.list_calibration(lists, liked[0], liked[1], cats[0], cats[1], cats[2], ks, smoothing=check_smoothing(smoothing), users=users)
    kl, has = kl.cpu().numpy(), support.cpu().numpy() > 0
    return {'miscalibration_at_{}'.format(k): float(kl[has, q].mean()) if has.any() else 0.0 for q, k in enumerate(ks)}


def diversity_metrics(lists, table, ks, metric, n_items):
    """{'ild_at_<k>', 'item_coverage_at_<k>'} of device lists (int32 [m, K] item rows, -1 padded): the ILD per list from
    amar_list_diversity_f64, averaged in float64 over the lists that have at least two items in their first k ranks (0 when none
    has); the coverage by integer work on the device."""
    check_width(table.shape[1], 'item vectors')
    table = _as_device_matrix(table, lists.device, 'table')
    ild, count = capi.list_diversity(lists, table, ks, metric=check_metric(metric))
    ild, count = ild.cpu().numpy(), count.cpu().numpy()
    out = {}
    for q, k in enumerate(ks):
        has = count[:, q] >= 2
        out['ild_at_{}'.format(k)] = float(ild[has, q].mean()) if has.any() else 0.0
        head = lists[:, :k]
        seen = torch.zeros(n_items + 1, dtype=torch.bool, device=lists.device)
        seen[torch.where(head >= 0, head, n_items).reshape(-1).to(torch.int64)] = True
        out['item_coverage_at_{}'.format(k)] = int(seen[:n_items].sum()) / float(n_items) if n_items else 0.0
    return out


def _finish(users, items, scores, n_users):
    if _ON_DEVICE:
        return users, items, scores
    items = items.cpu().numpy().astype(np.int64)
    items = np.where(items >= 0, items + n_users, -1)
    return users, items, scores.cpu().numpy().astype(np.float32)


def _ranker_args(towers, plan, trainset=None, exclude_seen=False, listed=None):
    """What the fused routes hand capi's rankers, as (head, keywords): head = (tu, ti, wpack, dims, acts, in_act), their six leading
    arguments, from the split towers and their plan; with a `trainset`, excl_ptr / excl_items = its exclusion CSR on the device
    (None without exclude_seen); with `listed` (host user indices), users = those rows as int32 on the towers' device."""
    blob, dims, acts = plan['rest']
    kw = {}
    if trainset is not None:
        excl = _exclusion_device(trainset, *_sizes(trainset), exclude_seen)
        kw.update(excl_ptr=excl[0] if excl else None, excl_items=excl[1] if excl else None)
    if listed is not None:
        kw['users'] = torch.from_numpy(listed.astype(np.int32)).to(towers[0].device)
    return (towers[0], towers[1], blob, dims, acts, plan['in_act']), kw


def fused(towers, plan, trainset, k, users, exclude_seen):
    """One amar_recommend_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in)."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen, None if users is None else u)
    items, scores = capi.recommend(*head, k, **kw)
    return _finish(u, items, scores, n_users)


def _unseen_mask(uc, n_items, excl, dev):
    """bool [c, n_items] on the device: True where the item row is not in the exclusion row of user uc[row] (`excl` = the device
    CSR of `_exclusion_device`, None: everything is kept)."""
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
    return keep


def _kept_mask(ptr, rows, lo, c, n_items, dev):
    """bool [c, n_items] on the device: True where the item row is in segment lo + row of the host CSR (ptr, rows) over the listed
    users — `_unseen_mask`'s construction, with True for the listed rows."""
    keep = torch.zeros((c, n_items), dtype=torch.bool, device=dev)
    b, e = int(ptr[lo]), int(ptr[lo + c])
    if e > b:
        cnt = torch.from_numpy(np.diff(ptr[lo:lo + c + 1])).to(dev)
        at = torch.repeat_interleave(torch.arange(c, device=dev), cnt)
        keep[at, torch.from_numpy(np.ascontiguousarray(rows[b:e], dtype=np.int64)).to(dev)] = True
    return keep


def _scored_chunks(score_fn, trainset, u, exclude_seen, dev, keep_items=None):
    """The pair route's scoring, per chunk of the listed users `u` (host int64): the unexcluded (user, item) list built on the device
    and scored once by `score_fn`.  Yields (lo, c, seg_ptr int32 [c + 1], item rows int32, scores float32): the arguments of
    amar_topk_segmented_f32 / amar_topk_segmented_after_f32 for the listed rows lo .. lo + c - 1.  keep_items as in `pairs`."""
    n_users, n_items = _sizes(trainset)
    excl = _exclusion_device(trainset, n_users, n_items, exclude_seen)
    chunk = max(1, PAIRS_PER_CHUNK // max(1, n_items))
    keep_row = None
    if keep_items is not None and not isinstance(keep_items, tuple):
        keep_row = torch.zeros(n_items, dtype=torch.bool, device=dev)
        keep_row[torch.from_numpy(np.ascontiguousarray(keep_items, dtype=np.int64)).to(dev)] = True
    for lo in range(0, len(u), chunk):
        uc = torch.from_numpy(u[lo:lo + chunk]).to(dev)
        c = int(uc.numel())
        keep = _unseen_mask(uc, n_items, excl, dev)
        if keep_row is not None:
            keep &= keep_row[None, :]
        elif keep_items is not None:
            keep &= _kept_mask(keep_items[0], keep_items[1], lo, c, n_items, dev)
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
        yield lo, c, seg.to(torch.int32), i_ids, scores


def pairs(score_fn, trainset, k, users, exclude_seen, device=None, keep_items=None, after=None):
    """Pair route: per user chunk, the unexcluded (user, item) list built on the device, scored by `score_fn(u_ids, i_ids)` (int32 rows
    of the user / item tower tables -> [P, 1] scores) and ranked by amar_topk_segmented_f32.
    keep_items (None: every item) restricts the list to candidates, as `check_candidates` returns them: item rows (one set for
    every user, a bool row ANDed into the chunk's mask) or a CSR (ptr, rows) over the listed users (a mask per chunk).  Only kept
    pairs are scored.
    after (None: from the start) = (item rows int32 [m], scores float32 [m]) on the device, one cursor per listed user as
    `check_after` reads them: every list starts strictly after its cursor (amar_topk_segmented_after_f32)."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    dev = device or default_device()
    out_i, out_s = [], []
    for lo, c, seg, i_ids, scores in _scored_chunks(score_fn, trainset, u, exclude_seen, dev, keep_items):
        if after is None:
            items, sc = capi.topk_segmented(seg, i_ids, scores, k)
        else:
            items, sc = capi.topk_segmented_after(seg, i_ids, scores, k, after[0][lo:lo + c], after[1][lo:lo + c])
        out_i.append(items)
        out_s.append(sc)
    return _finish(u, torch.cat(out_i), torch.cat(out_s), n_users)


# -- paging (amar_recommend_after_f32 / amar_topk_segmented_after_f32): "the next page", and lists longer than K_MAX ------------------
DEEP_K_MAX = 1024                    # recommend_deep: ceil(k / K_MAX) chained pages; K_MAX stays the length of one launch's list


def check_deep_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= DEEP_K_MAX:
        raise ValueError("k must be an integer in [1, {}] (got {!r})".format(DEEP_K_MAX, k))
    return int(k)


def page_sizes(k):
    """The lengths of the chained pages of a list of k: whole pages of K_MAX, then the rest."""
    return [min(K_MAX, k - at) for at in range(0, k, K_MAX)]


def check_after(after, n_listed, n_users, n_items):
    """The `after` argument of `recommend_after`, checked: (items, scores) with one entry per listed user — items integer node ids
    as `recommend()` returns them (|U|..|U|+|I|-1, or -1: the padding of an exhausted list), scores numbers that are not NaN (the
    infinities are the start and the end).  Returns the host cursor (item rows int32 [n_listed] with -1 kept, scores float32
    [n_listed]).  ValueError, naming `after`, for anything else."""
    if isinstance(after, (str, bytes, dict)) or not hasattr(after, '__len__') or len(after) != 2:
        raise ValueError("after must be a pair (items, scores) with one entry per listed user")
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    try:
        items, scores = host(after[0]).reshape(-1), host(after[1]).reshape(-1)
    except (ValueError, TypeError):
        raise ValueError("after must be a pair (items, scores) of 1-D sequences")
    if len(items) != n_listed or len(scores) != n_listed:
        raise ValueError("after must hold one item and one score per listed user ({} items and {} scores for {} users)".format(
            len(items), len(scores), n_listed))
    if items.size and (items.dtype == np.bool_ or not np.issubdtype(items.dtype, np.integer)):
        raise ValueError("after: the items must be integer node ids")
    if scores.size and (scores.dtype == np.bool_ or not (np.issubdtype(scores.dtype, np.floating) or np.issubdtype(scores.dtype, np.integer))):
        raise ValueError("after: the scores must be numbers")
    items = items.astype(np.int64)
    real = items[items != -1]
    if real.size and (real.min() < n_users or real.max() >= n_users + n_items):
        raise ValueError("after: the items must be node ids in [{}, {}) or -1".format(n_users, n_users + n_items))
    scores = scores.astype(np.float32)
    if np.isnan(scores).any():
        raise ValueError("after: a NaN score is no position in a ranking")
    return np.where(items >= 0, items - n_users, -1).astype(np.int32), scores


def _cursor_device(after, dev):
    return torch.from_numpy(after[0]).to(dev), torch.from_numpy(after[1]).to(dev)


def after_fused(towers, plan, trainset, k, users, exclude_seen, after):
    """One amar_recommend_after_f32 call over the split towers: `fused` from the cursors `after` (host item rows / scores of
    `check_after`, one per listed user)."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen, None if users is None else u)
    items, scores = capi.recommend_after(*head, k, *_cursor_device(after, towers[0].device), **kw)
    return _finish(u, items, scores, n_users)


def deep_fused(towers, plan, trainset, k, users, exclude_seen):
    """The first k entries of every listed user's ranking, k <= DEEP_K_MAX, fused: amar_recommend_f32 for the first page, then one
    amar_recommend_after_f32 launch per further page of K_MAX with the previous page's last column as its cursor.  The cursors are
    slices of the previous outputs: they never leave the device and nothing waits between the pages.  Every page scores the whole
    catalogue again."""
    n_users, n_items = _sizes(trainset)
    k = check_deep_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen, None if users is None else u)
    out_i, out_s = [], []
    for page_k in page_sizes(k):
        if not out_i:
            items, scores = capi.recommend(*head, page_k, **kw)
        else:
            items, scores = capi.recommend_after(*head, page_k, out_i[-1][:, -1].contiguous(), out_s[-1][:, -1].contiguous(), **kw)
        out_i.append(items)
        out_s.append(scores)
    return _finish(u, torch.cat(out_i, 1), torch.cat(out_s, 1), n_users)


def deep_pairs(score_fn, trainset, k, users, exclude_seen, device=None):
    """`deep_fused` on the pair route: every user chunk is scored ONCE (`_scored_chunks`) and ranked page by page on the same scores,
    amar_topk_segmented_f32 first and amar_topk_segmented_after_f32 from each page's last column."""
    n_users, n_items = _sizes(trainset)
    k = check_deep_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    dev = device or default_device()
    out_i, out_s = [], []
    for lo, c, seg, i_ids, scores in _scored_chunks(score_fn, trainset, u, exclude_seen, dev):
        page_i, page_s = [], []
        for page_k in page_sizes(k):
            if not page_i:
                items, sc = capi.topk_segmented(seg, i_ids, scores, page_k)
            else:
                items, sc = capi.topk_segmented_after(seg, i_ids, scores, page_k, page_i[-1][:, -1].contiguous(), page_s[-1][:, -1].contiguous())
            page_i.append(items)
            page_s.append(sc)
        out_i.append(torch.cat(page_i, 1))
        out_s.append(torch.cat(page_s, 1))
    return _finish(u, torch.cat(out_i), torch.cat(out_s), n_users)


# -- candidates (amar_recommend_among_f32): "the best k among THESE items" ----------------------------------------------------------
def _candidate_rows(c, n_users, n_items, what):
    """One candidate set as sorted, distinct item rows (int64): a bool mask of length |I| or integer item node ids."""
    try:
        a = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
    except ValueError:                                                    # ragged: neither a set nor one set per user
        a = np.empty(0, dtype=object)
    if a.dtype == np.bool_:
        if a.ndim != 1 or len(a) != n_items:
            raise ValueError("{}: a boolean mask must have one entry per item ({} items, shape {})".format(what, n_items, a.shape))
        return np.flatnonzero(a).astype(np.int64)
    if a.ndim != 1 or a.dtype == object:
        raise ValueError("{} must be a 1-D sequence of item node ids, a boolean mask over the items, or one such sequence per listed "
                         "user".format(what))
    return np.unique(check_ids(a, n_users, n_users + n_items, what)) - n_users


def check_candidates(candidates, n_users, n_items, n_listed=None):
    """The `candidates` argument of `recommend_among`, checked and in the form the routes take:
      * a 1-D integer sequence of item NODE ids (|U|..|U|+|I|-1: what `recommend()` returns and `similar_items(items=)` takes;
        duplicates collapse, the order does not matter) or a boolean mask of length |I| -> item rows, int64, ascending and distinct:
        one set for every user;
      * a sequence of such sequences, one per listed user (`n_listed` of them, in the order of `users`) -> a CSR (ptr int64
        [n_listed + 1], item rows int64 ascending and distinct per user): per-user candidates.
    ValueError, naming `candidates`, for anything else: a non-integer dtype, ids out of range, a mask of the wrong length, a per-user
    list whose length is not the number of listed users."""
    what = 'candidates'
    if isinstance(candidates, torch.Tensor):
        candidates = candidates.detach().cpu().numpy()
    if candidates is None or isinstance(candidates, (str, bytes, dict)) or not hasattr(candidates, '__len__'):
        raise ValueError("{} must be a sequence of item node ids, a boolean mask over the items, or one such sequence per listed "
                         "user".format(what))
    if isinstance(candidates, np.ndarray):
        nested = candidates.ndim == 2
    else:
        nested = len(candidates) > 0 and all(hasattr(c, '__len__') and not isinstance(c, (str, bytes, dict)) for c in candidates)
    if not nested:
        return _candidate_rows(candidates, n_users, n_items, what)
    if n_listed is not None and len(candidates) != n_listed:
        raise ValueError("{}: per-user candidates need one sequence per listed user ({} users, {} sequences)".format(
            what, n_listed, len(candidates)))
    segs = [_candidate_rows(c, n_users, n_items, what) for c in candidates]
    ptr = np.zeros(len(segs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in segs], out=ptr[1:])
    return ptr, (np.concatenate(segs) if segs else np.zeros(0, dtype=np.int64))


def items_with_properties(trainset, any_of=None, all_of=None, none_of=None):
    """Sorted item node ids of the items whose properties (`item_property_csr(trainset)`, property indices 0..|P|-1 as that CSR numbers
    them) pass the filter: at least one of `any_of`, every one of `all_of`, none of `none_of`; an argument left at None does not
    constrain.  ValueError for a trainset without properties and for indices outside 0..|P|-1.  Pure numpy: feed the result to
    `recommend_among(candidates=...)`."""
    csr = item_property_csr(trainset)
    if csr is None:
        raise ValueError("items_with_properties: the trainset's graph has no item properties")
    ptr, props, df, _ = csr
    n_users, n_items = _sizes(trainset)
    n_props = len(df)
    item_of = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(ptr))
    passed = np.ones(n_items, dtype=bool)
    for name, chosen in (('any_of', any_of), ('all_of', all_of), ('none_of', none_of)):
        if chosen is None:
            continue
        if isinstance(chosen, (str, bytes, dict)) or np.ndim(chosen) != 1:
            raise ValueError("items_with_properties: {} must be a 1-D sequence of property indices".format(name))
        p = np.unique(check_ids(chosen, 0, n_props, name, "items_with_properties: {what} must be integer property indices",
                                "items_with_properties: {what} must lie in [{lo}, {hi}) (got {min}..{max})"))
        held = np.bincount(item_of[np.isin(props, p)], minlength=n_items)          # how many of the chosen ones every item has
        passed &= (held > 0) if name == 'any_of' else ((held == len(p)) if name == 'all_of' else (held == 0))
    return np.flatnonzero(passed).astype(np.int64) + n_users


def among_fused(towers, plan, trainset, cand_rows, k, users, exclude_seen):
    """One amar_recommend_among_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in): `fused` with the tile loop
    over `cand_rows` (host item rows, ascending and distinct: `check_candidates`) instead of the catalogue."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen, None if users is None else u)
    items, scores = capi.recommend_among(*head, k, cand_rows, **kw)
    return _finish(u, items, scores, n_users)


# -- per-user candidate lists (amar_recommend_lists_f32): "the best k of THIS user's candidates" --------------------------------------
def _is_padded_lists(c):
    """A 2-D integer array or tensor [m, P] of node ids, -1 padded: the shape `recommend()`, `similar_items()` and
    `device_lists()` hand out."""
    if isinstance(c, torch.Tensor):
        return c.dim() == 2 and not c.dtype.is_floating_point and c.dtype != torch.bool and not c.dtype.is_complex
    return isinstance(c, np.ndarray) and c.ndim == 2 and c.dtype != np.bool_ and np.issubdtype(c.dtype, np.integer)


def check_candidate_lists(candidates, n_users, n_items, n_listed):
    """The `candidates` argument of `recommend_from`, checked and as a CSR over the listed users: (ptr int64 [n_listed + 1], item
    rows int64, ascending and distinct inside every list).  It takes
      * one sequence of item node ids (|U|..|U|+|I|-1, any order, duplicates collapse; or a boolean mask over the items) per listed
        user, in the order of `users`: the per-user form of `check_candidates`, with its ValueErrors;
      * a 2-D integer array or HOST tensor [n_listed, P] of node ids padded with -1 (any order, duplicates collapse).
    A DEVICE tensor [n_listed, P] is not read here: the shape and the dtype are checked and the tensor itself comes back
    (`device_candidate_csr` turns it into the CSR where it is).  One flat sequence is refused: a set for every user is
    `recommend_among`'s."""
    what = 'candidates'
    if candidates is None or isinstance(candidates, (str, bytes, dict)) or not hasattr(candidates, '__len__'):
        check_candidates(candidates, n_users, n_items)                    # raises
    if isinstance(candidates, torch.Tensor) and (candidates.is_cuda or candidates.dim() == 2):
        if not _is_padded_lists(candidates):
            raise ValueError("{}: a tensor must be a 2-D integer tensor [listed users, P] of item node ids, -1 padded".format(what))
        if candidates.shape[0] != n_listed:
            raise ValueError("{}: per-user candidates need one sequence per listed user ({} users, {} sequences)".format(
                what, n_listed, candidates.shape[0]))
        if candidates.is_cuda:
            return candidates
        candidates = candidates.numpy()
    if _is_padded_lists(candidates):
        if len(candidates) != n_listed:
            raise ValueError("{}: per-user candidates need one sequence per listed user ({} users, {} sequences)".format(
                what, n_listed, len(candidates)))
        candidates = [row[row != -1] for row in candidates]
    got = check_candidates(candidates, n_users, n_items, n_listed=n_listed) if len(candidates) or n_listed else \
        (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if not isinstance(got, tuple):
        raise ValueError("{} must hold one sequence of item node ids per listed user (one set for every user is "
                         "recommend_among's)".format(what))
    return got


def device_candidate_csr(lists, n_users, n_items):
    """A device tensor [m, P] of item node ids (any order, duplicates allowed; an entry that is no item node id of the trainset, the
    -1 padding among them, is no candidate) as the CSR of amar_recommend_lists_f32 on the same device: (ptr int32 [m + 1], item rows
    int32, strictly ascending inside every list).  Sorted, de-duplicated and compacted where it is: no value is read on the host."""
    m, P = int(lists.shape[0]), int(lists.shape[1])
    if m * P >= 1 << 31:
        raise ValueError("candidates: the lists must hold fewer than 2^31 entries together")
    dev = lists.device
    if m == 0 or P == 0:
        return torch.zeros(m + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    rows = lists.to(torch.int64) - n_users
    rows = torch.where((rows >= 0) & (rows < n_items), rows, torch.full_like(rows, n_items))       # n_items: sorts last, is dropped
    rows, _ = torch.sort(rows, dim=1)
    keep = rows < n_items
    keep[:, 1:] &= rows[:, 1:] != rows[:, :-1]
    within = torch.cumsum(keep, dim=1)                                                              # kept entries up to and with this one
    ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    torch.cumsum(within[:, -1], dim=0, out=ptr[1:])
    at = torch.where(keep, ptr[:-1, None] + within - 1, torch.full_like(within, m * P))             # dropped entries: one spare slot
    out = torch.empty(m * P + 1, dtype=torch.int32, device=dev)
    out[at.reshape(-1)] = rows.reshape(-1).to(torch.int32)
    return ptr.to(torch.int32), out[:m * P]


def lists_fused(towers, plan, trainset, lists, k, users, exclude_seen):
    """One amar_recommend_lists_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in): `fused` with every listed
    user walking its own candidates.  `lists`: what `check_candidate_lists` returned, the host CSR or the device tensor."""
    n_users, n_items = _sizes(trainset)
    k = check_k(k)
    u = check_users(users, n_users)
    if len(u) == 0:
        return _empty(k)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen, None if users is None else u)
    if isinstance(lists, torch.Tensor):
        ptr, rows = device_candidate_csr(lists.to(towers[0].device), n_users, n_items)
    else:
        ptr, rows = lists
    items, scores = capi.recommend_lists(*head, k, ptr, rows, **kw)
    return _finish(u, items, scores, n_users)


def evaluate_ranking_sampled(model, trainset, test_ratings, ks, n_negatives=99, seed=0, users=None):
    """The 1 + N sampled-negatives protocol: every listed user (all by default) that has a held-out positive ranks its held-out items
    against `n_negatives` items it rated neither in training nor in test (utilities.metrics.sampled_negatives: uniform without
    replacement, a function of `seed` and the user alone), and Precision / Recall / NDCG / HitRate @k are taken over those short
    lists: HR@10 / NDCG@10 against 99 negatives as most implicit-feedback papers report them.  One `recommend_from` call with the
    lists kept on the device, scored by amar_rank_metrics_f64.  Returns the dict of `evaluate_ranking`, same keys; users without a
    held-out positive are skipped and counted.  With n_negatives >= every user's unrated items, and test ratings that hold no
    disliked pair (an item rated in test is never drawn, so a label-0 one is no candidate at all), it is `evaluate_ranking` itself."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics, full_ranking_metrics_device, sampled_negatives
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("evaluate_ranking_sampled needs at least one k")
    k = check_k(max(ks))
    n_users, n_items = _sizes(trainset)
    u = check_users(users, n_users)
    drawn_users, drawn = sampled_negatives(trainset, test_ratings, n_negatives, seed)
    row_of = np.full(n_users, -1, dtype=np.int64)
    row_of[drawn_users] = np.arange(len(drawn_users))
    has = row_of[u] >= 0
    lists = np.full((len(u), max(1, drawn.shape[1])), -1, dtype=np.int64)                  # no held-out positive: an empty list
    lists[has, :drawn.shape[1]] = drawn[row_of[u[has]]]
    with device_lists():
        u, items, _ = model.recommend_from(trainset, lists, k=k, users=users)
    if len(u) == 0:
        return full_ranking_metrics(u, items, test_ratings, ks)
    return full_ranking_metrics_device(None if users is None else u, items.contiguous(), test_ratings, ks, n_users, n_items)


# -- similarity search (amar_nearest_f32): "which rows of this table are like these vectors?" ---------------------------------------
METRICS = ('dot', 'cosine')


def check_metric(metric):
    if metric not in METRICS:
        raise ValueError("metric must be one of {} (got {!r})".format(METRICS, metric))
    return metric


def check_width(d, what='vectors'):
    """The widths amar_nearest_f32 takes: d % 4 == 0, 4 <= d <= 512."""
    if not capi.nearest_supported(int(d), 1):
        raise NotImplementedError("similarity search takes widths that are multiples of 4 in [4, {}]: the {} are {} wide".format(
            capi.NEAREST_MAX_D, what, int(d)))
    return int(d)


def lists_csr(lists, n_rows, what='exclude'):
    """Per-query row lists as the exclusion CSR of amar_nearest_f32: (ptr int32 [m+1], rows int32), every segment sorted ascending and
    de-duplicated, values checked against 0..n_rows-1."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    segs = []
    for j, l in enumerate(lists):
        a = np.unique(np.asarray(l, dtype=np.int64).reshape(-1)) if len(l) else np.zeros(0, dtype=np.int64)
        if a.size and (a[0] < 0 or a[-1] >= n_rows):
            raise ValueError("{}: rows must lie in [0, {}) (got {}..{})".format(what, n_rows, int(a[0]), int(a[-1])))
        segs.append(a)
        ptr[j + 1] = ptr[j] + a.size
    rows = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int64)
    return ptr.astype(np.int32), rows.astype(np.int32)


def _as_device_matrix(x, dev, name):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    if t.dim() != 2:
        raise ValueError("{} must be a 2-D [n, d] array".format(name))
    t = t.to(device=dev, dtype=torch.float32)
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.stride(0) % 4 or t.data_ptr() % 16:                # the kernel reads float4s: rows on 16-byte boundaries
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def nearest(queries, table, k=10, metric='cosine', exclude=None, query_rows=None):
    """The k rows of `table` [n, d] most similar to every query vector of `queries` [m, d] (host or device arrays) under `metric`
    ('cosine' or 'dot'; a zero vector scores 0 under cosine).  `exclude`: one sequence of table rows per query that must not be
    returned, or an (excl_ptr, excl_rows) CSR already on the device.  `query_rows`: int32 device rows of `queries` to search for
    (all rows by default).  Returns (rows int64 [m, k] (-1 padded), scores float32 [m, k] (-inf padded)) on the host, ordered by
    score descending then row ascending; inside ``device_lists()`` the device tensors (rows int32)."""
    k = check_k(k)
    check_metric(metric)
    dev = table.device if isinstance(table, torch.Tensor) and table.is_cuda else (
        queries.device if isinstance(queries, torch.Tensor) and queries.is_cuda else default_device())
    q, t = _as_device_matrix(queries, dev, 'queries'), _as_device_matrix(table, dev, 'table')
    if q.shape[1] != t.shape[1]:
        raise ValueError("queries are {} wide, the table {}".format(q.shape[1], t.shape[1]))
    check_width(t.shape[1])
    m = int(query_rows.numel()) if query_rows is not None else int(q.shape[0])
    ptr = rows = None
    if exclude is not None:
        if isinstance(exclude, tuple) and len(exclude) == 2 and isinstance(exclude[0], torch.Tensor):
            ptr, rows = exclude
        else:
            if len(exclude) != m:
                raise ValueError("exclude must hold one list per query ({} lists for {} queries)".format(len(exclude), m))
            p, r = lists_csr(exclude, int(t.shape[0]))
            ptr, rows = torch.from_numpy(p).to(dev), torch.from_numpy(r).to(dev)
    out_rows, out_scores = capi.nearest(q, t, k, metric=metric, query_rows=query_rows, excl_ptr=ptr, excl_rows=rows)
    if _ON_DEVICE:
        return out_rows, out_scores
    return out_rows.cpu().numpy().astype(np.int64), out_scores.cpu().numpy().astype(np.float32)


def check_trade_off(trade_off):
    if isinstance(trade_off, bool) or not isinstance(trade_off, (int, float, np.integer, np.floating)) or not 0.0 <= float(trade_off) <= 1.0:
        raise ValueError("trade_off must be a number in [0, 1] (got {!r})".format(trade_off))
    return float(trade_off)


def rerank_mmr(items, scores, table, k, trade_off=0.7, metric='cosine'):
    """Greedy Maximal Marginal Relevance over device pools, one amar_rerank_mmr_f32 launch: `items` int32 [m, P] rows of `table`
    (the valid entries as a prefix, the rest -1; P <= 64), `scores` float32 [m, P], `table` float32 [n, d].  Step 0 takes the best
    score; every later step the candidate that maximises trade_off * rel - (1 - trade_off) * max sim(candidate, chosen), rel the
    scores min-max normalised per pool, ties to the smaller pool position.  Returns the device tensors (items int32 [m, k] in
    selection order, -1 padded; scores float32 [m, k]: the pool's own scores of the chosen items, -inf padded)."""
    k = check_k(k)
    check_metric(metric)
    trade_off = check_trade_off(trade_off)
    if items.dim() != 2 or tuple(items.shape) != tuple(scores.shape):
        raise ValueError("items and scores must be [m, P] tensors of the same shape")
    if not k <= int(items.shape[1]) <= K_MAX:
        raise ValueError("the pools must hold between k = {} and {} candidates (got {})".format(k, K_MAX, int(items.shape[1])))
    check_width(table.shape[1], 'item vectors')
    table = _as_device_matrix(table, items.device, 'table')
    return capi.rerank_mmr(items.to(torch.int32).contiguous(), scores.to(torch.float32).contiguous(), table, k,
                           trade_off=trade_off, metric=metric)


def check_smoothing(smoothing):
    if isinstance(smoothing, bool) or not isinstance(smoothing, (int, float, np.integer, np.floating)) or not 0.0 < float(np.float32(smoothing)) < 1.0:
        raise ValueError("smoothing must be a number in (0, 1) (got {!r})".format(smoothing))
    return float(smoothing)


def check_pool(pool, k):
    if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)) or not k <= int(pool) <= K_MAX:
        raise ValueError("pool must be an integer in [k = {}, {}] (got {!r})".format(k, K_MAX, pool))
    return int(pool)


def rerank_calibrated(items, scores, users, liked, cats, k, trade_off=0.5, smoothing=0.01):
    """Greedy calibrated re-ranking over device pools, one amar_rerank_calibrated_f32 launch: `items` int32 [m, P] item rows (-1
    padded; P <= 64), `scores` float32 [m, P], `users` int32 [m] on the device or None for the identity, `liked` = (ptr, items) of
    `liked_csr` on the device, `cats` = (ptr, ids, G, longest row) of `item_category_csr` on the device.  Every step takes the
    candidate that maximises trade_off * rel - (1 - trade_off) * C(p, chosen + candidate): rel the scores min-max normalised per
    pool, C the smoothed Kullback-Leibler distance between the categories of what the user liked and of the list; ties to the
    smaller pool position.  Returns the device tensors (items int32 [m, k] in selection order, -1 padded; scores float32 [m, k]:
    the pool's own scores of the chosen items, -inf padded)."""
    k = check_k(k)
    trade_off, smoothing = check_trade_off(trade_off), check_smoothing(smoothing)
    if items.dim() != 2 or tuple(items.shape) != tuple(scores.shape):
        raise ValueError("items and scores must be [m, P] tensors of the same shape")
    if not k <= int(items.shape[1]) <= K_MAX:
        raise ValueError("the pools must hold between k = {} and {} candidates (got {})".format(k, K_MAX, int(items.shape[1])))
    return capi.rerank_calibrated(items.to(torch.int32).contiguous(), scores.to(torch.float32).contiguous(), liked[0], liked[1],
                                  cats[0], cats[1], cats[2], k, trade_off=trade_off, smoothing=smoothing, users=users, max_cat_row=cats[3])


def _item_rows_device(items, n_users, n_items, device, rows=None, widths=None):
    """An [m, K] host array of item node ids (-1 padded) as int32 item rows on `device` (-1 stays -1).  rows: the m the caller
    expects; widths: the (least, greatest) K it takes; None: any."""
    a = np.asarray(items.cpu() if isinstance(items, torch.Tensor) else items)
    if a.ndim != 2 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("items must be a 2-D [m, K] array of integer node ids")
    if (rows is not None and a.shape[0] != rows) or (widths is not None and not widths[0] <= a.shape[1] <= widths[1]):
        raise ValueError("items must hold one row of {}..{} node ids per user ({} rows for {} users)".format(widths[0], widths[1], a.shape[0], rows))
    a = a.astype(np.int64)
    real = a[a != -1]
    if real.size and (real.min() < n_users or real.max() >= n_users + n_items):
        raise ValueError("items must be node ids in [{}, {}) or -1".format(n_users, n_users + n_items))
    return torch.from_numpy(np.where(a >= 0, a - n_users, -1).astype(np.int32)).to(device)


def similar_rows(table, rows, k, metric, exclude_self, base):
    """`nearest` of rows `rows` (host int64) of a device table against the table itself; neighbours come back as node ids (+ base)."""
    k = check_k(k)
    check_metric(metric)
    if len(rows) == 0:
        return (np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)) if not _ON_DEVICE else (
            torch.zeros((0, k), dtype=torch.int32, device=table.device), torch.zeros((0, k), dtype=torch.float32, device=table.device))
    dev = table.device
    q_rows = torch.from_numpy(rows.astype(np.int32)).to(dev)
    excl = None
    if exclude_self:                                         # segment j = {rows[j]}
        excl = (torch.arange(len(rows) + 1, dtype=torch.int32, device=dev), q_rows)
    nb, sc = nearest(table, table, k, metric, exclude=excl, query_rows=q_rows)
    if _ON_DEVICE:
        return nb, sc
    return np.where(nb >= 0, nb + base, -1), sc


def profile_queries(table, liked_rows):
    """Float32 mean of the liked rows of every profile, on the device: [m, d].  liked_rows: list of host int64 row arrays, none empty."""
    dev = table.device
    sizes = np.array([len(l) for l in liked_rows], dtype=np.int64)
    # profiles padded to the longest one and summed along the padding (no atomics: the same bits on every run)
    idx = np.zeros((len(liked_rows), int(sizes.max())), dtype=np.int64)
    for j, l in enumerate(liked_rows):
        idx[j, :len(l)] = l
    keep = torch.from_numpy((np.arange(idx.shape[1])[None, :] < sizes[:, None]).astype(np.float32)).to(dev)
    rows = table.to(torch.float32)[torch.from_numpy(idx).to(dev)] * keep[:, :, None]
    return rows.sum(1) / torch.from_numpy(sizes.astype(np.float32)).to(dev)[:, None]


EXPLAIN_KEYS = ('users', 'items', 'evidence', 'evidence_sim', 'properties', 'property_score', 'property_support')


def check_count(n, lo, hi, what):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not lo <= int(n) <= hi:
        raise ValueError("{} must be an integer in [{}, {}] (got {!r})".format(what, lo, hi, n))
    return int(n)


def explain_lists(lists, users, liked, table, props, n_evidence, n_properties, metric='cosine'):
    """One amar_explain_f32 launch over device lists (int32 [m, K] rows of `table`, -1 padded; `users` int32 [m] on the device or
    None for the identity): `liked` = (ptr, items) of `liked_csr` on the device, `props` = (ptr, ids, weights, longest row) of the
    item-property CSR on the device or None.  Returns the device tensors (evidence int32 [m, K, E], evidence_sim float32,
    properties int32 [m, K, Q], property_score float32, property_support int32); without `props` Q is 0.  The caller has checked the
    table's width (`check_width`); the library refuses any other."""
    table = _as_device_matrix(table, lists.device, 'table')
    if props is None:
        return capi.explain(lists, liked[0], liked[1], table, n_evidence, 0, metric=check_metric(metric), users=users)
    if props[3] > capi.EXPLAIN_MAX_PROP_ROW:
        raise NotImplementedError("explain takes items with at most {} properties: the longest row has {}".format(
            capi.EXPLAIN_MAX_PROP_ROW, props[3]))
    return capi.explain(lists, liked[0], liked[1], table, n_evidence, n_properties, metric=check_metric(metric), users=users,
                        prop_ptr=props[0], prop_ids=props[1], prop_weight=props[2], max_prop_row=props[3])


# -- group recommendation (amar_recommend_group_f32): "what should WE watch?" --------------------------------------------------------
def check_strategy(name):
    if not isinstance(name, str) or name not in capi.GROUP_STRATEGIES:
        raise ValueError("strategy must be one of {} (got {!r})".format(sorted(capi.GROUP_STRATEGIES), name))
    return name


def check_min_score(x):
    """The veto floor as a float: None = -inf (no veto); a finite number or -inf; NaN, +inf and non-numbers are ValueErrors."""
    if x is None:
        return float('-inf')
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or np.isnan(x) or float(x) == float('inf'):
        raise ValueError("min_score must be None, a finite number or -inf (got {!r})".format(x))
    return float(x)


def group_csr(groups, n_users):
    """A sequence of user-index sequences as (ptr int32 [g + 1], users int32): the members of every group sorted ascending, so that
    a result never depends on the order a caller lists people in.  Empty groups are allowed.  ValueError for a duplicate member, a
    non-integer or out-of-range index, or `groups` that is not a sequence of sequences."""
    not_nested = "groups must be a sequence of sequences of user indices"
    if isinstance(groups, (str, bytes, dict)) or not hasattr(groups, '__len__') or not hasattr(groups, '__iter__'):
        raise ValueError(not_nested)
    ptr, segs = np.zeros(len(groups) + 1, dtype=np.int64), []
    for j, members in enumerate(groups):
        if isinstance(members, (str, bytes, dict)) or not hasattr(members, '__len__') or np.ndim(members) != 1:
            raise ValueError(not_nested)
        a = np.sort(check_ids(members, 0, n_users, 'group members', "{what} must be integer indices",
                              "user indices must lie in [{lo}, {hi}) (got {min}..{max})"))
        if a.size > 1 and (a[1:] == a[:-1]).any():
            raise ValueError("group {} lists a member twice".format(j))
        segs.append(a)
        ptr[j + 1] = ptr[j] + a.size
    users = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int64)
    return ptr.astype(np.int32), users.astype(np.int32)


def group_exclusion_csr(ratings, grp_ptr, grp_users, n_users, n_items):
    """The union of the members' training items per group, as a CSR over groups: (ptr int64 [g + 1], items int64) with item ROWS
    sorted and de-duplicated per group (`exclusion_csr` per user, then the union)."""
    ptr, items = exclusion_csr(ratings, n_users, n_items)
    grp_ptr, members = np.asarray(grp_ptr, dtype=np.int64), np.asarray(grp_users, dtype=np.int64)
    g = len(grp_ptr) - 1
    cnt = ptr[members + 1] - ptr[members]
    total = int(cnt.sum())
    out = np.zeros(g + 1, dtype=np.int64)
    if total == 0:
        return out, np.zeros(0, dtype=np.int64)
    group_of = np.repeat(np.arange(g, dtype=np.int64), np.diff(grp_ptr))
    pos = np.repeat(ptr[members] - (np.cumsum(cnt) - cnt), cnt) + np.arange(total, dtype=np.int64)
    key = np.unique(np.repeat(group_of, cnt) * n_items + items[pos])      # sorted by (group, item), duplicates gone
    np.cumsum(np.bincount(key // n_items, minlength=g), out=out[1:])
    return out, key % n_items


def _i32_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def group_fused(towers, plan, grp_ptr, grp_users, excl, k, strategy, min_score):
    """One amar_recommend_group_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in); `excl` = the host CSR
    over groups or None.  Returns the device tensors (item rows int32 [g, k], scores float32 [g, k])."""
    head, _ = _ranker_args(towers, plan)
    dev = head[0].device
    return capi.recommend_group(*head, k, _i32_device(grp_ptr, dev), _i32_device(grp_users, dev), strategy=strategy, min_score=min_score,
                                excl_ptr=None if excl is None else _i32_device(excl[0], dev),
                                excl_items=None if excl is None else _i32_device(excl[1], dev))


MEMBER_SCORE_GROUPS = 32             # groups whose chosen items share one compact table in `fused_member_scores`


def fused_member_scores(towers, plan, grp_ptr, grp_users, rows, per):
    """Every member's own score of every chosen item of its group (rows int64 [g, k] item rows, -1 padded), written into per[j]
    [n_members_j, k], with the bits the fused ranking gave them: the ranking kernel itself scores them.  (The pair stage would not
    do: for some heads it multiplies on split bf16 operands, a few float32 ulps away.)  Per chunk of MEMBER_SCORE_GROUPS groups the
    chosen items' Ti rows form one compact table, every member is a group of one, and its exclusion segment is the rest of the
    table: one amar_recommend_group_f32 launch per chunk, nothing of size members x |I|."""
    (tu, ti, *rest), _ = _ranker_args(towers, plan)
    g, k = rows.shape
    sizes = np.diff(np.asarray(grp_ptr, dtype=np.int64))
    for lo in range(0, g, MEMBER_SCORE_GROUPS):
        hi = min(g, lo + MEMBER_SCORE_GROUPS)
        c, m0, m1 = hi - lo, int(grp_ptr[lo]), int(grp_ptr[hi])
        valid = rows[lo:hi] >= 0                                          # [c, k]
        if m1 == m0 or not valid.any():
            continue
        table = ti[torch.from_numpy(np.maximum(rows[lo:hi], 0).reshape(-1)).to(ti.device)]      # compact row q * k + r = rows[lo + q, r]
        group_of = np.repeat(np.arange(c), sizes[lo:hi])                  # member -> its group in the chunk
        allowed = np.zeros((m1 - m0, c, k), dtype=bool)
        allowed[np.arange(m1 - m0), group_of] = valid[group_of]
        banned = ~allowed.reshape(m1 - m0, c * k)
        e_ptr = np.zeros(m1 - m0 + 1, dtype=np.int64)
        np.cumsum(banned.sum(1), out=e_ptr[1:])
        items, scores = capi.recommend_group(tu, table, *rest, k, _i32_device(np.arange(m1 - m0 + 1), tu.device),
                                             _i32_device(grp_users[m0:m1], tu.device), strategy='max',
                                             excl_ptr=_i32_device(e_ptr, tu.device), excl_items=_i32_device(np.nonzero(banned)[1], tu.device))
        items, scores = items.cpu().numpy(), scores.cpu().numpy()
        for s_, q in enumerate(group_of.tolist()):
            got = items[s_] >= 0
            per[lo + q][s_ + m0 - int(grp_ptr[lo + q]), items[s_][got] - q * k] = scores[s_][got]


def group_pairs(score_fn, n_items, grp_ptr, grp_users, excl, k, strategy, min_score, dev):
    """Pair route of the group ranking: per chunk of groups, members x all items scored by `score_fn(u_ids, i_ids)`, aggregated on
    the device by a loop over the member position (acc = acc + s_t elementwise, or the running minimum / maximum: the float32 order
    of amar_recommend_group_f32, not a tree sum), divided by the group size, the group's union and the vetoed items masked out,
    then amar_topk_segmented_f32.  Returns the device tensors (item rows int32 [g, k], scores float32 [g, k])."""
    g = len(grp_ptr) - 1
    sizes = np.diff(np.asarray(grp_ptr, dtype=np.int64))
    budget = max(1, PAIRS_PER_CHUNK // max(1, n_items))              # member rows scored per chunk
    all_items = torch.arange(n_items, dtype=torch.int32, device=dev)
    out_i, out_s = [], []
    lo = 0
    while lo < g:
        hi = lo + 1
        while hi < g and int(grp_ptr[hi + 1] - grp_ptr[lo]) <= budget:
            hi += 1
        c, m0, m1 = hi - lo, int(grp_ptr[lo]), int(grp_ptr[hi])
        size = sizes[lo:hi]
        keep = torch.ones((c, n_items), dtype=torch.bool, device=dev)
        agg = torch.zeros((c, n_items), dtype=torch.float32, device=dev)
        if m1 > m0 and n_items:
            members = _i32_device(grp_users[m0:m1], dev)
            s = score_fn(torch.repeat_interleave(members, n_items).contiguous(), all_items.repeat(m1 - m0).contiguous()).reshape(m1 - m0, n_items)
            low = torch.zeros_like(agg)
            first = np.asarray(grp_ptr[lo:hi], dtype=np.int64) - m0
            for t in range(int(size.max())):                         # member position t of every group that has one
                has = np.nonzero(size > t)[0]
                rows, st = torch.from_numpy(has).to(dev), s[torch.from_numpy(first[has] + t).to(dev)]
                if t == 0:
                    agg[rows], low[rows] = st, st
                    continue
                at = agg[rows]
                agg[rows] = at + st if strategy == 'mean' else (torch.minimum(at, st) if strategy == 'min' else torch.maximum(at, st))
                low[rows] = torch.minimum(low[rows], st)
            if strategy == 'mean':
                # the quotient in float64, rounded once more to float32: the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits)
                n = torch.from_numpy(np.maximum(size, 1).astype(np.float64)).to(dev)[:, None]
                agg = (agg.to(torch.float64) / n).to(torch.float32)
            keep &= low >= min_score
        keep &= torch.from_numpy(size > 0).to(dev)[:, None]
        if excl is not None:
            e0, e1 = int(excl[0][lo]), int(excl[0][hi])
            if e1 > e0:
                rows = np.repeat(np.arange(c), np.diff(np.asarray(excl[0][lo:hi + 1], dtype=np.int64)))
                keep[torch.from_numpy(rows).to(dev), torch.from_numpy(np.asarray(excl[1][e0:e1], dtype=np.int64)).to(dev)] = False
        r, i = keep.nonzero(as_tuple=True)                           # row-major: groups in order, items ascending
        seg = torch.zeros(c + 1, dtype=torch.int64, device=dev)
        torch.cumsum(keep.sum(1), 0, out=seg[1:])
        i_ids, scores = i.to(torch.int32).contiguous(), agg[r, i].contiguous()
        if i_ids.numel() == 0:
            scores = torch.zeros(1, dtype=torch.float32, device=dev)
            i_ids = torch.zeros(1, dtype=torch.int32, device=dev)
        items, sc = capi.topk_segmented(seg.to(torch.int32), i_ids, scores, k)
        out_i.append(items)
        out_s.append(sc)
        lo = hi
    return torch.cat(out_i), torch.cat(out_s)


# -- exact positions (amar_rank_of_f32): "where does THIS item stand for this user?" --------------------------------------------------
RANK_KEYS = ('scores', 'greater', 'eq_before', 'eq_after')


def check_targets_csr(targets_csr, n_entries, n_items):
    """(ptr int64 [n_entries + 1], item rows int64) of a targets CSR over the listed users, checked: rows in 0..n_items-1, ascending
    and distinct inside an entry."""
    ptr, items = (np.asarray(x, dtype=np.int64).reshape(-1) for x in targets_csr)
    if len(ptr) != n_entries + 1 or ptr[0] != 0 or ptr[-1] != len(items) or (np.diff(ptr) < 0).any():
        raise ValueError("targets must be a CSR over the listed users ({} users, {} pointers, {} items)".format(n_entries, len(ptr), len(items)))
    if len(items) and (items.min() < 0 or items.max() >= n_items):
        raise ValueError("target items must be item rows in [0, {})".format(n_items))
    if len(items) > 1:
        inside = np.ones(len(items) - 1, dtype=bool)
        inside[ptr[1:-1][(ptr[1:-1] > 0) & (ptr[1:-1] < len(items))] - 1] = False       # pairs that straddle two entries
        if (np.diff(items)[inside] <= 0).any():
            raise ValueError("the targets of an entry must be ascending and distinct")
    return ptr, items


def rank_of_fused(towers, plan, trainset, users, targets_csr, exclude_seen):
    """One amar_rank_of_f32 call over the split towers (tu [U, c1], ti [I, c1] with b1 folded in): for every listed user (host
    indices; a user may be listed more than once) and every item row of its entry of `targets_csr` = (ptr, item rows) the score and
    the counts of the candidates that score higher / the same with a smaller row / the same with a larger row, among the items
    outside the user's training row (all items with exclude_seen=False).  Returns the four device tensors of `capi.rank_of`, one
    value per target in the CSR's order."""
    n_users, n_items = _sizes(trainset)
    u = check_users(users, n_users)
    ptr, items = check_targets_csr(targets_csr, len(u), n_items)
    head, kw = _ranker_args(towers, plan, trainset, exclude_seen)
    return capi.rank_of(*head, u, ptr, items, **kw)


def rank_of_pairs(score_fn, trainset, users, targets_csr, exclude_seen, device=None):
    """Pair route of `rank_of_fused`, for the hybrids and the heads without a split plan: per user chunk the unexcluded pair list of
    `pairs()` scored by `score_fn`, the targets scored by one more call, and torch comparisons of every candidate row against its
    targets' scores (at most PAIRS_PER_CHUNK comparisons in memory at a time).  The same four outputs in the same order."""
    n_users, n_items = _sizes(trainset)
    u = check_users(users, n_users)
    ptr, items = check_targets_csr(targets_csr, len(u), n_items)
    dev = device or default_device()
    excl = _exclusion_device(trainset, n_users, n_items, exclude_seen)
    n_t = len(items)
    scores = torch.zeros(n_t, dtype=torch.float32, device=dev)
    greater, before, after = (torch.zeros(n_t, dtype=torch.int32, device=dev) for _ in range(3))
    chunk = max(1, PAIRS_PER_CHUNK // max(1, n_items))
    rows_all = torch.arange(n_items, device=dev)[None, :]
    for lo in range(0, len(u), chunk):
        hi = min(len(u), lo + chunk)
        t0, t1 = int(ptr[lo]), int(ptr[hi])
        if t1 == t0:
            continue
        uc = torch.from_numpy(u[lo:hi]).to(dev)
        keep = _unseen_mask(uc, n_items, excl, dev)
        r, i = keep.nonzero(as_tuple=True)
        S = torch.full((hi - lo, n_items), float('nan'), dtype=torch.float32, device=dev)
        if i.numel():
            S[r, i] = score_fn(uc[r].to(torch.int32).contiguous(), i.to(torch.int32).contiguous()).reshape(-1)
        row_of = torch.from_numpy(np.repeat(np.arange(hi - lo), np.diff(ptr[lo:hi + 1]))).to(dev)
        tgt = torch.from_numpy(items[t0:t1]).to(dev)
        s_t = score_fn(uc[row_of].to(torch.int32).contiguous(), tgt.to(torch.int32).contiguous()).reshape(-1)
        scores[t0:t1] = s_t
        for b0 in range(0, t1 - t0, chunk):
            b1 = min(t1 - t0, b0 + chunk)
            rows, st, it = row_of[b0:b1], s_t[b0:b1, None], tgt[b0:b1, None]
            kept, sc = keep[rows], S[rows]
            greater[t0 + b0:t0 + b1] = (kept & (sc > st)).sum(1).to(torch.int32)
            tie = kept & (sc == st)
            before[t0 + b0:t0 + b1] = (tie & (rows_all < it)).sum(1).to(torch.int32)
            after[t0 + b0:t0 + b1] = (tie & (rows_all > it)).sum(1).to(torch.int32)
    return scores, greater, before, after


def rank_of_route(model, trainset, users, targets_csr, exclude_seen):
    """`rank_of_fused` or `rank_of_pairs`, chosen as the model's `recommend()` chooses its route — for amar_rank_of_f32's own capacity:
    its LDS sum is the largest of the three rankers', so a head whose `recommend()` is fused may be counted by pairs here."""
    route = model._group_route(trainset, 'rank_of')
    if route[0] == 'fused':
        return rank_of_fused(route[1], route[2], trainset, users, targets_csr, exclude_seen)
    return rank_of_pairs(route[1], trainset, users, targets_csr, exclude_seen, device=route[2])


# Held-out targets per ratings pair (test ratings, training ratings), built once: R'(u) = relevant(u) \ excl(u) as a host CSR over
# all users and |C(u)|.  Keyed and held like the device CSRs above; the training ratings are checked by identity on every hit.
_HELDOUT_CACHE = {}


def heldout_targets(trainset, test_ratings, exclude_seen=True):
    """(ptr int64 [|U| + 1], item rows int64, n_cand int64 [|U|]): for every user the label-1 test items that are not among its
    training items (all of them with exclude_seen=False), ascending, and the number of items outside its training row."""
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import relevant_csr
    n_users, n_items = _sizes(trainset)
    ratings = trainset.ratings

    def build():
        r_ptr, r_items = relevant_csr(test_ratings, n_users, n_items)
        n_cand = np.full(n_users, n_items, dtype=np.int64)
        if exclude_seen:
            e_ptr, e_items = exclusion_csr(ratings, n_users, n_items)
            n_cand -= np.diff(e_ptr)
            rel = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(r_ptr)) * n_items + r_items
            seen = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(e_ptr)) * n_items + e_items
            rel = np.setdiff1d(rel, seen, assume_unique=True)
            r_ptr = np.zeros(n_users + 1, dtype=np.int64)
            np.cumsum(np.bincount(rel // n_items, minlength=n_users), out=r_ptr[1:])
            r_items = rel % n_items
        try:
            held = weakref.ref(ratings)
        except TypeError:
            held = (lambda o: (lambda: o))(ratings)
        return held, (r_ptr, r_items, n_cand)
    key = (id(test_ratings), np.shape(test_ratings), id(ratings), np.shape(ratings), n_users, n_items, bool(exclude_seen))
    entry = _device_cached(_HELDOUT_CACHE, test_ratings, key, build)
    if entry[0]() is not ratings:                                     # the id of a dead training array, reused
        _HELDOUT_CACHE.pop(key, None)
        entry = _device_cached(_HELDOUT_CACHE, test_ratings, key, build)
    return entry[1]


def heldout_rank_metrics(model, trainset, test_ratings, users, exclude_seen, names):
    """{name: the float64 mean over the evaluated users, 'rank_metrics_users': (evaluated, skipped)} for `names` out of 'auc', 'mrr',
    'map': every listed user's held-out items (`heldout_targets`) ranked exactly in the full catalogue (`rank_of_route`: one
    amar_rank_of_f32 launch on the fused route) and turned into per-user AUC / reciprocal rank / average precision on the device
    (amar_rank_of_metrics_f64).  A user without a held-out item, or without a candidate that is not one, is skipped and counted; with
    nobody evaluated the means are 0."""
    n_users, n_items = _sizes(trainset)
    u = check_users(users, n_users)
    all_ptr, all_items, n_cand = heldout_targets(trainset, test_ratings, exclude_seen)
    cnt = all_ptr[u + 1] - all_ptr[u]
    ptr = np.zeros(len(u) + 1, dtype=np.int64)
    np.cumsum(cnt, out=ptr[1:])
    items = all_items[np.repeat(all_ptr[u] - ptr[:-1], cnt) + np.arange(int(ptr[-1]), dtype=np.int64)]
    mean, evaluated = np.zeros(3), 0
    if len(u):
        flat = rank_of_route(model, trainset, u, (ptr, items), exclude_seen)
        dev = flat[0].device
        values, valid = capi.rank_of_metrics(*flat, _i32_device(ptr, dev), _i32_device(n_cand[u], dev))
        values, valid = values.cpu().numpy(), valid.cpu().numpy() > 0
        evaluated = int(valid.sum())
        if evaluated:
            mean = values[valid].mean(axis=0)
    out = {name: float(mean[('auc', 'mrr', 'map').index(name)]) for name in names}
    out['rank_metrics_users'] = (evaluated, len(u) - evaluated)
    return out


RANK_ITEMS_KEYS = ('rank', 'score', 'ties', 'candidates', 'percentile')


class SimilarSearch:
    """Embedding accessors and similarity search shared by the scoring models.  A model names its spaces (`_embedding_spaces`:
    'graph' = the propagated, reduced node table, 'tower' = the first-stage Dense outputs per entity; the first one is the default)
    and returns the device tables of one (`_embedding_tables(trainset, space)` -> (users [|U|, d], items [|I|, d]))."""

    def _embedding_spaces(self):
        raise NotImplementedError

    # -- full-catalogue top-k: the route.  A model says which object scores and which tables one pass of it reads ---------------
    def _scoring_head(self):
        """The object that scores pairs (the model itself, or its `rs`): `towers(*tables)` per entity, `score_towers(towers, u_ids,
        i_ids)` per pair and, where the head has a fused ranking form, `_ranker_plan` / `_recommend_split` (models/basic.py:BasicRS;
        a head without them always ranks by pairs)."""
        raise NotImplementedError

    def _recommend_tables(self, trainset):
        """The arguments of the head's `towers()` for one pass over the users and items of `trainset`."""
        raise NotImplementedError

    def recommend(self, trainset, k=10, users=None, exclude_seen=True):
        """The k best items of every user in `users` (all users by default) among all items of `trainset` — every training pair of
        `trainset.ratings` excluded unless exclude_seen=False.  Returns (users int64 [m], items int64 [m, k] (node ids, -1 padded),
        scores float32 [m, k] (-inf padded)), see the module's docstring.  k and the users are checked before any tower is computed."""
        check_k(k)
        check_users(users, len(trainset.users))
        route = self._group_route(trainset, 'recommend')
        if route[0] == 'fused':
            return fused(route[1], route[2], trainset, k, users, exclude_seen)
        return pairs(route[1], trainset, k, users, exclude_seen, device=route[2])

    def _recommend_pairs(self, trainset, k=10, users=None, exclude_seen=True, towers=None, keep_items=None):
        """`recommend()` on the pair route, whatever the head (the tests' yardstick of the fused route); `towers`: the head's towers
        where the caller has them, `keep_items`: candidates as `pairs()` takes them."""
        check_k(k)
        check_users(users, len(trainset.users))
        head = self._scoring_head()
        towers = towers if towers is not None else head.towers(*self._recommend_tables(trainset))
        return pairs(lambda u, i: head.score_towers(towers, u, i), trainset, k, users, exclude_seen, device=towers[0].device,
                     keep_items=keep_items)

    # -- paging (amar_recommend_after_f32) -------------------------------------------------------------------------------------
    def recommend_after(self, trainset, after, k=10, users=None, exclude_seen=True):
        """The next page: the k best items (1 <= k <= K_MAX) of every user in `users` (all users by default) that come strictly AFTER
        a position of the user's ranking.  after = (items, scores), one entry per listed user: items are node ids as `recommend()`
        returns them (-1 = an exhausted list: the page is all padding), scores float32; typically `(items[:, -1], scores[:, -1])` of
        the previous page.  The order is `recommend()`'s (score descending, node id ascending), a strict total order, so the page is
        exactly what `recommend()` would return with the earlier pages added to every user's excluded items; the cursor's item need
        not be in the user's list (it is only a position).  Returns (users, items, scores) shaped and padded like `recommend()`'s.
        A front end pages without rebuilding any exclusion list; `recommend_deep` chains the pages itself.
        ValueError — before any tower is computed — for a bad k, bad users, lengths that do not match the users, non-integer items,
        node ids that are neither -1 nor items of the trainset, a NaN score.  The route is `recommend()`'s: one
        amar_recommend_after_f32 launch where `recommend()` is fused, amar_topk_segmented_after_f32 over pair scores elsewhere."""
        n_users, n_items = _sizes(trainset)
        k = check_k(k)
        u = check_users(users, n_users)
        cursor = check_after(after, len(u), n_users, n_items)
        if len(u) == 0:
            return _empty(k)
        route = self._group_route(trainset, 'recommend')
        if route[0] == 'fused':
            return after_fused(route[1], route[2], trainset, k, users, exclude_seen, cursor)
        dev = route[2] or default_device()
        return pairs(route[1], trainset, k, users, exclude_seen, device=dev, after=_cursor_device(cursor, dev))

    def recommend_deep(self, trainset, k, users=None, exclude_seen=True):
        """The first k entries of every listed user's full ranking for k up to DEEP_K_MAX = 1024: Recall@100, a 200-item retrieval
        stage, a hand-over to another system (`recommend()` stops at K_MAX = 64, the length of one launch's list).  Returns (users
        int64 [m], items int64 [m, k] node ids, -1 padded, scores float32 [m, k], -inf padded) in `recommend()`'s order; the first
        min(k, K_MAX) columns are `recommend()`'s.  utilities.metrics.full_ranking_metrics scores lists of any length.
        Fused route: ceil(k / 64) launches — amar_recommend_f32, then amar_recommend_after_f32 from the previous page's last column,
        the cursors staying on the device; every page scores the catalogue again.  Pair route: every user chunk is scored once and
        amar_topk_segmented_after_f32 pages over the same scores.  The route is `recommend()`'s."""
        check_deep_k(k)
        check_users(users, len(trainset.users))
        route = self._group_route(trainset, 'recommend')
        if route[0] == 'fused':
            return deep_fused(route[1], route[2], trainset, k, users, exclude_seen)
        return deep_pairs(route[1], trainset, k, users, exclude_seen, device=route[2])

    def _group_route(self, trainset, kind='group'):
        """How the model ranks a catalogue for the fused kernel `kind` ('recommend' | 'group' | 'rank_of' | 'among' | 'lists': capi.RANK_KINDS):
        ('fused', (tu, ti, ...), plan) = the split towers and their plan where the head has one and that kernel takes it
        (capi.rank_fits: the kernels' LDS sums differ, so a head may rank fused in one and by pairs in another), or
        ('pairs', score_fn(u_ids, i_ids) -> [P, 1] scores, device)."""
        head = self._scoring_head()
        tables = self._recommend_tables(trainset)
        split = head._recommend_split(*tables, kind=kind) if hasattr(head, '_recommend_split') else None
        if split is not None:
            return 'fused', split, split[2]
        towers = head.towers(*tables)
        return 'pairs', lambda u, i: head.score_towers(towers, u, i), towers[0].device

    def _recommend_route(self, trainset):
        """'fused' or 'pairs': the route `recommend()` takes for this trainset (the tables of one pass give the towers' input width)."""
        head = self._scoring_head()
        if not hasattr(head, '_ranker_plan'):
            return 'pairs'
        d = self._recommend_tables(trainset)[0].shape[1]
        return 'fused' if head._ranker_plan(d, d, 'recommend')[0] is not None else 'pairs'

    def _propagated(self):
        """The node table of one hoisted propagation of a model with a `gnn`; the model's hoist state (`gnn.hoist`, `gnn._hoisted`,
        `_towers`) is left as it was found."""
        saved = (self.gnn.hoist, getattr(self.gnn, '_hoisted', None), self._towers)
        self.gnn.hoist = True
        try:
            return self.gnn(None)
        finally:
            self.gnn.hoist, self.gnn._hoisted, self._towers = saved

    def _embedding_tables(self, trainset, space):
        raise NotImplementedError

    def _resolve_space(self, space):
        spaces = tuple(self._embedding_spaces())
        if space is None:
            return spaces[0]
        if space not in spaces:
            raise ValueError("{} has no {!r} embedding space: it has {}".format(type(self).__name__, space, list(spaces)))
        return space

    def _entity_table(self, trainset, space, side):
        return self._embedding_tables(trainset, self._resolve_space(space))[side]

    def _user_embeddings(self, trainset, space=None):
        return self._entity_table(trainset, space, 0)

    def _item_embeddings(self, trainset, space=None):
        return self._entity_table(trainset, space, 1)

    def user_embeddings(self, trainset, space=None):
        """The learned user vectors, float32 [|U|, d]: space 'graph' (the propagated node table's user rows) or 'tower' (the output
        of the user's first-stage Dense network(s)); None = 'graph' where the model has a GNN, else 'tower'."""
        return self._user_embeddings(trainset, space).cpu().numpy().astype(np.float32)

    def item_embeddings(self, trainset, space=None):
        """The learned item vectors, float32 [|I|, d] (row r = item node |U| + r); spaces as in `user_embeddings`."""
        return self._item_embeddings(trainset, space).cpu().numpy().astype(np.float32)

    def similar_items(self, trainset, items=None, k=10, metric='cosine', space=None, exclude_self=True):
        """The k items most similar to every item of `items` (node ids |U|..|U|+|I|-1, all items by default, in the caller's order)
        in the model's `space`.  Returns (items int64 [m], neighbours int64 [m, k] (node ids, -1 padded), scores float32 [m, k]
        (-inf padded)): score descending, node id ascending on ties.  One amar_nearest_f32 call: no |I| x |I| matrix."""
        check_k(k)
        check_metric(metric)
        n_users, n_items = _sizes(trainset)
        ids = check_ids(items, n_users, n_users + n_items, 'items')
        nb, sc = similar_rows(self._item_embeddings(trainset, space), ids - n_users, k, metric, exclude_self, n_users)
        return ids, nb, sc

    def similar_users(self, trainset, users=None, k=10, metric='cosine', space=None, exclude_self=True):
        """`similar_items` over the user rows: ids 0..|U|-1."""
        check_k(k)
        check_metric(metric)
        n_users, _ = _sizes(trainset)
        ids = check_ids(users, 0, n_users, 'users')
        nb, sc = similar_rows(self._user_embeddings(trainset, space), ids, k, metric, exclude_self, 0)
        return ids, nb, sc

    def recommend_like(self, trainset, liked, k=10, metric='cosine', space=None, exclude_liked=True):
        """The k items most similar to each PROFILE of `liked` (a list of lists of item node ids — a user given only by what they
        liked, with no row in the graph): the query is the float32 mean of the liked items' vectors.  The profile's own items are
        left out unless exclude_liked=False.  Returns (neighbours int64 [m, k] (node ids, -1 padded), scores float32 [m, k])."""
        k = check_k(k)
        check_metric(metric)
        n_users, n_items = _sizes(trainset)
        rows = []
        for j, profile in enumerate(liked):
            ids = check_ids(profile, n_users, n_users + n_items, 'liked items')
            if ids.size == 0:
                raise ValueError("profile {} is empty: recommend_like needs at least one liked item per profile".format(j))
            rows.append(ids - n_users)
        if not rows:
            return np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32)
        table = self._item_embeddings(trainset, space)
        nb, sc = nearest(profile_queries(table, rows), table, k, metric, exclude=rows if exclude_liked else None)
        if _ON_DEVICE:
            return nb, sc
        return np.where(nb >= 0, nb + n_users, -1), sc

    # -- diversified lists (amar_rerank_mmr_f32, amar_list_diversity_f64) ----------------------------------------------
    def recommend_diverse(self, trainset, k=10, pool=50, trade_off=0.7, metric='cosine', space=None, users=None, exclude_seen=True):
        """Diversified top-k: the `pool` best items of every user (`recommend(k=pool)`, kept on the device) re-ranked by Maximal
        Marginal Relevance over the item vectors of the model's `space` (`rerank_mmr`: trade_off = 1 is `recommend(k)` itself,
        smaller values weigh dissimilarity to the items already chosen more).  Returns (users int64 [m], items int64 [m, k] node ids
        in SELECTION order (-1 padded), scores float32 [m, k]: the model's own scores of the chosen items (-inf padded)); inside
        ``device_lists()`` the device tensors (item rows int32)."""
        k = check_k(k)
        check_metric(metric)
        trade_off = check_trade_off(trade_off)
        if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)) or not k <= int(pool) <= K_MAX:
            raise ValueError("pool must be an integer in [k = {}, {}] (got {!r})".format(k, K_MAX, pool))
        n_users, _ = _sizes(trainset)
        table = self._item_embeddings(trainset, space)
        check_width(table.shape[1], 'item vectors')
        with device_lists():
            u, items, scores = self.recommend(trainset, k=int(pool), users=users, exclude_seen=exclude_seen)
        if len(u) == 0:
            return _empty(k)
        items, scores = rerank_mmr(items, scores, table, k, trade_off=trade_off, metric=metric)
        return _finish(u, items, scores, n_users)

    def list_diversity(self, trainset, items, ks=None, metric='cosine', space=None):
        """Intra-list diversity of lists of items in the model's `space`: `items` [m, K] node ids (host, -1 padded: what `recommend`
        returns) or, inside ``device_lists()``, int32 item rows on the device; `ks` the cutoffs (K alone by default).  Returns
        (ild float64 [m, nk]: the mean of 1 - sim over the pairs of items in the first ks[q] ranks, 0 below two items;
        count int32 [m, nk]: the items in those ranks) — host arrays, device tensors inside ``device_lists()``."""
        check_metric(metric)
        n_users, n_items = _sizes(trainset)
        table = self._item_embeddings(trainset, space)
        check_width(table.shape[1], 'item vectors')
        if isinstance(items, torch.Tensor) and items.is_cuda:
            lists = items.to(torch.int32)
        else:
            lists = _item_rows_device(items, n_users, n_items, table.device)
        if lists.dim() != 2:
            raise ValueError("items must be a 2-D [m, K] array")
        ks, _ = capi.rank_metrics_args(int(lists.shape[1]), [int(lists.shape[1])] if ks is None else ks)
        ild, count = capi.list_diversity(lists.contiguous(), _as_device_matrix(table, table.device, 'table'), ks, metric=metric)
        if _ON_DEVICE:
            return ild, count
        return ild.cpu().numpy(), count.cpu().numpy()

    # -- calibrated lists (amar_rerank_calibrated_f32, amar_list_calibration_f64) -----------------------------------------
    def recommend_calibrated(self, trainset, k=10, pool=50, trade_off=0.5, smoothing=0.01, categories=None, users=None, exclude_seen=True):
        """Calibrated top-k (Steck 2018): the `pool` best items of every user (`recommend(k=pool)`, kept on the device) re-ranked so
        that the list's categories follow the categories of what the user liked in training (`rerank_calibrated`: trade_off = 1 is
        `recommend(k)` itself, smaller values weigh the proportion more; `categories` as in `item_category_csr`).  A user without a
        liked item that has a category keeps the score order.  Returns (users int64 [m], items int64 [m, k] node ids in SELECTION
        order (-1 padded), scores float32 [m, k]: the model's own scores of the chosen items (-inf padded)); inside
        ``device_lists()`` the device tensors (item rows int32)."""
        k = check_k(k)
        trade_off, smoothing, pool = check_trade_off(trade_off), check_smoothing(smoothing), check_pool(pool, k)
        n_users, n_items = _sizes(trainset)
        cats = _cats_device(trainset, n_items, categories)
        with device_lists():
            u, items, scores = self.recommend(trainset, k=pool, users=users, exclude_seen=exclude_seen)
        if len(u) == 0:
            return _empty(k)
        u_dev = None if users is None else torch.from_numpy(u.astype(np.int32)).to(items.device)
        items, scores = rerank_calibrated(items, scores, u_dev, _liked_device(trainset, n_users, n_items), cats, k,
                                          trade_off=trade_off, smoothing=smoothing)
        return _finish(u, items, scores, n_users)

    def list_calibration(self, trainset, items, users=None, ks=None, smoothing=0.01, categories=None):
        """Miscalibration of lists of items against their users' liked training items: `items` [m, K] node ids (host, -1 padded: what
        `recommend` returns) or, inside ``device_lists()``, int32 item rows on the device, one row per user of `users` (all users by
        default); `ks` the cutoffs (K alone by default).  Returns (kl float64 [m, nk]: C(p, the first ks[q] ranks), 0 for a user
        without a target; count int32 [m, nk]: the items with a category in those ranks; support int32 [m]: the user's liked items
        with a category) — host arrays, device tensors inside ``device_lists()``."""
        smoothing = check_smoothing(smoothing)
        n_users, n_items = _sizes(trainset)
        u = check_users(users, n_users)
        cats = _cats_device(trainset, n_items, categories)
        if isinstance(items, torch.Tensor) and items.is_cuda:
            lists = items.to(torch.int32)
        else:
            lists = _item_rows_device(items, n_users, n_items, default_device())
        if lists.dim() != 2 or int(lists.shape[0]) != len(u):
            raise ValueError("items must be a 2-D [m, K] array with one row per user ({} rows for {} users)".format(int(lists.shape[0]), len(u)))
        ks, _ = capi.rank_metrics_args(int(lists.shape[1]), [int(lists.shape[1])] if ks is None else ks)
        u_dev = None if users is None else torch.from_numpy(u.astype(np.int32)).to(lists.device)
        liked = _liked_device(trainset, n_users, n_items)
        out = capi.list_calibration(lists.contiguous(), liked[0], liked[1], cats[0], cats[1], cats[2], ks, smoothing=smoothing, users=u_dev)
        if _ON_DEVICE:
            return out
        return tuple(t.cpu().numpy() for t in out)

    # -- explanations (amar_explain_f32) --------------------------------------------------------------------------------
    def explain(self, trainset, users=None, items=None, k=10, n_evidence=3, n_properties=3, metric='cosine', space=None,
                property_weight='idf', exclude_seen=True):
        """Why these items for these users, in the model's item `space`.  items=None explains `recommend(k)` (the lists stay on the
        device between the two launches); otherwise `items` is an [m, K] array of item node ids (-1 padded) for `users`.  For every
        (user, item): the `n_evidence` liked training items of the user most similar to the item (similarity descending, node id
        ascending on ties, never the item itself), and the `n_properties` properties the item shares with other liked items,
        by score w_p * sum max(sim, 0) over those items (w_p = log(|I| / df_p) for property_weight='idf', 1 for 'none'), with
        their support (how many liked items have the property).  Returns a dict of host arrays: users int64 [m], items int64 [m, K]
        node ids, evidence int64 [m, K, n_evidence] node ids (-1 padded), evidence_sim float32 (-inf padded), properties int64
        [m, K, n_properties] property indices (-1 padded), property_score float32 (-inf padded), property_support int32 (0 padded);
        the three property arrays have a last dimension of 0 for a trainset without properties.  Inside ``device_lists()`` the
        device tensors (item rows int32)."""
        check_metric(metric)
        E = check_count(n_evidence, 1, capi.EXPLAIN_MAX_E, 'n_evidence')
        Q = check_count(n_properties, 0, capi.EXPLAIN_MAX_E, 'n_properties')
        if property_weight not in ('idf', 'none'):
            raise ValueError("property_weight must be 'idf' or 'none' (got {!r})".format(property_weight))
        n_users, n_items = _sizes(trainset)
        if items is None:
            k = check_k(k)
        table = self._item_embeddings(trainset, space)
        check_width(table.shape[1], 'item vectors')
        if items is None:
            with device_lists():
                u, lists, _ = self.recommend(trainset, k=k, users=users, exclude_seen=exclude_seen)
            if len(u) == 0:
                lists = torch.zeros((0, k), dtype=torch.int32, device=table.device)
        else:
            u = check_users(users, n_users)
            lists = _item_rows_device(items, n_users, n_items, table.device, rows=len(u), widths=(1, K_MAX))
        u_dev = None if users is None else torch.from_numpy(u.astype(np.int32)).to(table.device)
        out = explain_lists(lists.contiguous(), u_dev, _liked_device(trainset, n_users, n_items), table,
                            _props_device(trainset, n_items, property_weight), E, Q, metric)
        if _ON_DEVICE:
            return dict(zip(EXPLAIN_KEYS, (u, lists) + out))
        rows = lambda t: (lambda x: np.where(x >= 0, x + n_users, -1))(t.cpu().numpy().astype(np.int64))
        ev, sim, pr, ps, pc = out
        return dict(zip(EXPLAIN_KEYS, (u, rows(lists), rows(ev), sim.cpu().numpy(), pr.cpu().numpy().astype(np.int64), ps.cpu().numpy(),
                                       pc.cpu().numpy())))

    # -- exact positions (amar_rank_of_f32) ---------------------------------------------------------------------------------
    def rank_items(self, trainset, users, items, exclude_seen=True):
        """Where every (users[p], items[p]) pair stands in the user's full ranking: `users` user indices 0..|U|-1 and `items` item
        node ids |U|..|U|+|I|-1, parallel arrays.  The candidates of a user are all items of `trainset` outside its training row
        (all items with exclude_seen=False).  Returns a dict of host arrays, one value per pair: 'rank' int64 (1-based: the position
        `recommend()` with an unbounded k would list the item at — score descending, node id ascending on ties; 0 = "seen": the item
        is in the user's training row), 'score' float32 (the model's score, filled for seen items too), 'ties' int64 (the other
        candidates with exactly that score), 'candidates' int64 (the user's |C(u)|) and 'percentile' float64
        (1 - (rank - 1) / candidates: 1 for the best item; NaN for a seen one).  Heads with a fused ranking kernel run one
        amar_rank_of_f32 launch (nothing of size |U| x |I| in memory); the others compare pair-route scores per user chunk."""
        n_users, n_items = _sizes(trainset)
        if users is None or items is None:
            raise ValueError("rank_items needs `users` and `items`: parallel arrays of user indices and item node ids")
        u = check_users(users, n_users)
        it = check_ids(items, n_users, n_users + n_items, 'items')
        if len(u) != len(it):
            raise ValueError("users and items must be parallel arrays ({} users, {} items)".format(len(u), len(it)))
        if len(u) == 0:
            return {'rank': np.zeros(0, dtype=np.int64), 'score': np.zeros(0, dtype=np.float32), 'ties': np.zeros(0, dtype=np.int64),
                    'candidates': np.zeros(0, dtype=np.int64), 'percentile': np.zeros(0, dtype=np.float64)}
        pair, inverse = np.unique(u * n_items + (it - n_users), return_inverse=True)        # by user, then item row: the entries
        uu, rows = pair // n_items, pair % n_items
        entry_users, counts = np.unique(uu, return_counts=True)
        ptr = np.zeros(len(entry_users) + 1, dtype=np.int64)
        np.cumsum(counts, out=ptr[1:])
        score, greater, before, after = (t.cpu().numpy() for t in rank_of_route(self, trainset, entry_users, (ptr, rows), exclude_seen))
        candidates = np.full(len(pair), n_items, dtype=np.int64)
        seen = np.zeros(len(pair), dtype=bool)
        excl = _exclusion_device(trainset, n_users, n_items, exclude_seen)
        if excl is not None:
            e_ptr, e_items = excl[0].cpu().numpy().astype(np.int64), excl[1].cpu().numpy().astype(np.int64)
            candidates -= np.diff(e_ptr)[uu]
            seen = np.isin(pair, np.repeat(np.arange(n_users, dtype=np.int64), np.diff(e_ptr)) * n_items + e_items)
        rank = np.where(seen, 0, 1 + greater.astype(np.int64) + before.astype(np.int64))
        with np.errstate(divide='ignore', invalid='ignore'):
            percentile = np.where(seen, np.nan, 1.0 - (rank - 1).astype(np.float64) / candidates.astype(np.float64))
        out = (rank, score.astype(np.float32), before.astype(np.int64) + after.astype(np.int64), candidates, percentile)
        inverse = inverse.reshape(-1)
        return {key: value[inverse] for key, value in zip(RANK_ITEMS_KEYS, out)}

    # -- candidates (amar_recommend_among_f32) ------------------------------------------------------------------------------
    def recommend_among(self, trainset, candidates, k=10, users=None, exclude_seen=True):
        """The k best items of every user in `users` (user indices, all users by default) among `candidates` only: one genre, what
        is in stock, a shelf, the output of a retrieval stage.  `candidates` (`check_candidates`): item node ids |U|..|U|+|I|-1 in
        any order, a boolean mask over the items, or one such sequence per listed user (`items_with_properties` builds sets from the
        graph's properties).  Training pairs are excluded unless exclude_seen=False.  Returns (users int64 [m], items int64 [m, k]
        node ids, -1 padded, scores float32 [m, k], -inf padded), shaped and ordered like `recommend()`: exactly the user's full
        ranking with everything outside the candidates struck out.
        One candidate set for every user and a head with a fused ranking kernel: one amar_recommend_among_f32 launch over
        |U| x |C| pairs (nothing of that size in memory).  Everything else — a head that kernel does not take, the hybrids,
        per-user candidates — is ranked by the pair route over the kept pairs; nothing raises."""
        n_users, n_items = _sizes(trainset)
        k = check_k(k)
        u = check_users(users, n_users)
        cand = check_candidates(candidates, n_users, n_items, n_listed=len(u))
        if len(u) == 0:
            return _empty(k)
        if isinstance(cand, tuple):                                       # per-user candidates: the model's pair route
            return self._recommend_pairs(trainset, k, users, exclude_seen, keep_items=cand)
        route = self._group_route(trainset, kind='among')
        if route[0] == 'fused':
            return among_fused(route[1], route[2], trainset, cand, k, users, exclude_seen)
        return pairs(route[1], trainset, k, users, exclude_seen, device=route[2], keep_items=cand)

    # -- per-user candidate lists (amar_recommend_lists_f32) ------------------------------------------------------------------
    def recommend_from(self, trainset, candidates, k=10, users=None, exclude_seen=True):
        """The k best items of every user in `users` (user indices, all users by default) among THAT USER's candidates: a retrieval
        stage's output to re-rank, per-user availability, a "similar to what you liked" pool, a held-out item against sampled
        negatives.  `candidates` (`check_candidate_lists`): one sequence of item node ids |U|..|U|+|I|-1 per listed user, or a 2-D
        integer array / tensor [m, P] of node ids padded with -1 — the shape `recommend()`, `similar_items()` and `device_lists()`
        hand out; any order, duplicates collapse.  Training pairs are excluded unless exclude_seen=False.  Returns (users int64 [m],
        items int64 [m, k] node ids, -1 padded, scores float32 [m, k], -inf padded), shaped and ordered like `recommend()`: exactly
        the user's full ranking with everything outside its own list struck out — on the fused route bit for bit.
        A head with a fused ranking kernel: one amar_recommend_lists_f32 launch over sum |C_u| pairs, nothing of size |U| x |I| built
        anywhere; a device tensor is sorted, de-duplicated and compacted on the device without a host round trip (an entry that is
        no item node id counts as padding there).  The kernel keeps no item tile in LDS, so it also takes heads `recommend()` has no
        room for.  The hybrids and heads past its capacity rank the kept pairs on the pair route; nothing raises.  One set for all
        users is `recommend_among`'s case."""
        n_users, n_items = _sizes(trainset)
        k = check_k(k)
        u = check_users(users, n_users)
        lists = check_candidate_lists(candidates, n_users, n_items, len(u))
        if len(u) == 0:
            return _empty(k)
        route = self._group_route(trainset, kind='lists')
        if route[0] == 'fused':
            return lists_fused(route[1], route[2], trainset, lists, k, users, exclude_seen)
        if isinstance(lists, torch.Tensor):                               # the pair route reads its candidates on the host
            lists = check_candidate_lists(lists.cpu(), n_users, n_items, len(u))
        return pairs(route[1], trainset, k, users, exclude_seen, device=route[2], keep_items=lists)

    def evaluate_ranking_sampled(self, trainset, test_ratings, ks, n_negatives=99, seed=0, users=None):
        """Precision / Recall / NDCG / HitRate @k under the 1 + N sampled-negatives protocol (recommend.evaluate_ranking_sampled):
        every user's held-out positives ranked against `n_negatives` unrated items drawn from `seed` and the user alone."""
        return evaluate_ranking_sampled(self, trainset, test_ratings, ks, n_negatives=n_negatives, seed=seed, users=users)

    # -- group recommendation (amar_recommend_group_f32) ----------------------------------------------------------------
    def recommend_group(self, trainset, groups, k=10, strategy='mean', min_score=None, exclude_seen=True, member_scores=False):
        """The k best items for every GROUP of `groups` (a sequence of sequences of user indices 0..|U|-1; the order of the members
        does not matter, empty groups are allowed) among all items of `trainset`: every member's score of every item, combined by
        `strategy` — 'mean' (average: the scores added in ascending member order, divided by the group size), 'min' (least misery)
        or 'max' (most pleasure) — in float32; an item that any member scores below `min_score` is dropped (None: no veto), and so is,
        unless exclude_seen=False, every training item of any member.  Heads with a fused ranking kernel run one
        amar_recommend_group_f32 launch (nothing of size members x |I| in memory); the others aggregate pair-route scores.
        Returns (items int64 [g, k] node ids, -1 padded; scores float32 [g, k], -inf padded): aggregate descending, node id ascending
        on ties.  member_scores=True adds a list of g float32 arrays [n_members_j, k]: each member's own score of each chosen item
        (members in ascending order; NaN where the list is padded), with the bits that went into the aggregate: from the ranking
        kernel on the fused route (`fused_member_scores`), from one pair-scoring call over the (member, chosen item) pairs on the
        pair route."""
        k, strategy, floor = check_k(k), check_strategy(strategy), check_min_score(min_score)
        n_users, n_items = _sizes(trainset)
        ptr, members = group_csr(groups, n_users)
        g = len(ptr) - 1
        if g == 0:
            out = (np.zeros((0, k), dtype=np.int64), np.zeros((0, k), dtype=np.float32))
            return out + ([],) if member_scores else out
        excl = group_exclusion_csr(trainset.ratings, ptr, members, n_users, n_items) if exclude_seen else None
        route = self._group_route(trainset)
        if route[0] == 'fused':
            towers, plan = route[1], route[2]
            score_fn = None
            rows, scores = group_fused(towers, plan, ptr, members, excl, k, strategy, floor)
        else:
            score_fn, dev = route[1], route[2] or default_device()
            rows, scores = group_pairs(score_fn, n_items, ptr, members, excl, k, strategy, floor, dev)
        rows = rows.cpu().numpy().astype(np.int64)
        out = (np.where(rows >= 0, rows + n_users, -1), scores.cpu().numpy().astype(np.float32))
        if not member_scores:
            return out
        sizes = np.diff(ptr.astype(np.int64))
        valid = rows >= 0                                                # [g, k]
        per = [np.full((int(sizes[j]), k), np.nan, dtype=np.float32) for j in range(g)]
        if score_fn is None:
            fused_member_scores(towers, plan, ptr, members, rows, per)
            return out + (per,)
        u_ids = np.concatenate([np.repeat(members[ptr[j]:ptr[j + 1]], int(valid[j].sum())) for j in range(g)])
        i_ids = np.concatenate([np.tile(rows[j][valid[j]], int(sizes[j])) for j in range(g)])
        if u_ids.size:
            s = score_fn(_i32_device(u_ids, dev), _i32_device(i_ids, dev)).reshape(-1).cpu().numpy().astype(np.float32)
            at = 0
            for j in range(g):
                n_j, v_j = int(sizes[j]), int(valid[j].sum())
                per[j][:, valid[j]] = s[at:at + n_j * v_j].reshape(n_j, v_j)
                at += n_j * v_j
        return out + (per,)
