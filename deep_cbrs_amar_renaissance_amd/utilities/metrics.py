"""Ranking step after the scoring head — mirrors `/root/reference/src/utilities/metrics.py:11-80`.

``top_k_predictions`` keeps, for every user, the k best-scored items among THAT USER'S test
pairs (`metrics.py:11-34`), on the GPU (`amar_topk_segmented_f32`: one wavefront per user).
Ordering is (user ascending, score descending); equal scores — left to pandas' sort in the reference
(`metrics.py:27`: whatever order `sort_values` leaves a tie in) — break on item id ascending here.  The reference's own
function, run on committed inputs, gives the same rows in the same order (tests/golden/topk_reference.npz).

``top_k_metrics`` in the reference shells out to ``java -jar binaries/mimir.jar`` (RiVal
Precision/Recall, `metrics.py:60-65`); no JVM exists where this runs, so the holdout
Precision/Recall/F1@k is restated on the host from RiVal's ranking-metric semantics
(``precision_recall_f1_at_k``: hand-computed vectors in tests/test_metrics_cpu.py; the choices the
jar's behaviour cannot settle here are explicit switches) and writes the same ``results.tsv``
(label, P, R, F1 — `experiment.py:211-213` reads columns 1..3).

The metrics of ``Model.compile(metrics=...)`` live here too: `resolve_metrics` names the ones the training kernel counts
(include/amar_hip.h: amar_loss_grad_f32's counter block), `metric_counters` restates that block in numpy and `metric_values` turns
either into Keras' accuracy / Precision / Recall / AUC.
"""
import logging
import os

import numpy as np
import pandas as pd
import torch

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd.engine import default_device

logging.basicConfig(format="%(message)s", level=logging.INFO)
logger = logging.getLogger(__name__)


def top_k_arrays(u_idx, i_idx, scores, k):
    """Per-user top-k on the device. Returns (user index [n], item index [n, k] (-1 padded), score [n, k])."""
    u_idx = np.asarray(u_idx, dtype=np.int64)
    i_idx = np.asarray(i_idx, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    order = np.argsort(u_idx, kind='stable')
    seg_users, counts = np.unique(u_idx[order], return_counts=True)
    seg_ptr = np.zeros(len(seg_users) + 1, dtype=np.int64)
    np.cumsum(counts, out=seg_ptr[1:])
    dev = default_device()
    items_dev = torch.from_numpy(i_idx[order].astype(np.int32)).to(dev)
    scores_dev = torch.from_numpy(scores[order]).to(dev)
    seg_dev = torch.from_numpy(seg_ptr.astype(np.int32)).to(dev)
    out_items, out_scores = capi.topk_segmented(seg_dev, items_dev, scores_dev, int(k))
    return seg_users, out_items.cpu().numpy(), out_scores.cpu().numpy()


def top_k_predictions(predictions, users, items, k=5):
    """
    Top-K suggested items for each user.

    :param predictions: [P, 3] array (user index, item index (offset by |U|), score).
    :param users: original user identifiers.
    :param items: original item identifiers.
    :param k: the K parameter.
    :return: DataFrame (users, items, scores) with the original identifiers, k rows per user at most.
    """
    seg_users, top_items, top_scores = top_k_arrays(predictions[:, 0], predictions[:, 1], predictions[:, 2], k)
    valid = top_items >= 0
    df = pd.DataFrame()
    df['users'] = np.asarray(users)[np.repeat(seg_users, k).reshape(-1, k)[valid]]
    df['items'] = np.asarray(items)[top_items[valid] - len(users)]
    df['scores'] = top_scores[valid].astype(np.float64)
    return df


def recommendations_frame(users, items, scores, user_ids, item_ids):
    """`recommend()`'s output (user indices [m], node ids [m, k] (-1 padded), scores [m, k]) as the (users, items, scores) DataFrame
    of `top_k_predictions`: original identifiers, each user's rows best first, padding dropped."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    items = np.asarray(items, dtype=np.int64).reshape(len(users), -1)
    scores = np.asarray(scores, dtype=np.float32).reshape(items.shape)
    valid = items >= 0
    df = pd.DataFrame()
    df['users'] = np.asarray(user_ids)[np.repeat(users, items.shape[1]).reshape(items.shape)[valid]]
    df['items'] = np.asarray(item_ids)[items[valid] - len(user_ids)]
    df['scores'] = scores[valid].astype(np.float64)
    return df


def explanations_frame(explained, user_ids, item_ids, prop_ids=None):
    """`model.explain()`'s dict as a DataFrame with one row per (user, item, rank): original user and item identifiers, the rank
    (1 = best), and — padding dropped, best first, joined by spaces — the evidence items with their similarities and the shared
    properties (original identifiers from `prop_ids`, property indices without it) with their scores and supports."""
    users = np.asarray(explained['users'], dtype=np.int64).reshape(-1)
    items = np.asarray(explained['items'], dtype=np.int64).reshape(len(users), -1)
    item_ids, n_users = np.asarray(item_ids), len(user_ids)
    join = lambda values: ' '.join(str(v) for v in values)
    rows = []
    for j, u in enumerate(users):
        for t, i in enumerate(items[j]):
            if i < 0:
                continue
            ev = np.asarray(explained['evidence'][j, t])
            pr = np.asarray(explained['properties'][j, t])
            keep_e, keep_p = ev >= 0, pr >= 0
            props = pr[keep_p] if prop_ids is None else np.asarray(prop_ids)[pr[keep_p]]
            rows.append((np.asarray(user_ids)[u], item_ids[i - n_users], t + 1, join(item_ids[ev[keep_e] - n_users]),
                         join(np.asarray(explained['evidence_sim'][j, t])[keep_e]), join(props),
                         join(np.asarray(explained['property_score'][j, t])[keep_p]),
                         join(np.asarray(explained['property_support'][j, t])[keep_p])))
    return pd.DataFrame(rows, columns=['users', 'items', 'rank', 'evidence', 'evidence_sim', 'properties', 'property_score',
                                       'property_support'])


def full_ranking_metrics(users, items, test_ratings, ks):
    """Full-ranking evaluation of `recommend()`'s lists (users [m], node ids [m, K] best first, -1 padded) against the test
    ratings ([P, 3]: user index, item node id, label): for every k in `ks` (<= K) the means over the users of `users` that have at
    least one relevant test item (label 1) of
        Precision@k = hits / k,  Recall@k = hits / |relevant|,  HitRate@k = [hits > 0],
        NDCG@k = sum_{hit at rank r <= k} 1 / log2(r + 1)  /  sum_{r <= min(|relevant|, k)} 1 / log2(r + 1)
    A list shorter than k counts its missing ranks as misses.  Returns {'precision_at_<k>', 'recall_at_<k>', 'ndcg_at_<k>',
    'hit_at_<k>' for each k, 'users_evaluated', 'users_skipped'} (users without a relevant test item are skipped and counted)."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    items = np.asarray(items, dtype=np.int64).reshape(len(users), -1)
    ks = [int(k) for k in ks]
    if any(k < 1 or k > items.shape[1] for k in ks):
        raise ValueError("every k must lie in [1, {}] (the length of the lists)".format(items.shape[1]))
    t = np.asarray(test_ratings)
    relevant = {}
    if len(t):
        liked = t[t[:, 2] == 1]
        for u, i in zip(liked[:, 0].astype(np.int64).tolist(), liked[:, 1].astype(np.int64).tolist()):
            relevant.setdefault(u, set()).add(i)
    disc = 1.0 / np.log2(np.arange(items.shape[1]) + 2.0)
    sums = {k: np.zeros(4) for k in ks}
    evaluated = skipped = 0
    for row, u in enumerate(users.tolist()):
        rel = relevant.get(u)
        if not rel:
            skipped += 1
            continue
        evaluated += 1
        hit = np.array([i in rel for i in items[row].tolist()], dtype=np.float64)
        for k in ks:
            h = hit[:k].sum()
            idcg = disc[:min(len(rel), k)].sum()
            sums[k] += (h / k, h / len(rel), float((hit[:k] * disc[:k]).sum() / idcg), float(h > 0))
    out = {}
    for k in ks:
        mean = sums[k] / evaluated if evaluated else sums[k]
        out.update({'precision_at_{}'.format(k): float(mean[0]), 'recall_at_{}'.format(k): float(mean[1]),
                    'ndcg_at_{}'.format(k): float(mean[2]), 'hit_at_{}'.format(k): float(mean[3])})
    out['users_evaluated'], out['users_skipped'] = evaluated, skipped
    return out


RANK_METRICS = ('auc', 'mrr', 'map')


def check_rank_metrics(names):
    """The cut-off-free measures asked for, as a tuple in the order given, each once: a subset of RANK_METRICS; ValueError otherwise."""
    if isinstance(names, str) or not hasattr(names, '__iter__'):
        raise ValueError("rank_metrics must be a sequence of names out of {} (got {!r})".format(RANK_METRICS, names))
    out = []
    for name in names:
        if not isinstance(name, str) or name not in RANK_METRICS:
            raise ValueError("unknown rank metric {!r}; supported: {}".format(name, ', '.join(RANK_METRICS)))
        if name not in out:
            out.append(name)
    if not out:
        raise ValueError("rank_metrics names no metric; supported: {}".format(', '.join(RANK_METRICS)))
    return tuple(out)


def full_ranking_rank_metrics(scores_by_user, relevant, excluded=None, per_user=False):
    """AUC, MRR and MAP of full rankings on the host, in float64, from dense score rows: what amar_rank_of_f32 +
    amar_rank_of_metrics_f64 compute on the device without the rows (include/amar_hip.h has the same formulas).
    `scores_by_user` [n, |I|]: row v holds user v's score of every item row (compared as float32); `relevant[v]` / `excluded[v]`: the
    item rows that are relevant / excluded for the user (any iterable; excluded=None: nothing is).  Per user, with
    C = {items} minus excluded, the targets R' = relevant minus excluded in ascending item row, R = |R'|, N_neg = |C| - R, and for t in R'
        greater_t = #{i in C, i != t : s_i > s_t},  eq_before_t / eq_after_t = #{i in C, i != t : s_i == s_t, i < t / i > t},
        r_t = 1 + greater_t + eq_before_t   (the position recommend() with an unbounded k would list t at),
        h_t = #{t' in R' : r_t' <= r_t}:
        rr = 1 / min_t r_t,   ap = (1 / R) sum_t h_t / r_t   (terms added in target order),
        auc = 1 - [sum_t (neg_greater_t + neg_equal_t / 2)] / (R N_neg),
    neg_greater_t = greater_t - #{t' != t : s_t' > s_t} and neg_equal_t = eq_before_t + eq_after_t - #{t' != t : s_t' == s_t}: the
    Mann-Whitney statistic with ties at 1/2, which does not depend on the numbering of the items (rr and ap do, through r_t, when
    scores tie).  A user with R = 0 or N_neg = 0 is skipped and counted.  Returns {'auc', 'mrr', 'map': the float64 means over the
    evaluated users (0 when there is none), 'rank_metrics_users': (evaluated, skipped)}; per_user=True returns instead
    (values float64 [n, 3] in the order auc, rr, ap — zeros for a skipped user —, valid bool [n])."""
    S = np.asarray(scores_by_user, dtype=np.float32)
    if S.ndim != 2 or len(relevant) != len(S) or (excluded is not None and len(excluded) != len(S)):
        raise ValueError("scores_by_user must be [n, items] with one relevant (and one excluded) collection per row")
    n, n_items = S.shape
    values, valid = np.zeros((n, 3), dtype=np.float64), np.zeros(n, dtype=bool)
    for v in range(n):
        cand = np.ones(n_items, dtype=bool)
        if excluded is not None:
            cand[np.asarray(sorted(excluded[v]), dtype=np.int64)] = False
        rel = np.asarray(sorted(set(int(i) for i in relevant[v])), dtype=np.int64)
        if rel.size and (rel[0] < 0 or rel[-1] >= n_items):
            raise ValueError("relevant items must be item rows in [0, {})".format(n_items))
        targets = rel[cand[rel]] if rel.size else rel
        R, n_neg = len(targets), int(cand.sum()) - len(targets)
        if R == 0 or n_neg <= 0:
            continue
        s, rows = S[v], np.arange(n_items)
        greater = np.array([int((cand & (s > s[t])).sum()) for t in targets], dtype=np.int64)
        before = np.array([int((cand & (s == s[t]) & (rows < t)).sum()) for t in targets], dtype=np.int64)
        after = np.array([int((cand & (s == s[t]) & (rows > t)).sum()) for t in targets], dtype=np.int64)
        st = s[targets]
        r = 1 + greater + before
        h = (r[None, :] <= r[:, None]).sum(axis=1)
        neg_greater = greater - (st[None, :] > st[:, None]).sum(axis=1)
        neg_equal = before + after - ((st[None, :] == st[:, None]).sum(axis=1) - 1)
        ap = 0.0
        for term in (h.astype(np.float64) / r.astype(np.float64)).tolist():
            ap += term
        values[v] = (1.0 - float((neg_greater + 0.5 * neg_equal).sum()) / (float(R) * float(n_neg)), 1.0 / float(r.min()), ap / float(R))
        valid[v] = True
    if per_user:
        return values, valid
    mean = values[valid].mean(axis=0) if valid.any() else np.zeros(3)
    return {'auc': float(mean[0]), 'mrr': float(mean[1]), 'map': float(mean[2]), 'rank_metrics_users': (int(valid.sum()), int(n - valid.sum()))}


def intra_list_diversity(lists, vectors, ks=None, metric='cosine'):
    """Intra-list diversity on the host, in float64 (what amar_list_diversity_f64 computes on the device): `lists` [m, K] ROWS of
    `vectors` [n, d], -1 padded; for every cutoff k of `ks` (K alone by default) the mean over the pairs a < b of valid items in the
    first k ranks of 1 - sim(a, b), sim the dot product or the cosine (0 against a zero vector); 0 below two items.  Returns
    (ild float64 [m, nk], count int64 [m, nk])."""
    if metric not in ('dot', 'cosine'):
        raise ValueError("metric must be 'dot' or 'cosine' (got {!r})".format(metric))
    lists = np.asarray(lists, dtype=np.int64)
    if lists.ndim != 2:
        raise ValueError("lists must be a 2-D [m, K] array")
    x = np.asarray(vectors, dtype=np.float64)
    ks = [int(lists.shape[1])] if ks is None else [int(k) for k in ks]
    if any(k < 1 or k > lists.shape[1] for k in ks):
        raise ValueError("every k must lie in [1, {}] (the length of the lists)".format(lists.shape[1]))
    if metric == 'cosine':
        sq = (x * x).sum(axis=1)
        x = x * np.where(sq > 0, 1.0 / np.sqrt(np.where(sq > 0, sq, 1.0)), 0.0)[:, None]
    ild = np.zeros((len(lists), len(ks)), dtype=np.float64)
    count = np.zeros((len(lists), len(ks)), dtype=np.int64)
    for j, row in enumerate(lists):
        for q, k in enumerate(ks):
            head = row[:k][row[:k] >= 0]
            count[j, q] = n = len(head)
            if n >= 2:
                gram = x[head] @ x[head].T
                ild[j, q] = (1.0 - gram[np.triu_indices(n, 1)]).mean()
    return ild, count


def miscalibration(lists, users, liked, cats, ks=None, smoothing=0.01):
    """Miscalibration (Steck 2018) on the host, in float64 (what amar_list_calibration_f64 computes on the device): `lists` [m, K]
    item ROWS, -1 padded, row j belonging to users[j] (None: user j); `liked` = (ptr, items), the liked items as a CSR over users
    (recommend.liked_csr); `cats` = (ptr, ids, ...), the categories as a CSR over item rows (recommend.item_category_csr).  With
    p(g) = the mean over the user's liked items that have a category of 1/len_i on the categories of item i, and q(g) the same mean
    over the items with a category in the first k ranks (0 when there is none),
        C = sum over p(g) > 0, g ascending, of p(g) log(p(g) / ((1 - a) q(g) + a p(g))),    a = smoothing as a float32 (the C ABI's),
    for every cutoff k of `ks` (K alone by default); 0 for a user without a liked item that has a category.  The sums run liked item
    ascending, rank ascending and g ascending.  Returns (kl float64 [m, nk], count int64 [m, nk]: the items with a category in the
    first k ranks, support int64 [m]: the user's liked items with a category)."""
    lists = np.asarray(lists, dtype=np.int64)
    if lists.ndim != 2:
        raise ValueError("lists must be a 2-D [m, K] array")
    m, K = lists.shape
    ks = [int(K)] if ks is None else [int(k) for k in ks]
    if any(k < 1 or k > K for k in ks):
        raise ValueError("every k must lie in [1, {}] (the length of the lists)".format(K))
    alpha = float(np.float32(smoothing))
    if not 0.0 < alpha < 1.0:
        raise ValueError("smoothing must lie in (0, 1) (got {!r})".format(smoothing))
    l_ptr, l_items = np.asarray(liked[0], dtype=np.int64), np.asarray(liked[1], dtype=np.int64)
    c_ptr, c_ids = np.asarray(cats[0], dtype=np.int64), np.asarray(cats[1], dtype=np.int64)
    n_items, G = len(c_ptr) - 1, int(c_ids.max()) + 1 if len(c_ids) else 1
    users = np.arange(m, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
    if len(users) != m:
        raise ValueError("users must name one user per list")
    oma = 1.0 - alpha
    kl = np.zeros((m, len(ks)), dtype=np.float64)
    count = np.zeros((m, len(ks)), dtype=np.int64)
    support = np.zeros(m, dtype=np.int64)

    def add_rows(acc, items):
        added = []
        for i in items:
            row = c_ids[c_ptr[i]:c_ptr[i + 1]] if 0 <= i < n_items else c_ids[:0]
            if len(row):
                acc[row] += 1.0 / len(row)                    # the ids of a row are distinct
            added.append(len(row) > 0)
        return added

    for j, u in enumerate(users):
        if not 0 <= u < len(l_ptr) - 1:
            continue
        p = np.zeros(G, dtype=np.float64)
        support[j] = sum(add_rows(p, l_items[l_ptr[u]:l_ptr[u + 1]]))
        full = np.cumsum(add_rows(np.zeros(G), lists[j]))       # the items with a category among the first r + 1 ranks
        if support[j]:
            p /= float(support[j])
        has = np.nonzero(p > 0)[0]
        for q, k in enumerate(ks):
            count[j, q] = full[k - 1]
            if not support[j]:
                continue
            n = np.zeros(G, dtype=np.float64)
            add_rows(n, lists[j, :k])
            qg = n / float(count[j, q]) if count[j, q] else n
            c = 0.0
            for t in (p[has] * np.log(p[has] / (oma * qg[has] + alpha * p[has]))).tolist():
                c += t
            kl[j, q] = c
    return kl, count, support


def relevant_csr(test_ratings, n_users, n_items):
    """The relevant (label 1) pairs of `test_ratings` as a CSR over users: (ptr int64 [n_users + 1], item ROWS int64, sorted and
    de-duplicated per user) — recommend.exclusion_csr over the liked pairs only."""
    from deep_cbrs_amar_renaissance_amd.recommend import exclusion_csr
    t = np.asarray(test_ratings)
    return exclusion_csr(t[t[:, 2] == 1] if len(t) else t, n_users, n_items)


def sampled_negatives(trainset, test_ratings, n_negatives=99, seed=0):
    """The candidate lists of the 1 + N sampled-negatives protocol, in host numpy.  For every user with a held-out positive (a
    label-1 pair of `test_ratings`) its held-out items plus `n_negatives` items it rated neither in `trainset.ratings` nor in
    `test_ratings` (whatever the label), drawn uniformly without replacement — all of them where fewer exist.  The draw of a user is
    a function of `seed` and the user's index alone: not of the other users, their order or their number.
    Returns (users int64 [n] ascending, lists int64 [n, P] of item NODE ids, -1 padded; a row holds the held-out items ascending,
    then the negatives ascending): the second form of `recommend_from(candidates=)`."""
    from deep_cbrs_amar_renaissance_amd.recommend import exclusion_csr
    if isinstance(n_negatives, bool) or not isinstance(n_negatives, (int, np.integer)) or n_negatives < 0:
        raise ValueError("n_negatives must be a non-negative integer (got {!r})".format(n_negatives))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("seed must be a non-negative integer (got {!r})".format(seed))
    n_users, n_items = len(trainset.users), len(trainset.items)
    t = np.asarray(test_ratings).reshape(-1, 3)
    pos_ptr, pos_items = relevant_csr(t, n_users, n_items)
    train = np.asarray(trainset.ratings).reshape(-1, 3)
    rated_ptr, rated_items = exclusion_csr(np.concatenate([train[:, :3], t]) if len(train) else t, n_users, n_items)
    users = np.flatnonzero(np.diff(pos_ptr) > 0).astype(np.int64)
    rows = []
    for u in users.tolist():
        free = np.ones(n_items, dtype=bool)
        free[rated_items[rated_ptr[u]:rated_ptr[u + 1]]] = False
        free = np.flatnonzero(free)
        if len(free) > n_negatives:
            free = np.sort(np.random.default_rng([int(seed), u]).choice(free, size=int(n_negatives), replace=False))
        rows.append(np.concatenate([pos_items[pos_ptr[u]:pos_ptr[u + 1]], free]))
    lists = np.full((len(users), max([len(r) for r in rows], default=0)), -1, dtype=np.int64)
    for j, r in enumerate(rows):
        lists[j, :len(r)] = r + n_users
    return users, lists


# Relevant CSRs on the device, built once per ratings array (held weakly, as recommend._EXCL_CACHE holds the exclusion CSRs).
_REL_CACHE = {}


def _relevant_device(test_ratings, n_users, n_items):
    import weakref
    dev = default_device()
    key = (id(test_ratings), n_users, n_items, str(dev))
    hit = _REL_CACHE.get(key)
    if hit is not None and hit[0]() is test_ratings and hit[1] == np.shape(test_ratings):
        return hit[2]
    ptr, items = relevant_csr(test_ratings, n_users, n_items)
    entry = (torch.from_numpy(ptr.astype(np.int32)).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev))
    try:
        ref = weakref.ref(test_ratings)
        weakref.finalize(test_ratings, _REL_CACHE.pop, key, None)
    except TypeError:                                    # not weakly referenceable: keep the array alive with its entry
        ref = (lambda obj: (lambda: obj))(test_ratings)
    _REL_CACHE[key] = (ref, np.shape(test_ratings), entry)
    return entry


def full_ranking_metrics_device(users, lists, test_ratings, ks, n_users, n_items):
    """`full_ranking_metrics` for lists that are still on the device (amar_rank_metrics_f64: a wavefront per user, float64 sums in a
    fixed order): `lists` int32 [m, K] item ROWS best first, -1 padded (what capi.recommend / capi.topk_segmented return), `users`
    the user index of every row (host or device integers; None: row j is user j, m == n_users).  The relevant CSR of `test_ratings`
    goes to the device once per array.  Returns the dict of `full_ranking_metrics`, same keys."""
    ks = [int(k) for k in ks]
    rel_ptr, rel_items = _relevant_device(test_ratings, int(n_users), int(n_items))
    if users is not None:
        if not isinstance(users, torch.Tensor):
            users = torch.from_numpy(np.asarray(users).reshape(-1).astype(np.int32))
        users = users.to(device=lists.device, dtype=torch.int32).contiguous()
    means, evaluated, skipped = capi.rank_metrics(lists, rel_ptr, rel_items, ks, users=users)
    out = {}
    for q, k in enumerate(ks):
        out.update({'precision_at_{}'.format(k): float(means[q, 0]), 'recall_at_{}'.format(k): float(means[q, 1]),
                    'ndcg_at_{}'.format(k): float(means[q, 2]), 'hit_at_{}'.format(k): float(means[q, 3])})
    out['users_evaluated'], out['users_skipped'] = evaluated, skipped
    return out


def precision_recall_f1_at_k(test_filepath, predictions_filepath, k, sep='\t', short_lists='skip', no_relevant='skip',
                             relevance_threshold=1.0, counts=None):
    """Precision / Recall / F1 @k of a top-k predictions file against the test ratings, as `mimir.jar -holdout -cutoff k`
    computes them (metrics.py:60-65) — restated from RiVal's ranking metrics, the library inside the jar
    (net.recommenders.rival.evaluation.metric.ranking.{AbstractRankingMetric,Precision,Recall}; there is no JVM here, so
    the jar itself cannot be run: what its behaviour cannot settle is an explicit switch below):

    * per TEST user with predictions, items are ranked by predicted score (the file's order inside a user is kept: the
      reference writes each user's rows best first, metrics.py:27-33) and each carries its test relevance
      (rating >= relevance_threshold -> relevant; an item absent from the user's test rows is not relevant);
    * P@k(u) = (relevant among the first k) / k, R@k(u) = (relevant among the first k) / (relevant test items of u);
    * RiVal records a user's value at cutoff k only when the ranked list REACHES rank k (`if (rank == at)`), so a user with
      fewer than k predicted items contributes to neither mean: short_lists='skip' (default).  'count' keeps such users
      with P = hits / k, R = hits / relevant — what an evaluator that pads short lists would report;
    * a user without any relevant test item has R = 0 / 0 = NaN, which RiVal's getValueAt drops from the recall mean
      (no_relevant='skip', default; 'zero' counts it as recall 0); its precision is 0 and is counted;
    * both means are plain averages over the remaining users; F1 = 2 P R / (P + R) of the two MEANS (the jar's f1Measure
      takes the aggregated precision and recall), 0 when both are 0.
    `relevance_threshold`: the jar's constant is not recoverable from its call site; with the {0, 1} ratings of every
    dataset in the reference any threshold in (0, 1] gives the same result.
    `counts` (a dict, optional) receives how many users each mean covers and how many the switches dropped — the defaults are
    RiVal's behaviour as restated from its source, NOT checked against mimir.jar, so what they exclude is
    reported with every result.
    """
    if short_lists not in ('skip', 'count') or no_relevant not in ('skip', 'zero'):
        raise ValueError("short_lists must be 'skip' or 'count', no_relevant 'skip' or 'zero'")
    test = pd.read_csv(test_filepath, sep=sep, header=None).to_numpy()
    pred = pd.read_csv(predictions_filepath, sep=sep, header=None).to_numpy()
    test_users = set(test[:, 0].astype(np.int64).tolist())
    liked = test[test[:, 2] >= relevance_threshold]
    liked_keys = set(zip(liked[:, 0].astype(np.int64).tolist(), liked[:, 1].astype(np.int64).tolist()))
    n_liked = pd.Series(liked[:, 0].astype(np.int64)).value_counts().to_dict()
    hits, listed = {}, {}
    for u, i in zip(pred[:, 0].astype(np.int64).tolist(), pred[:, 1].astype(np.int64).tolist()):
        if u not in test_users:
            continue                                              # RiVal walks the test model's users
        rank = listed.get(u, 0)
        if rank < k:                                              # only the first k rows of a user count
            hits[u] = hits.get(u, 0) + ((u, i) in liked_keys)
        listed[u] = rank + 1
    users = sorted(u for u in listed if short_lists == 'count' or listed[u] >= k)
    prec = [hits[u] / k for u in users]
    rec = [hits[u] / n_liked[u] if n_liked.get(u, 0) > 0 else (0.0 if no_relevant == 'zero' else None) for u in users]
    rec = [r for r in rec if r is not None]
    precision = float(np.mean(prec)) if prec else 0.0
    recall = float(np.mean(rec)) if rec else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    info = {'users_with_predictions': len(listed), 'users_in_precision_mean': len(prec), 'users_in_recall_mean': len(rec),
            'skipped_short_list': len(listed) - len(users), 'skipped_no_relevant_item': len(users) - len(rec),
            'short_lists': short_lists, 'no_relevant': no_relevant}
    if info['skipped_short_list'] or info['skipped_no_relevant_item']:
        logger.info("P/R/F1@%d of %s: %d users with fewer than %d predictions left out of both means (short_lists='%s'), %d users "
                    "without a relevant test item left out of the recall mean (no_relevant='%s')", k, predictions_filepath,
                    info['skipped_short_list'], k, short_lists, info['skipped_no_relevant_item'], no_relevant)
    if counts is not None:
        counts.update(info)
    return precision, recall, f1


def top_k_metrics(test_filepath, predictions_path, short_lists=None, no_relevant=None):
    """Write ``results.tsv`` (label, precision, recall, F1) next to every ``predictions*`` file found, and ``results_users.tsv``
    (users in the precision / recall means, users skipped by each switch) beside it.  The switches come from the arguments, else
    from AMAR_METRICS_SHORT_LISTS / AMAR_METRICS_NO_RELEVANT, else the RiVal defaults ('skip', 'skip')."""
    short_lists = short_lists or os.environ.get('AMAR_METRICS_SHORT_LISTS', 'skip')
    no_relevant = no_relevant or os.environ.get('AMAR_METRICS_NO_RELEVANT', 'skip')
    if not os.path.isdir(predictions_path):
        logger.error("Invalid predictions path specified. Unable to run evaluator.")
        return
    for root, _, files in os.walk(predictions_path):
        found = sorted(f for f in files if f.startswith("predictions"))
        if not found:
            continue
        cutoff = int(str(root)[root.rfind(os.sep):].split("_")[1])
        infos = [{} for _ in found]
        rows = [precision_recall_f1_at_k(test_filepath, os.path.join(root, f), cutoff, short_lists=short_lists, no_relevant=no_relevant,
                                         counts=info) for f, info in zip(found, infos)]
        p, r, f1 = np.mean(np.asarray(rows), axis=0)
        pd.DataFrame([["top_{}".format(cutoff), p, r, f1]]).to_csv(
            os.path.join(root, "results.tsv"), sep='\t', header=False, index=False)
        keys = ['users_with_predictions', 'users_in_precision_mean', 'users_in_recall_mean', 'skipped_short_list', 'skipped_no_relevant_item',
                'short_lists', 'no_relevant']
        pd.DataFrame([[f] + [info[key] for key in keys] for f, info in zip(found, infos)], columns=['file'] + keys).to_csv(
            os.path.join(root, "results_users.tsv"), sep='\t', index=False)


# ---- compiled metrics (Model.compile(metrics=...)): binary accuracy, Precision, Recall, AUC from integer counters ----------------------
AUC_BUCKETS = 199                                                      # include/amar_hip.h: AMAR_AUC_BUCKETS
N_COUNTERS = 4 + 2 * AUC_BUCKETS                                       # tp, fp, tn, fn, then hist[label][bucket]
_METRIC_ALIASES = {'accuracy': 'accuracy', 'acc': 'accuracy', 'binary_accuracy': 'accuracy', 'BinaryAccuracy': 'accuracy',
                   'Precision': 'precision', 'precision': 'precision', 'Recall': 'recall', 'recall': 'recall',
                   'AUC': 'auc', 'auc': 'auc'}
_KERAS_METRICS_WITHOUT_KERNEL = {
    'TopKCategoricalAccuracy', 'top_k_categorical_accuracy', 'SparseTopKCategoricalAccuracy', 'sparse_top_k_categorical_accuracy',
    'CategoricalAccuracy', 'categorical_accuracy', 'SparseCategoricalAccuracy', 'sparse_categorical_accuracy',
    'TruePositives', 'TrueNegatives', 'FalsePositives', 'FalseNegatives', 'PrecisionAtRecall', 'RecallAtPrecision',
    'SensitivityAtSpecificity', 'SpecificityAtSensitivity', 'MeanSquaredError', 'mean_squared_error', 'mse', 'MSE',
    'RootMeanSquaredError', 'MeanAbsoluteError', 'mean_absolute_error', 'mae', 'MAE', 'BinaryCrossentropy', 'binary_crossentropy',
    'CategoricalCrossentropy', 'categorical_crossentropy', 'KLDivergence', 'kl_divergence', 'CosineSimilarity', 'cosine_similarity',
    'Hinge', 'hinge', 'SquaredHinge', 'squared_hinge', 'LogCoshError', 'logcosh', 'Poisson', 'poisson', 'MeanIoU', 'BinaryIoU', 'F1Score',
}


def resolve_metrics(names):
    """History names ('accuracy', 'precision', 'recall', 'auc') of the compiled metrics, in compile order, each once.
    NotImplementedError: a metric Keras knows and the counters do not give; ValueError: any other name."""
    out = []
    for name in names or []:
        if not isinstance(name, str) or name not in _METRIC_ALIASES:
            supported = ', '.join(sorted(_METRIC_ALIASES))
            if isinstance(name, str) and name in _KERAS_METRICS_WITHOUT_KERNEL:
                raise NotImplementedError("metric '{}' is not computed here; supported: {}".format(name, supported))
            raise ValueError("unknown metric {!r}; supported: {}".format(name, supported))
        if _METRIC_ALIASES[name] not in out:
            out.append(_METRIC_ALIASES[name])
    return out


def resolve_compiled(loss, metrics):
    """(loss code, hyper, metric history names) of a Model.compile(loss=..., metrics=...), with the errors of `resolve_loss` and
    `resolve_metrics`.  Under BPRLoss the labels carry no meaning: 'accuracy' is accepted and left out, any other metric raises
    NotImplementedError."""
    from deep_cbrs_amar_renaissance_amd.utilities.losses import BPR, GROUP_KINDS, resolve_loss
    code, hyper, loss_name = resolve_loss(loss)
    names = resolve_metrics(metrics)
    if code == BPR or code in GROUP_KINDS:                           # (the listwise losses train on BPR's batches)
        if any(name != 'accuracy' for name in names):
            raise NotImplementedError("{} trains on (positive, negative) pairs whose labels carry no meaning: metrics {} are not "
                                      "defined under it".format(loss_name, [n for n in names if n != 'accuracy']))
        names = []
    return code, hyper, names


def auc_thresholds():
    """The 198 interior thresholds of Keras' AUC(num_thresholds=200): float32((i + 1) / 199) computed in double, as Keras does."""
    return (np.arange(1, AUC_BUCKETS, dtype=np.float64) / float(AUC_BUCKETS)).astype(np.float32)


def metric_counters(p, y):
    """The counter block of amar_loss_grad_f32 for probabilities p (compared as float32) and labels y, as int64 [N_COUNTERS]:
    tp, fp, tn, fn at threshold 0.5, then for each label the histogram of how many interior AUC thresholds p exceeds."""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    actual = np.asarray(y, dtype=np.float32).reshape(-1) > np.float32(0.5)
    predicted = p > np.float32(0.5)
    out = np.zeros(N_COUNTERS, dtype=np.int64)
    out[0], out[1] = np.sum(actual & predicted), np.sum(~actual & predicted)
    out[2], out[3] = np.sum(~actual & ~predicted), np.sum(actual & ~predicted)
    bucket = (p[:, None] > auc_thresholds()[None, :]).sum(axis=1) if len(p) else np.zeros(0, dtype=np.int64)
    for label in (0, 1):
        out[4 + label * AUC_BUCKETS:4 + (label + 1) * AUC_BUCKETS] = np.bincount(bucket[actual == bool(label)], minlength=AUC_BUCKETS)
    return out


def _div_no_nan(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=b != 0)


def metric_values(counters, names):
    """{history name: value} of the metrics `names` (as `resolve_metrics` returns them) from a counter block: accuracy = (tp + tn) / n,
    precision = tp / (tp + fp) and recall = tp / (tp + fn) with Keras' div_no_nan (0 for an empty denominator), auc = Keras'
    AUC(num_thresholds=200, curve='ROC', summation_method='interpolation'): cumulative counts above each of the 200 thresholds (every
    p in [0, 1] exceeds the first, -1e-7, and none the last, 1 + 1e-7), then the trapezoid rule over (false-positive rate, recall)."""
    c = np.asarray(counters, dtype=np.int64).reshape(-1)
    if len(c) != N_COUNTERS:
        raise ValueError("a counter block holds {} cells".format(N_COUNTERS))
    tp, fp, tn, fn = (float(v) for v in c[:4])
    out = {}
    for name in names:
        if name == 'accuracy':
            out[name] = float(_div_no_nan(tp + tn, tp + fp + tn + fn))
        elif name == 'precision':
            out[name] = float(_div_no_nan(tp, tp + fp))
        elif name == 'recall':
            out[name] = float(_div_no_nan(tp, tp + fn))
        elif name == 'auc':
            hist = c[4:].reshape(2, AUC_BUCKETS).astype(np.float64)
            above = np.concatenate([np.cumsum(hist[:, ::-1], axis=1)[:, ::-1], np.zeros((2, 1))], axis=1)   # [label, 200 thresholds]
            total = hist.sum(axis=1, keepdims=True)
            fpr, rec = _div_no_nan(above[0], total[0]), _div_no_nan(above[1], total[1])
            out[name] = float(np.sum((fpr[:-1] - fpr[1:]) * (rec[:-1] + rec[1:]) / 2.0))
        else:
            raise ValueError("no metric named {!r}".format(name))
    return out
