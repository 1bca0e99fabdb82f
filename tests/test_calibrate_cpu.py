"""CPU: the float64 restatement of the calibrated re-ranking on hand-worked cases, the host metric against a double loop, the
category selection, the argument checks of the model methods and the seeds of the GPU grid (tests/calibrate_ref.py)."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import calibrate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_CASE = dict(P=17, G=64, lam=0.5, alpha=0.01)                    # the planted case whose lists the GPU test compares exactly


def _greedy(pool, scores, user, lam, alpha, k):
    cats, liked = ref.two_genre_case()
    return ref.greedy64(np.asarray(pool), np.asarray(scores, dtype=np.float32), ref.liked_of(liked, user), cats, 2, lam, alpha, k, n_items=24)


def test_a_70_30_user_gets_a_70_30_list():
    pool = list(range(0, 10)) + list(range(10, 20))                      # ten dramas, every one scored above the ten comedies
    scores = np.linspace(2.0, 1.0, 20)
    items, sc, v, kl, near = _greedy(pool, scores, 0, 0.0, 0.01, 10)
    assert sum(i < 10 for i in items) == 7 and sum(i >= 10 for i in items) == 3
    assert items[0] == 0                                                 # a drama first: 0.7 is nearer to it
    assert abs(kl[-1]) < 1e-6                                            # 7 : 3 is the target itself
    plain = _greedy(pool, scores, 0, 1.0, 0.01, 10)
    assert plain[0].tolist() == list(range(10))                          # the score order: ten dramas
    assert plain[3][-1] > 0.3


def test_trade_off_one_is_the_score_order_with_ties_by_position():
    pool = [12, 3, 20, 15, 1]
    scores = [0.5, 0.9, 0.9, 0.1, 0.7]
    items, sc, _, _, near = _greedy(pool, scores, 0, 1.0, 0.01, 5)
    assert items.tolist() == [3, 20, 1, 12, 15] and not near
    assert sc.tolist() == [np.float32(x) for x in (0.9, 0.9, 0.7, 0.5, 0.1)]


def test_neutral_items_leave_the_miscalibration_unchanged():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    cats, liked = ref.two_genre_case()
    lists = np.array([[0, 10, 1, -1, -1], [20, 0, 21, 10, 1]])
    kl, count, support = miscalibration(lists, [0, 0], liked, cats, (3, 5), 0.01)
    assert kl[0, 0] == kl[1, 1] and count.tolist() == [[3, 3], [1, 3]] and support.tolist() == [10, 10]
    # a neutral candidate's C is the current list's
    items, _, _, kl_steps, _ = _greedy([0, 20, 10], [1.0, 3.0, 2.0], 0, 0.9, 0.01, 3)
    assert items.tolist() == [20, 10, 0]                                 # the neutral item on its score; then 0.45 - 0.29 beats 0 - 0.11
    assert abs(kl_steps[0] - math.log(1.0 / float(np.float32(0.01)))) < 1e-6       # nothing with a category yet


def test_a_user_without_a_target_keeps_the_score_order():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    cats, liked = ref.two_genre_case()
    for user in (1, 2):                                                   # neutral liked items only; no liked item
        items, _, v, kl, near = _greedy([10, 0, 20, 11], [0.1, 0.4, 0.3, 0.2], user, 0.0, 0.01, 4)
        assert items.tolist() == [0, 20, 11, 10] and not near and np.all(kl == 0.0)
    kl, count, support = miscalibration(np.array([[0, 10], [0, 10]]), [1, 2], liked, cats, (1, 2), 0.01)
    assert np.all(kl == 0.0) and support.tolist() == [0, 0] and count.tolist() == [[1, 2], [1, 2]]


@pytest.mark.parametrize('alpha', [0.01, 0.5, 0.9])
def test_a_neutral_only_list_has_the_largest_miscalibration(alpha):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    cats, liked = ref.two_genre_case()
    kl, count, _ = miscalibration(np.array([[20, 21, -1], [0, 1, 2], [10, 11, 12]]), [0, 0, 0], liked, cats, (3,), alpha)
    top = math.log(1.0 / float(np.float32(alpha)))
    assert abs(kl[0, 0] - top) <= 1e-12 and count[0, 0] == 0
    assert np.all(kl >= 0) and np.all(kl <= top + 1e-12)


def test_miscalibration_against_a_double_loop():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    (ptr, ids, _), liked, pool, _, users = ref.planted_case(17, 65)
    ks, alpha = (1, 5, 17), float(np.float32(0.05))
    kl, count, support = miscalibration(pool, users, liked, (ptr, ids), ks, 0.05)
    assert kl.dtype == np.float64 and kl.shape == (ref.M_LISTS, 3)
    for j in range(ref.M_LISTS):
        p = [0.0] * 65
        sup = 0
        for i in ref.liked_of(liked, int(users[j])):
            row = ids[ptr[i]:ptr[i + 1]]
            sup += len(row) > 0
            for g in row:
                p[g] += 1.0 / len(row)
        assert support[j] == sup
        for q, k in enumerate(ks):
            n, cnt = [0.0] * 65, 0
            for i in pool[j, :k]:
                row = ids[ptr[i]:ptr[i + 1]] if i >= 0 else []
                cnt += len(row) > 0
                for g in row:
                    n[g] += 1.0 / len(row)
            want = 0.0
            for g in range(65):
                if sup and p[g] > 0:
                    pg = p[g] / sup
                    want += pg * math.log(pg / ((1.0 - alpha) * (n[g] / cnt if cnt else 0.0) + alpha * pg))
            assert count[j, q] == cnt and abs(kl[j, q] - want) <= 1e-12, (j, k, kl[j, q], want)
    assert np.array_equal(miscalibration(pool, users, liked, (ptr, ids), None, 0.05)[0][:, 0], kl[:, 2])
    for bad in (dict(ks=(18,)), dict(smoothing=0.0), dict(smoothing=1.0), dict(users=users[:3])):
        with pytest.raises(ValueError):
            miscalibration(pool, **dict(dict(users=users, liked=liked, cats=(ptr, ids), ks=(1,), smoothing=0.05), **bad))


class _Uip:
    """3 users, 5 items, 6 properties in one 'unary-uip' adjacency; property 5 is linked to no item, 0 and 3 to three items each."""
    users, items, ratings = np.arange(3), np.arange(5), np.zeros((0, 3), dtype=np.int64)
    links = [(0, 0), (0, 3), (1, 0), (1, 1), (2, 3), (2, 4), (3, 0), (3, 3), (3, 2), (3, 2)]         # item 4 has none; one duplicate

    def __init__(self):
        n = 3 + 5 + 6
        r = [3 + i for i, _ in self.links]
        c = [8 + p for _, p in self.links]
        self.adj_matrix = sp.coo_matrix((np.ones(2 * len(r)), (r + c, c + r)), shape=(n, n)).tocsr()


class _NoTables:
    users, items, ratings = np.arange(3), np.arange(5), np.zeros((0, 3), dtype=np.int64)


def test_item_category_csr_selection_and_refusals():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    t = _Uip()
    ptr, ids, props, max_row = rec.item_category_csr(t)
    assert props.tolist() == [0, 1, 2, 3, 4] and max_row == 3                       # df > 0 only, ascending property index
    assert ptr.tolist() == [0, 2, 4, 6, 9, 9] and ids.tolist() == [0, 3, 0, 1, 3, 4, 0, 2, 3]
    ptr, ids, props, max_row = rec.item_category_csr(t, 3)                          # df 3, 3, then the tie 1 | 2 | 4 goes to property 1
    assert props.tolist() == [0, 1, 3] and ptr.tolist() == [0, 2, 4, 5, 7, 7] and ids.tolist() == [0, 2, 0, 1, 2, 0, 2] and max_row == 2
    ptr, ids, props, _ = rec.item_category_csr(t, [4, 2])
    assert props.tolist() == [2, 4] and ptr.tolist() == [0, 0, 0, 1, 2, 2] and ids.tolist() == [1, 0]
    dense = np.array([[1, 0], [0, 0], [1, 1], [0, 1], [0, 0]])
    for matrix in (dense, sp.csr_matrix(dense)):
        ptr, ids, props, max_row = rec.item_category_csr(_NoTables(), matrix)
        assert ptr.tolist() == [0, 1, 1, 3, 4, 4] and ids.tolist() == [0, 0, 1, 1] and props.tolist() == [0, 1] and max_row == 2
    for bad in ([0, 0], [6], [-1], 0, rec.capi.CALIBRATE_MAX_G + 1, True, 'genre', 2.5, [1.5], np.zeros((4, 2)),
                np.zeros((5, rec.capi.CALIBRATE_MAX_G + 1)), [[1, 0], [0, 1]], [[0, 1]]):
        with pytest.raises(ValueError):
            rec.item_category_csr(t, bad)
    with pytest.raises(ValueError, match='membership matrix'):
        rec.item_category_csr(_NoTables())


def test_model_methods_refuse_bad_arguments_before_any_work(monkeypatch):
    from deep_cbrs_amar_renaissance_amd import recommend as rec

    class Model(rec.SimilarSearch):
        def recommend(self, *args, **kwargs):
            raise AssertionError("the arguments are checked first")

    model = Model()
    for kwargs in (dict(k=10, pool=9), dict(k=10, pool=rec.K_MAX + 1), dict(k=0), dict(k=65, pool=65), dict(pool=50.0),
                   dict(trade_off=-0.1), dict(trade_off=1.5), dict(trade_off=float('nan')), dict(trade_off='0.5'),
                   dict(smoothing=0.0), dict(smoothing=1.0), dict(smoothing=float('nan')), dict(smoothing='0.01'),
                   dict(smoothing=1e-60), dict(categories=0), dict(categories='genre')):
        with pytest.raises(ValueError):
            model.recommend_calibrated(_NoTables(), **kwargs)
    with pytest.raises(ValueError, match='membership matrix'):             # no properties and no matrix
        model.recommend_calibrated(_NoTables())
    # a bool is not the integer it equals, a nested list is not a matrix: neither may ride on a cached entry
    uip, seen = _Uip(), []
    monkeypatch.setattr(rec, '_device_cached', lambda cache, obj, key, build: seen.append(key) or build())
    monkeypatch.setattr(rec, 'default_device', lambda: 'cpu')
    assert rec._cats_device(uip, 5, 1)[2] == 1 and len(seen) == 1
    for bad in (True, [[1, 0]], 2.5):
        with pytest.raises(ValueError):
            rec._cats_device(uip, 5, bad)
    assert len(seen) == 1 or all(key != seen[0] for key in seen[1:])
    for kwargs in (dict(smoothing=0.0), dict(smoothing=2), dict(users=[3]), dict(users=[0.5]), dict(categories=[9])):
        with pytest.raises(ValueError):
            model.list_calibration(_Uip(), np.zeros((3, 2), dtype=np.int64), **kwargs)
    with pytest.raises(ValueError, match='calibration'):
        rec.evaluate_ranking(None, _NoTables(), np.zeros((0, 3)), [5], calibration={'smoothing': 0.01, 'k': 3})
    with pytest.raises(ValueError):
        rec.evaluate_ranking(None, _NoTables(), np.zeros((0, 3)), [5], calibration={'smoothing': 1.5})


def test_entry_points_are_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_rerank_calibrated_f32', 'amar_list_calibration_f64'):
        assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header)
        declared = re.search(r'\bint\s+' + sym + r'\s*\(([^;]*)\);', header).group(1)
        assert len(declared.split(',')) == len(capi.SIGNATURES[sym][1])
    assert callable(capi.rerank_calibrated) and callable(capi.list_calibration)
    assert re.search(r'#define\s+AMAR_CALIBRATE_MAX_G\s+1024\b', header) and capi.CALIBRATE_MAX_G == 1024
    assert re.search(r'#define\s+AMAR_CALIBRATE_POOL_BUDGET\s+{}\b'.format(ref.POOL_BUDGET), header) and capi.CALIBRATE_POOL_BUDGET == ref.POOL_BUDGET
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_calibrate.hip' in makefile


def test_planted_case_holds_what_the_gpu_grid_needs():
    (ptr, ids, max_row), liked, pool, scores, users = ref.planted_case(64, 64)
    lens = np.diff(ptr)
    assert lens[0] == 0 and lens[1] == 1 and lens[2] == 64 == max_row and (lens == 0).sum() > 10
    liked_lens = np.diff(liked[0])
    assert set(ref.LIKED_LENGTHS) <= set(liked_lens.tolist())
    assert all(lens[i] == 0 for i in ref.liked_of(liked, 8)) and len(ref.liked_of(liked, 8)) > 1 and liked_lens[7] == 1
    valid = (pool >= 0).sum(axis=1)
    assert valid[0] == 0 and valid[1] == 1 and (valid == 64).sum() >= ref.FULL_LISTS and {0, 1, 2} <= set(pool[3].tolist())
    assert np.any(pool[2, :np.nonzero(pool[2] >= 0)[0].max()] == -1)                # holes, not a prefix
    assert np.array_equal(users, np.arange(ref.M_LISTS))
    for j in range(len(pool)):
        row = pool[j][pool[j] >= 0]
        assert len(set(row.tolist())) == len(row) and np.all(row < ref.N_ITEMS)
    # the dense variants put a full pool's rows past the staging budget, the plain ones keep them inside
    for P, G in ref.DENSE_CASES:
        (dptr, _, _), _, dpool, _, _ = ref.planted_case(P, G, dense=True)
        assert np.diff(dptr)[dpool[-1]].sum() > ref.POOL_BUDGET
    assert lens[pool[-1]].sum() <= ref.POOL_BUDGET


@pytest.mark.parametrize('G', ref.GRID_G)
@pytest.mark.parametrize('P', ref.GRID_P)
def test_gpu_grid_seeds_stay_within_the_near_tie_cap(P, G):
    """The lists of every kernel-grid case that float64 itself cannot tell apart (a step where another candidate stands within the
    two tolerances of the pick) number at most MAX_NEAR_TIE_LISTS: the census at k = P covers every smaller k, whose steps are a
    prefix."""
    for lam in ref.GRID_LAMBDA:
        case = ref.grid_case(P, G, lam)
        if lam > 0:
            assert ((case[2] >= 0).sum(axis=1) == P).sum() >= ref.FULL_LISTS        # full width wherever the scores count
        for alpha in ref.GRID_ALPHA:
            near = ref.near_tie_lists(case, G, lam, alpha, P)
            assert near <= ref.MAX_NEAR_TIE_LISTS, (P, G, lam, alpha, near)
            if dict(P=P, G=G, lam=lam, alpha=alpha) == EXACT_CASE:
                assert near == 0


@pytest.mark.parametrize('P,G', ref.DENSE_CASES)
def test_dense_cases_stay_within_the_near_tie_cap(P, G):
    case = ref.planted_case(P, G, dense=True)
    for lam, alpha, k in ref.dense_settings(P):
        assert ref.near_tie_lists(case, G, lam, alpha, k) <= ref.MAX_NEAR_TIE_LISTS, (P, G, lam, alpha, k)
