"""CPU: the float64 restatement of the diversified re-ranking (tests/diversify_ref.py) on hand-computed cases, the host ILD metric,
the declarations of the two entry points, the argument refusals of recommend_diverse, and the near-tie census of the GPU grid's seeds."""
import os
import re

import numpy as np
import pytest

from tests import diversify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# four unit-ish vectors in the plane: rows 0 and 1 almost parallel, row 2 orthogonal to row 0, row 3 opposite to row 0, row 4 zero
T = np.array([[1, 0, 0, 0], [0.8, 0.6, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32)


def _run(pool, scores, lam, k, metric='cosine', table=T):
    return ref.mmr64(np.asarray(pool), np.asarray(scores, dtype=np.float64), ref.sim(table, metric), lam, k)


def test_lambda_one_is_the_score_order():
    pos, items, scores, v, _ = _run([2, 0, 3, 1], [0.1, 0.9, 0.5, 0.9], 1.0, 3)
    assert pos == [1, 3, 2] and items.tolist() == [0, 1, 3] and scores.tolist() == [0.9, 0.9, 0.5]      # the tie: position 1 before 3
    assert np.allclose(v, [1.0, 1.0, 0.5])


def test_lambda_zero_takes_the_least_similar_remaining_item():
    # step 0: the best score (row 0).  Then: sims to row 0 are 0.8 (row 1), 0 (row 2), -1 (row 3), 0 (row 4) -> row 3; then the
    # maxima over {0, 3} are 0.8, 0, 0 -> row 2 (position 2) before the zero row (position 4) on the tie
    pos, items, _, v, _ = _run([0, 1, 2, 3, 4], [5, 4, 3, 2, 1], 0.0, 5)
    assert items.tolist() == [0, 3, 2, 4, 1] and pos == [0, 3, 2, 4, 1]
    assert np.allclose(v, [0.0, 1.0, 0.0, 0.0, -0.8])


def test_trade_off_in_between_by_hand():
    # lam = 0.5, scores 1, 0.9, 0.5, 0 -> rel the same.  Step 1: 0.45 - 0.4 = 0.05 (row 1), 0.25 - 0 (row 2), 0 + 0.5 (row 3) -> row 3
    pos, items, scores, v, gaps = _run([0, 1, 2, 3], [1.0, 0.9, 0.5, 0.0], 0.5, 3)
    assert items.tolist() == [0, 3, 2] and scores.tolist() == [1.0, 0.0, 0.5]
    assert np.allclose(v, [0.5, 0.5, 0.25]) and np.allclose(gaps[:2], [0.1, 0.25])


def test_equal_scores_give_rel_one_and_ties_go_to_the_smaller_position():
    assert ref.rel64([2.0, 2.0, 2.0]).tolist() == [1.0, 1.0, 1.0] and ref.rel64([7.0]).tolist() == [1.0]
    pos, items, _, v, _ = _run([2, 0, 1], [2.0, 2.0, 2.0], 0.7, 3)
    assert pos[0] == 0 and v[0] == 0.7                                   # all rel equal: position 0
    # after row 2: row 0 has sim 0, row 1 has 0.6 -> row 0
    assert items.tolist() == [2, 0, 1]


def test_zero_rows_are_similar_to_nothing():
    grid = ref.sim(T, 'cosine')
    assert np.all(grid[4] == 0) and np.all(grid[:, 4] == 0) and not np.isnan(grid).any()
    assert ref.ild64([4, 0], grid) == (1.0, 2)


def test_short_lists_are_padded():
    pos, items, scores, v, gaps = _run([1, 3, -1, -1], [0.2, 0.4, 9.0, 9.0], 0.3, 4)
    assert pos == [1, 0] and items.tolist() == [3, 1, -1, -1]
    assert scores.tolist()[:2] == [0.4, 0.2] and np.all(np.isneginf(scores[2:])) and np.all(np.isneginf(v[2:]))
    assert _run([-1, -1], [0.0, 0.0], 0.5, 2)[1].tolist() == [-1, -1]
    assert ref.ild64([-1, -1], ref.sim(T, 'dot')) == (0.0, 0) and ref.ild64([2, -1], ref.sim(T, 'dot')) == (0.0, 1)


@pytest.mark.parametrize('metric', ['dot', 'cosine'])
def test_intra_list_diversity_against_a_double_loop(metric):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import intra_list_diversity
    rng = np.random.default_rng(8)
    X = rng.normal(0, 1, size=(30, 12)).astype(np.float32)
    X[7] = 0
    lists = np.stack([rng.choice(30, size=9, replace=False) for _ in range(11)])
    lists[0, :] = -1
    lists[1, 1:] = -1
    lists[2, 4:] = -1
    lists[3, 0] = 7
    ks = (1, 2, 5, 9)
    ild, count = intra_list_diversity(lists, X, ks, metric)
    assert ild.shape == (11, 4) and ild.dtype == np.float64 and count.shape == (11, 4)
    x64 = X.astype(np.float64)
    for j in range(11):
        for q, k in enumerate(ks):
            head = [i for i in lists[j, :k] if i >= 0]
            total, pairs = 0.0, 0
            for a in range(len(head)):
                for b in range(a + 1, len(head)):
                    s = float(x64[head[a]] @ x64[head[b]])
                    if metric == 'cosine':
                        na, nb = np.sqrt(x64[head[a]] @ x64[head[a]]), np.sqrt(x64[head[b]] @ x64[head[b]])
                        s = s / (na * nb) if na > 0 and nb > 0 else 0.0
                    total, pairs = total + 1.0 - s, pairs + 1
            assert count[j, q] == len(head)
            assert abs(ild[j, q] - (total / pairs if pairs else 0.0)) <= 1e-12
            assert abs(ild[j, q] - ref.ild64(lists[j, :k], ref.sim(X, metric))[0]) <= 1e-12
    assert np.array_equal(intra_list_diversity(lists, X, None, metric)[0][:, 0], ild[:, 3])
    with pytest.raises(ValueError):
        intra_list_diversity(lists, X, (10,), metric)
    with pytest.raises(ValueError):
        intra_list_diversity(lists, X, (1,), 'euclid')


def test_entry_points_are_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_rerank_mmr_f32', 'amar_list_diversity_f64'):
        assert sym in capi.SIGNATURES and re.search(r'\bint\s+' + sym + r'\s*\(', header)
    assert callable(capi.rerank_mmr) and callable(capi.list_diversity)
    assert re.search(r'#define\s+AMAR_DIVERSIFY_MAX_P\s+64\b', header) and capi.DIVERSIFY_MAX_P == 64
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_diversify.hip' in makefile


class _NoTables:
    users, items, ratings = np.arange(3), np.arange(5), np.zeros((0, 3), dtype=np.int64)


def test_recommend_diverse_refuses_bad_arguments_before_any_work():
    from deep_cbrs_amar_renaissance_amd import recommend as rec

    class Model(rec.SimilarSearch):
        def _embedding_spaces(self):
            raise AssertionError("the arguments are checked first")

        def recommend(self, *args, **kwargs):
            raise AssertionError("the arguments are checked first")

    model = Model()
    for kwargs in (dict(k=10, pool=9), dict(k=10, pool=rec.K_MAX + 1), dict(k=0), dict(k=65, pool=65), dict(pool=50.0),
                   dict(trade_off=-0.1), dict(trade_off=1.5), dict(trade_off=float('nan')), dict(trade_off='0.5'),
                   dict(metric='euclid')):
        with pytest.raises(ValueError):
            model.recommend_diverse(_NoTables(), **kwargs)
    with pytest.raises(AssertionError, match='checked first'):              # good arguments get past the checks
        model.recommend_diverse(_NoTables(), k=10, pool=10, trade_off=1)


def test_evaluate_ranking_refuses_unknown_diversity_keys():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    with pytest.raises(ValueError, match='diversity'):
        rec.evaluate_ranking(None, _NoTables(), np.zeros((0, 3)), [5], diversity={'metric': 'cosine', 'k': 3})
    with pytest.raises(ValueError):
        rec.evaluate_ranking(None, _NoTables(), np.zeros((0, 3)), [5], diversity={'metric': 'euclid'})


def test_planted_case_holds_what_the_gpu_grid_needs():
    T_, pool, scores = ref.planted_case(33, 20, 'cosine')
    valid = (pool >= 0).sum(axis=1)
    assert valid[0] == 0 and valid[1] == 1 and valid[2] == 3 and valid[3] == 33
    assert (valid == 33).sum() >= ref.FULL_LISTS + 1                  # list 3 and the full lists reach every unit of the Gram matrix
    assert np.all(T_[3] == 0) and np.array_equal(T_[1], T_[150]) and {3, 1, 150} <= set(pool[3].tolist())
    for j in range(len(pool)):
        row = pool[j, :valid[j]]
        assert np.all(pool[j, valid[j]:] == -1) and len(set(row.tolist())) == len(row) and np.all(row < ref.N_ROWS)
    assert any(np.any(np.diff(scores[j, :valid[j]]) > 0) for j in range(4, len(pool)))          # unsorted pools


@pytest.mark.parametrize('metric', ref.GRID_METRIC)
@pytest.mark.parametrize('d', ref.GRID_D)
def test_gpu_grid_seeds_stay_within_the_near_tie_cap(d, metric):
    """The lists of every kernel-grid case that float64 itself cannot tell apart (a step whose gap to the runner-up is below
    2 tol_v) number at most MAX_NEAR_TIE_LISTS: the census at k = P covers every smaller k, whose steps are a prefix."""
    for P in ref.GRID_P:
        T_, pool, scores = ref.planted_case(P, d, metric)
        for lam in ref.GRID_LAMBDA:
            near = ref.near_tie_lists(T_, pool, scores, metric, lam, P)
            assert near <= ref.MAX_NEAR_TIE_LISTS, (P, d, metric, lam, near)
