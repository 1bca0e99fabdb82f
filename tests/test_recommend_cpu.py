"""Full-catalogue recommendation, host side (no GPU): metrics, the output frame, the exclusion CSR, argument checks."""
import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import recommend as rec
from deep_cbrs_amar_renaissance_amd.utilities import metrics


def _log2(r):
    return 1.0 / np.log2(r + 1.0)


def test_full_ranking_metrics_hand_computed():
    # 3 users, node ids: items are 10.. (|U| = 10 in the id space the lists use)
    users = np.array([0, 1, 2])
    items = np.array([[10, 11, 12, 13],         # user 0: relevant {10, 12} -> hits at ranks 1 and 3
                      [14, 15, -1, -1],         # user 1: a list shorter than k; relevant {15, 19}
                      [10, 11, 12, 13]])        # user 2: only a label-0 test item -> skipped
    test = np.array([[0, 10, 1], [0, 12, 1], [0, 13, 0], [1, 15, 1], [1, 19, 1], [2, 11, 0]])
    got = metrics.full_ranking_metrics(users, items, test, [1, 3, 4])
    assert got['users_evaluated'] == 2 and got['users_skipped'] == 1
    # k = 3
    p0, r0 = 2 / 3, 2 / 2
    ndcg0 = (_log2(1) + _log2(3)) / (_log2(1) + _log2(2))
    p1, r1 = 1 / 3, 1 / 2
    ndcg1 = _log2(2) / (_log2(1) + _log2(2))
    assert got['precision_at_3'] == pytest.approx((p0 + p1) / 2)
    assert got['recall_at_3'] == pytest.approx((r0 + r1) / 2)
    assert got['ndcg_at_3'] == pytest.approx((ndcg0 + ndcg1) / 2)
    assert got['hit_at_3'] == pytest.approx(1.0)
    # k = 1: user 0 hits, user 1 misses
    assert got['precision_at_1'] == pytest.approx(0.5)
    assert got['recall_at_1'] == pytest.approx((1 / 2 + 0) / 2)
    assert got['ndcg_at_1'] == pytest.approx(0.5)
    assert got['hit_at_1'] == pytest.approx(0.5)
    # k = 4: the short list's missing ranks are misses; IDCG over min(|relevant|, k) = 2 ranks
    assert got['precision_at_4'] == pytest.approx((2 / 4 + 1 / 4) / 2)
    assert got['ndcg_at_4'] == pytest.approx((ndcg0 + ndcg1) / 2)
    with pytest.raises(ValueError):
        metrics.full_ranking_metrics(users, items, test, [5])


def test_full_ranking_metrics_without_relevant_users():
    got = metrics.full_ranking_metrics(np.array([0]), np.array([[5, 6]]), np.array([[0, 5, 0]]), [2])
    assert got['users_evaluated'] == 0 and got['users_skipped'] == 1
    assert got['precision_at_2'] == 0.0 and got['hit_at_2'] == 0.0


def test_recommendations_frame_maps_ids_like_top_k_predictions():
    user_ids = np.array([101, 102, 103])
    item_ids = np.array([7, 8, 9, 11])
    users = np.array([2, 0])
    items = np.array([[4, 6, -1], [3, 5, 6]])           # node ids: item row + |U| (3)
    scores = np.array([[0.9, 0.5, -np.inf], [0.8, 0.7, 0.1]], dtype=np.float32)
    df = metrics.recommendations_frame(users, items, scores, user_ids, item_ids)
    assert list(df.columns) == ['users', 'items', 'scores']
    assert df['users'].tolist() == [103, 103, 101, 101, 101]
    assert df['items'].tolist() == [8, 11, 7, 9, 11]
    assert np.allclose(df['scores'].to_numpy(), [0.9, 0.5, 0.8, 0.7, 0.1])
    assert df['scores'].dtype == np.float64


def test_exclusion_csr_sorted_and_deduplicated():
    n_users, n_items = 3, 5
    # node ids: items are 3..7; duplicates and both labels, unsorted
    ratings = np.array([[1, 7, 1], [0, 4, 0], [1, 3, 1], [1, 7, 0], [0, 4, 1], [0, 3, 1], [1, 5, 1]])
    ptr, items = rec.exclusion_csr(ratings, n_users, n_items)
    assert ptr.tolist() == [0, 2, 5, 5]
    assert items.tolist() == [0, 1, 0, 2, 4]
    with pytest.raises(ValueError):
        rec.exclusion_csr(np.array([[0, 9, 1]]), n_users, n_items)
    ptr, items = rec.exclusion_csr(np.zeros((0, 3), dtype=np.int64), n_users, n_items)
    assert ptr.tolist() == [0, 0, 0, 0] and items.size == 0


def test_argument_validation():
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            rec.check_k(bad)
    assert rec.check_k(1) == 1 and rec.check_k(64) == 64
    with pytest.raises(ValueError):
        rec.check_users([0, 4], 4)
    with pytest.raises(ValueError):
        rec.check_users([-1], 4)
    assert rec.check_users([3, 0, 2], 4).tolist() == [3, 0, 2]
    assert rec.check_users(None, 3).tolist() == [0, 1, 2]


class _Train:
    def __init__(self, n_users, n_items):
        self.users, self.items = np.arange(n_users), np.arange(n_items)
        self.ratings = np.zeros((0, 3), dtype=np.int64)


def test_models_reject_bad_arguments_before_any_device_work():
    """recommend() / _recommend_pairs() of every scoring class validate k and the users before touching the towers."""
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    train = _Train(4, 3)
    for cls in (basic.BasicRS, basic.BasicGNN, hybrid.HybridCBRS, hybrid.HybridBertGNN):
        model = object.__new__(cls)                     # no weights needed: the checks come first
        for method in (cls.recommend, cls._recommend_pairs):
            with pytest.raises(ValueError):
                method(model, train, k=0)
            with pytest.raises(ValueError):
                method(model, train, k=65)
            with pytest.raises(ValueError):
                method(model, train, k=5, users=[0, 4])
    for name in ('BasicGCN', 'BasicTSGCN', 'BasicTWGCN'):
        assert hasattr(getattr(basic, name), 'recommend')
    for name in ('HybridBertGCN', 'HybridBertTSGCN'):
        assert hasattr(getattr(hybrid, name), 'recommend')
