"""CPU: the host side of exact full-catalogue positions — the numpy reference against an argsort, the host restatement of the
cut-off-free metrics (`full_ranking_rank_metrics`) against the reference and on hand-checked cases, the binding's entry splitting,
the argument checks, and the declarations the binding rests on (pytest -m "not gpu")."""
import os
import re

import numpy as np
import pytest

from tests import rank_of_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scores(rng, n_users, n_items):
    """Random float32 scores with exact ties (duplicated columns) and saturated ones (many 1.0)."""
    S = rng.uniform(0, 1, size=(n_users, n_items)).astype(np.float32)
    if n_items > 6:
        S[:, n_items // 2] = S[:, 1]
        S[:, n_items - 1] = S[:, 1]
        S[:, 3] = S[:, 2]
        S[0, rng.choice(n_items, size=n_items // 2, replace=False)] = 1.0
        S[1, :] = 1.0
    return S


@pytest.mark.parametrize('n_items', [1, 7, 40])
def test_reference_counting_agrees_with_an_argsort(n_items):
    rng = np.random.default_rng(100 + n_items)
    S = _scores(rng, 6, n_items)
    for u in range(6):
        excluded = set(rng.choice(n_items, size=int(rng.integers(0, n_items)), replace=False).tolist())
        targets = sorted(rng.choice(n_items, size=int(rng.integers(1, n_items + 1)), replace=False).tolist())
        scores, greater, before, after = ref.counts(S[u], excluded, targets)
        assert np.array_equal(scores.view(np.int32), S[u][targets].view(np.int32))
        pos = ref.positions(S[u], excluded)
        for e, t in enumerate(targets):
            if t in excluded:
                # counted against the candidates like any other: the position it would take if it were one
                order = sorted([i for i in range(n_items) if i not in excluded] + [t], key=lambda i: (-float(S[u, i]), i))
                assert 1 + greater[e] + before[e] == order.index(t) + 1
            else:
                assert 1 + greater[e] + before[e] == pos[t], (u, t)
            same = sum(1 for i in range(n_items) if i not in excluded and i != t and S[u, i] == S[u, t])
            assert before[e] + after[e] == same


def test_host_metrics_agree_with_the_reference():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_rank_metrics
    rng = np.random.default_rng(5)
    n_users, n_items = 12, 50
    S = _scores(rng, n_users, n_items)
    excluded = [set(rng.choice(n_items, size=int(rng.integers(0, 30)), replace=False).tolist()) for _ in range(n_users)]
    relevant = [set(rng.choice(n_items, size=int(rng.integers(0, 12)), replace=False).tolist()) for _ in range(n_users)]
    relevant[2] = set()                                        # nothing held out
    excluded[3] = set(range(n_items))                          # no candidate
    excluded[4] = set(range(n_items)) - {5, 9}
    relevant[4] = {5, 9, 11}                                   # every candidate is a target: no negative
    relevant[5] = set(excluded[5])                             # everything held out was seen
    values, valid = full_ranking_rank_metrics(S, relevant, excluded, per_user=True)
    want = [ref.metrics(S[u], excluded[u], relevant[u]) for u in range(n_users)]
    assert valid.tolist() == [w[3] for w in want] and not valid[2] and not valid[3] and not valid[4]
    assert not valid[5]
    assert np.abs(values - np.array([w[:3] for w in want])).max() <= 1e-12
    out = full_ranking_rank_metrics(S, relevant, excluded)
    mean = np.array([w[:3] for w in want if w[3]]).mean(axis=0)
    assert abs(out['auc'] - mean[0]) <= 1e-12 and abs(out['mrr'] - mean[1]) <= 1e-12 and abs(out['map'] - mean[2]) <= 1e-12
    assert out['rank_metrics_users'] == (int(valid.sum()), int(n_users - valid.sum()))
    # nothing excluded at all
    free, free_valid = full_ranking_rank_metrics(S, relevant, None, per_user=True)
    want = [ref.metrics(S[u], None, relevant[u]) for u in range(n_users)]
    assert free_valid.tolist() == [w[3] for w in want]
    assert np.abs(free - np.array([w[:3] for w in want])).max() <= 1e-12
    nobody = full_ranking_rank_metrics(S[:1], [set()], None)
    assert nobody == {'auc': 0.0, 'mrr': 0.0, 'map': 0.0, 'rank_metrics_users': (0, 1)}


def test_host_metrics_hand_checked():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_rank_metrics
    S = np.array([[0.9, 0.1, 0.5, 0.3]], dtype=np.float32)
    v, ok = full_ranking_rank_metrics(S, [{0}], None, per_user=True)          # the relevant item first
    assert ok[0] and v[0].tolist() == [1.0, 1.0, 1.0]
    v, ok = full_ranking_rank_metrics(S, [{1}], None, per_user=True)          # the relevant item last
    assert ok[0] and v[0, 0] == 0.0 and v[0, 1] == 0.25 and v[0, 2] == 0.25
    v, ok = full_ranking_rank_metrics(np.full((1, 5), 0.5, dtype=np.float32), [{1, 3}], None, per_user=True)      # everything tied
    assert ok[0] and v[0, 0] == 0.5                                            # exactly
    assert v[0, 1] == 0.5 and v[0, 2] == (1 / 2 + 2 / 4) / 2                  # ties break on the item row: positions 2 and 4
    # two relevant items at positions 1 and 3 of 4: auc = 1 - (0 + 1) / (2 * 2), ap = (1 / 1 + 2 / 3) / 2
    v, ok = full_ranking_rank_metrics(S, [{0, 3}], None, per_user=True)
    assert ok[0] and v[0, 0] == 0.75 and v[0, 1] == 1.0 and abs(v[0, 2] - (1.0 + 2.0 / 3.0) / 2.0) <= 1e-15
    # an excluded item above the target does not count; an excluded relevant item is no target
    v, ok = full_ranking_rank_metrics(S, [{2, 0}], [{0}], per_user=True)
    assert ok[0] and v[0].tolist() == [1.0, 1.0, 1.0]


def test_auc_does_not_depend_on_the_item_numbering():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_rank_metrics
    rng = np.random.default_rng(9)
    n_items = 30
    S = _scores(rng, 4, n_items)
    S[2] = np.round(S[2] * 4) / 4                              # a handful of distinct values: many ties
    relevant = [set(rng.choice(n_items, size=6, replace=False).tolist()) for _ in range(4)]
    excluded = [set(rng.choice(n_items, size=8, replace=False).tolist()) for _ in range(4)]
    base, ok = full_ranking_rank_metrics(S, relevant, excluded, per_user=True)
    perm = rng.permutation(n_items)                            # item i becomes item perm[i]
    S2 = np.zeros_like(S)
    S2[:, perm] = S
    moved, ok2 = full_ranking_rank_metrics(S2, [{int(perm[i]) for i in r} for r in relevant], [{int(perm[i]) for i in e} for e in excluded],
                                           per_user=True)
    assert ok.all() and ok2.all()
    assert np.abs(base[:, 0] - moved[:, 0]).max() <= 1e-15
    # rr and ap follow the documented order (ties by item row): they are what the reference's sort gives for the renumbered items
    want = [ref.metrics(S2[u], {int(perm[i]) for i in excluded[u]}, {int(perm[i]) for i in relevant[u]}) for u in range(4)]
    assert np.abs(moved - np.array([w[:3] for w in want])).max() <= 1e-12


def test_entry_splitting():
    from deep_cbrs_amar_renaissance_amd import capi
    T = capi.RANK_OF_MAX_TARGETS
    users, ptr = capi.rank_of_entries([7, 3, 7, 9, 2], [0, 0, T, T + 1, 2 * T + 2, 4 * T + 3])
    assert users.dtype == np.int32 and ptr.dtype == np.int32
    assert users.tolist() == [3, 7, 9, 9, 2, 2, 2]
    assert ptr.tolist() == [0, T, T + 1, 2 * T + 1, 2 * T + 2, 3 * T + 2, 4 * T + 2, 4 * T + 3]
    assert np.diff(ptr).max() <= T
    users, ptr = capi.rank_of_entries([], [0])
    assert users.size == 0 and ptr.tolist() == [0]
    users, ptr = capi.rank_of_entries([4, 5], [0, 0, 0])
    assert users.size == 0 and ptr.tolist() == [0]
    for bad in (([1, 2], [0, 1]), ([1], [1, 2]), ([1, 2], [0, 3, 2])):
        with pytest.raises(ValueError):
            capi.rank_of_entries(*bad)


class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def test_host_side_refusals():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import check_rank_metrics
    assert check_rank_metrics(['map', 'auc', 'map']) == ('map', 'auc') and check_rank_metrics(('auc', 'mrr', 'map')) == ('auc', 'mrr', 'map')
    for bad in (['ndcg'], ['auc', 'AUC'], 'auc', [], [3], None, 5):
        with pytest.raises(ValueError):
            check_rank_metrics(bad)
    with pytest.raises(ValueError):                                             # before the model is looked at
        rec.evaluate_ranking(None, None, None, [], rank_metrics=['recall'])
    with pytest.raises(ValueError):                                             # no cutoff and no rank metric: nothing to do
        rec.evaluate_ranking(None, None, None, [])

    class Model(rec.SimilarSearch):
        pass

    n_users, n_items = 5, 7
    train = _Train(np.zeros((0, 3), dtype=np.int64), n_users, n_items)
    for users, items in (([0, 1], [5]), ([0], [5, 6]), ([5], [6]), ([-1], [6]), ([0], [4]), ([0], [12]), ([0.5], [6]), ([0], [6.0]),
                         (None, [6]), ([0], None)):
        with pytest.raises(ValueError):
            Model().rank_items(train, users, items)
    out = Model().rank_items(train, [], [])
    assert sorted(out) == sorted(rec.RANK_ITEMS_KEYS) and all(len(v) == 0 for v in out.values())
    assert out['rank'].dtype == np.int64 and out['score'].dtype == np.float32 and out['percentile'].dtype == np.float64
    ptr, items = rec.check_targets_csr(([0, 2, 2, 3], [1, 4, 0]), 3, 5)
    assert ptr.tolist() == [0, 2, 2, 3] and items.tolist() == [1, 4, 0]
    for bad in (([0, 2], [1, 4]), ([0, 2, 3], [4, 1, 0]), ([0, 2, 3], [1, 1, 0]), ([0, 1, 3], [1, 2, 5]), ([0, 1, 2], [1, 2, 3]), ([1, 2, 3], [1, 2, 3])):
        with pytest.raises(ValueError):
            rec.check_targets_csr(bad, 2, 5)


def test_heldout_targets_are_the_relevant_items_not_seen_in_training():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    rng = np.random.default_rng(4)
    n_users, n_items = 9, 15
    keys = rng.choice(n_users * n_items, size=80, replace=False)
    pairs = np.stack([keys // n_items, keys % n_items + n_users, rng.integers(0, 2, size=80)], axis=1)
    train, test = pairs[:45], np.concatenate([pairs[40:], pairs[50:55]])         # five pairs in both, five listed twice
    ts = _Train(train, n_users, n_items)
    for exclude_seen in (True, False):
        ptr, items, n_cand = rec.heldout_targets(ts, test, exclude_seen)
        assert rec.heldout_targets(ts, test, exclude_seen)[1] is items            # built once per pair of arrays
        for u in range(n_users):
            seen = {int(i) - n_users for uu, i, _ in train if uu == u} if exclude_seen else set()
            want = sorted({int(i) - n_users for uu, i, y in test if uu == u and y == 1} - seen)
            assert items[ptr[u]:ptr[u + 1]].tolist() == want, (exclude_seen, u)
            assert n_cand[u] == n_items - len(seen)


def test_header_binding_and_makefile_agree():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_rank_of_slices', 'amar_rank_of_f32', 'amar_rank_of_metrics_f64'):
        found = re.search(r'\b' + sym + r'\s*\(([^;]*)\)\s*;', header)
        assert found and sym in capi.SIGNATURES, sym
        assert len(found.group(1).split(',')) == len(capi.SIGNATURES[sym][1]), sym
    order = list(capi.SIGNATURES)
    assert order.index('amar_rank_metrics_f64') < order.index('amar_rank_of_slices') < order.index('amar_rank_of_f32') \
        < order.index('amar_rank_of_metrics_f64') < order.index('amar_rerank_mmr_f32')
    assert header.index('amar_rank_metrics_f64(') < header.index('amar_rank_of_f32(') < header.index('amar_rerank_mmr_f32(')
    assert int(re.search(r'#define\s+AMAR_RANK_OF_MAX_TARGETS\s+(\d+)', header).group(1)) == capi.RANK_OF_MAX_TARGETS
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_rank_of.hip' in re.search(r'^SRCS\s*=(.*)$', makefile, flags=re.M).group(1).split()
    lib = capi.load()
    assert all(hasattr(lib, sym) for sym in ('amar_rank_of_slices', 'amar_rank_of_f32', 'amar_rank_of_metrics_f64'))


def test_cpu_tensors_are_refused_not_computed():
    """The no-fallback rule: a call with host tensors raises AmarError instead of computing anything."""
    import torch
    from deep_cbrs_amar_renaissance_amd import capi
    w = [np.eye(16, dtype=np.float32), np.ones((16, 1), dtype=np.float32)]
    blob, _ = capi.chain_pack(w, [np.zeros(16, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    tu, ti = torch.zeros((4, 16)), torch.zeros((9, 16))
    with pytest.raises(capi.AmarError):
        capi.rank_of(tu, ti, torch.from_numpy(blob), [16, 16, 1], ['relu', 'sigmoid'], 'relu', [0, 1], [0, 1, 2], [3, 4])
    for bad in (dict(users=[4], tgt_ptr=[0, 1], tgt_items=[0]), dict(users=[0], tgt_ptr=[0, 1], tgt_items=[9]),
                dict(users=[0], tgt_ptr=[0, 2], tgt_items=[1])):
        with pytest.raises(ValueError):
            capi.rank_of(tu, ti, torch.from_numpy(blob), [16, 16, 1], ['relu', 'sigmoid'], 'relu', **bad)
    flat = torch.zeros(3), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(capi.AmarError):
        capi.rank_of_metrics(*flat, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([9], dtype=torch.int32))
    with pytest.raises(ValueError):
        capi.rank_of_metrics(*flat, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([9, 9], dtype=torch.int32))


def test_slice_count_is_the_rankers():
    import ctypes
    from deep_cbrs_amar_renaissance_amd import capi
    lib = capi.load()
    dims = (ctypes.c_int32 * 3)(16, 16, 1)
    for n_items in (1, 17, 1100, 50000):
        for req in (0, 1, 2, 5):
            assert lib.amar_rank_of_slices(37, n_items, dims, 2, req) == lib.amar_recommend_slices(37, n_items, dims, 2, req)
    assert lib.amar_rank_of_slices(-1, 10, dims, 2, 0) == -1
