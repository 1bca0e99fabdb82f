"""CPU: the host side of group recommendation — group and exclusion CSRs, argument checks, the numpy reference on a hand-worked
case, and the declarations the binding rests on (pytest -m "not gpu")."""
import os
import re

import numpy as np
import pytest

from tests import group_recommend_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_csr_sorts_and_checks():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    ptr, users = rec.group_csr([[5, 1, 3], [], (2,), np.array([9, 0])], 10)
    assert ptr.dtype == np.int32 and users.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 4, 6] and users.tolist() == [1, 3, 5, 2, 0, 9]
    ptr, users = rec.group_csr([], 10)
    assert ptr.tolist() == [0] and users.size == 0
    ptr, users = rec.group_csr(np.array([[3, 2], [0, 1]]), 4)                  # a 2-D array: one group per row
    assert ptr.tolist() == [0, 2, 4] and users.tolist() == [2, 3, 0, 1]
    for bad in ([[1, 1]], [[0, 10]], [[-1]], [[0.5, 1.0]], [3, 4], 'ab', ['ab'], 7, None, [[[1]]]):
        with pytest.raises(ValueError):
            rec.group_csr(bad, 10)


def test_group_exclusion_csr_is_the_union_of_the_members():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    rng = np.random.default_rng(3)
    n_users, n_items = 12, 20
    keys = rng.choice(n_users * n_items, size=90, replace=False)
    ratings = np.stack([keys // n_items, keys % n_items + n_users, rng.integers(0, 2, size=90)], axis=1)
    ratings = np.concatenate([ratings, ratings[:7]])                           # duplicate pairs collapse
    ratings = ratings[ratings[:, 0] != 4]                                      # user 4 has no training pair
    groups = [[0, 1, 2], [], [4], [11, 3, 7, 0], [5], [4, 5]]
    ptr, users = rec.group_csr(groups, n_users)
    eptr, eitems = rec.group_exclusion_csr(ratings, ptr, users, n_users, n_items)
    assert eptr.shape == (len(groups) + 1,) and eptr[0] == 0
    for j, members in enumerate(groups):
        want = sorted({int(i) - n_users for u, i, _ in ratings if u in members})
        assert eitems[eptr[j]:eptr[j + 1]].tolist() == want, j
    eptr, eitems = rec.group_exclusion_csr(np.zeros((0, 3), dtype=np.int64), ptr, users, n_users, n_items)
    assert eptr.tolist() == [0] * (len(groups) + 1) and eitems.size == 0


def test_check_strategy_and_min_score():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    assert [rec.check_strategy(s) for s in ('mean', 'min', 'max')] == ['mean', 'min', 'max']
    for bad in ('avg', '', None, 0):
        with pytest.raises(ValueError):
            rec.check_strategy(bad)
    assert rec.check_min_score(None) == float('-inf') and rec.check_min_score(float('-inf')) == float('-inf')
    assert rec.check_min_score(0.25) == 0.25 and rec.check_min_score(np.float32(0.5)) == 0.5 and rec.check_min_score(1) == 1.0
    for bad in (float('nan'), np.float32('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            rec.check_min_score(bad)


# 3 users, 4 items; items 0 and 2 tie under every strategy for the group {0, 1}
S = np.array([[0.50, 0.25, 0.50, 0.75],
              [0.25, 0.75, 0.25, 0.10],
              [0.90, 0.10, 0.30, 0.20]], dtype=np.float32)


@pytest.mark.parametrize('strategy,want_items,want_scores', [
    ('mean', [1, 3, 0, 2], [0.5, 0.425, 0.375, 0.375]),
    ('min', [0, 1, 2, 3], [0.25, 0.25, 0.25, 0.10]),
    ('max', [1, 3, 0, 2], [0.75, 0.75, 0.5, 0.5])])
def test_reference_hand_worked(strategy, want_items, want_scores):
    items, scores = ref.group_topk(S, [1, 0], [], 4, strategy)
    assert items.tolist() == want_items and scores.dtype == np.float32
    want = np.array(want_scores, dtype=np.float32)
    if strategy == 'mean':
        want = (S[0] + S[1])[want_items] / np.float32(2)
    assert np.array_equal(scores.view(np.int32), want.view(np.int32))
    # the member order a caller lists does not matter; an excluded item leaves, the list is padded
    again, _ = ref.group_topk(S, [0, 1], [], 4, strategy)
    assert again.tolist() == want_items
    items, scores = ref.group_topk(S, [0, 1], [1], 4, strategy)
    assert items.tolist() == [i for i in want_items if i != 1] + [-1] and np.isneginf(scores[3])
    # veto at 0.25: item 3 (user 1 scores it 0.10) is dropped, the rest stays in order
    items, _ = ref.group_topk(S, [0, 1], [], 2, strategy, min_score=0.25)
    assert items.tolist() == [i for i in want_items if i != 3][:2]
    # three members under 'mean': ((s0 + s1) + s2) / 3 in float32
    if strategy == 'mean':
        agg = ref.aggregate(S, [2, 0, 1], 'mean')
        assert np.array_equal(agg.view(np.int32), (((S[0] + S[1]) + S[2]) / np.float32(3)).view(np.int32))
    # an empty group and a veto nobody passes: all padding
    assert ref.group_topk(S, [], [], 3, strategy)[0].tolist() == [-1, -1, -1]
    assert ref.group_topk(S, [0, 1, 2], [], 3, strategy, min_score=2.0)[0].tolist() == [-1, -1, -1]
    # a group of one is the member's own ranking
    items, scores = ref.group_topk(S, [2], [], 4, strategy)
    assert items.tolist() == [0, 2, 3, 1] and np.array_equal(scores, S[2][[0, 2, 3, 1]])


def test_header_binding_and_makefile_agree():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_recommend_group_slices', 'amar_recommend_group_f32'):
        assert re.search(r'\b' + sym + r'\s*\(', header) and sym in capi.SIGNATURES
    codes = {name: int(value) for name, value in re.findall(r'#define\s+AMAR_GROUP_(MEAN|MIN|MAX)\s+(\d+)', header)}
    assert codes == {'MEAN': 0, 'MIN': 1, 'MAX': 2}
    assert capi.GROUP_STRATEGIES == {name.lower(): code for name, code in codes.items()}
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=(.*)$', makefile, flags=re.M).group(1).split()
    assert 'amar_group.hip' in srcs
    lib = capi.load()
    assert hasattr(lib, 'amar_recommend_group_f32') and hasattr(lib, 'amar_recommend_group_slices')


def test_cpu_tensors_are_refused_not_computed():
    """The no-fallback rule: a call with host tensors raises AmarError instead of computing anything."""
    import torch
    from deep_cbrs_amar_renaissance_amd import capi
    w = [np.eye(16, dtype=np.float32), np.ones((16, 1), dtype=np.float32)]
    blob, _ = capi.chain_pack(w, [np.zeros(16, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    tu, ti = torch.zeros((4, 16)), torch.zeros((9, 16))
    ptr, users = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(capi.AmarError):
        capi.recommend_group(tu, ti, torch.from_numpy(blob), [16, 16, 1], ['relu', 'sigmoid'], 'relu', 3, ptr, users)
    with pytest.raises(ValueError):
        capi.recommend_group(tu, ti, torch.from_numpy(blob), [16, 16, 1], ['relu', 'sigmoid'], 'relu', 3, ptr, users, strategy='median')


def test_slice_count_looks_at_the_members():
    """amar_recommend_group_slices: a requested count is what amar_recommend_slices gives for as many queries; the automatic count
    never cuts finer when the same groups hold more members, and groups of one are cut like single users."""
    import ctypes
    from deep_cbrs_amar_renaissance_amd import capi
    lib = capi.load()
    dims = (ctypes.c_int32 * 3)(16, 16, 1)
    for n_items in (1, 17, 1100, 50000):
        for req in (1, 2, 5):
            assert lib.amar_recommend_group_slices(37, 90, n_items, dims, 2, req) == lib.amar_recommend_slices(37, n_items, dims, 2, req)
        assert lib.amar_recommend_group_slices(640, 640, n_items, dims, 2, 0) == lib.amar_recommend_slices(640, n_items, dims, 2, 0)
        auto = [lib.amar_recommend_group_slices(64, members, n_items, dims, 2, 0) for members in (64, 256, 1024, 8192)]
        assert all(a >= 1 for a in auto) and auto == sorted(auto), auto
    assert lib.amar_recommend_group_slices(-1, 0, 10, dims, 2, 0) == -1 and lib.amar_recommend_group_slices(4, -1, 10, dims, 2, 0) == -1
