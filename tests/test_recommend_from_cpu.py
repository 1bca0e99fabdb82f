"""Host side of recommendation from per-user candidate lists (no GPU): `check_candidate_lists` on every form it takes and every
refusal, the device normalisation `device_candidate_csr` (run on the CPU: it is plain torch) against the host one, the binding's
`check_candidate_lists`, `utilities.metrics.sampled_negatives`, the header / binding / library agreement on
amar_recommend_lists_f32 and AMAR_RANK_LISTS, the route query's byte count for kind 'lists', and the mixin's route decision."""
import ctypes
import os
import re

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd import recommend as rec
from deep_cbrs_amar_renaissance_amd.utilities import metrics
from tests import rank_forms_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, NI = 5, 7


# ---- 1. the candidate normalisation ------------------------------------------------------------------------------------------------
def test_candidate_lists_accept_every_form():
    import torch
    want_ptr, want_rows = [0, 2, 2, 3, 6], [0, 6, 1, 0, 3, 4]
    padded = np.array([[11, 5, -1, -1], [-1, -1, -1, -1], [6, 6, -1, 6], [9, 8, 5, 9]])
    forms = ([[11, 5], [], [6, 6, 6], [9, 8, 5, 9]],                          # sequences: any order, duplicates collapse
             [np.array([5, 11]), np.zeros(0, dtype=np.int64), (6,), torch.tensor([5, 8, 9])],
             padded, padded.astype(np.int32), padded[:, ::-1], torch.from_numpy(padded))
    for c in forms:
        ptr, rows = rec.check_candidate_lists(c, NU, NI, 4)
        assert ptr.dtype == rows.dtype == np.int64 and ptr.tolist() == want_ptr and rows.tolist() == want_rows
    mask = np.zeros(NI, dtype=bool)
    mask[[0, 6]] = True
    ptr, rows = rec.check_candidate_lists([mask, [6]], NU, NI, 2)             # a mask per user, as check_candidates takes it
    assert ptr.tolist() == [0, 2, 3] and rows.tolist() == [0, 6, 1]
    ptr, rows = rec.check_candidate_lists([], NU, NI, 0)
    assert ptr.tolist() == [0] and rows.size == 0
    ptr, rows = rec.check_candidate_lists(np.zeros((3, 0), dtype=np.int64), NU, NI, 3)
    assert ptr.tolist() == [0, 0, 0, 0] and rows.size == 0


@pytest.mark.parametrize('bad', [
    None, 'abc', 7, {5: 1},
    [5, 6], np.array([5, 6]), [],                      # one flat set: recommend_among's
    [[5.0], [6.0]], np.array([[5.5], [6.5]]),          # dtype
    [[4], [5]], [[5], [12]], np.array([[5, -2], [6, -1]]), np.array([[5, 12], [6, -1]]),       # out of range; only -1 pads
    [[5], 'ab'], [[[5]], [[6]]],
    [[5]], [[5], [6], [7]], np.array([[5], [6], [7]]),                        # not one list per listed user
])
def test_candidate_lists_refusals(bad):
    with pytest.raises(ValueError, match='candidates'):
        rec.check_candidate_lists(bad, NU, NI, 2)


def test_candidate_lists_tensor_refusals():
    import torch
    for bad in (torch.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.bool), torch.zeros((3, 3), dtype=torch.int64)):
        with pytest.raises(ValueError, match='candidates'):
            rec.check_candidate_lists(bad, NU, NI, 2)
    with pytest.raises(ValueError, match='candidates.*2 users, 3 sequences'):
        rec.check_candidate_lists(torch.zeros((3, 3), dtype=torch.int64), NU, NI, 2)


def test_device_normalisation_is_the_host_one():
    """device_candidate_csr is plain torch, so it runs here on CPU tensors: sorted, distinct, compacted, and what is no item node id
    (the -1 padding, a user's id, an id past the items) is no candidate."""
    import torch
    rng = np.random.default_rng(4)
    nu, ni = 9, 40
    for m, P in ((1, 1), (3, 5), (17, 64), (6, 0), (0, 4)):
        x = rng.integers(nu, nu + ni, size=(m, P))
        x[rng.random((m, P)) < 0.3] = -1
        if m > 2:
            x[1] = -1                                                         # an empty list in the middle
            x[2] = x[2, 0] if P else -1                                       # one item P times
        ptr, rows = rec.device_candidate_csr(torch.from_numpy(x), nu, ni)
        want_ptr, want_rows = rec.check_candidate_lists(x, nu, ni, m)
        assert ptr.dtype == rows.dtype == torch.int32 and ptr.tolist() == want_ptr.tolist()
        assert rows[:int(ptr[-1])].tolist() == want_rows.tolist()
        capi.check_candidate_lists(ptr.numpy(), rows[:int(ptr[-1])].numpy(), m, ni)              # the kernel's contract
    junk = torch.tensor([[nu - 1, nu + ni, -7, nu + 3, nu + 3, 2 ** 40]])
    ptr, rows = rec.device_candidate_csr(junk, nu, ni)
    assert ptr.tolist() == [0, 1] and rows[:1].tolist() == [3]


def test_binding_checks_the_kernels_precondition():
    ptr, rows = capi.check_candidate_lists([0, 2, 2, 3, 6], [0, 6, 1, 0, 3, 4], 4, NI)
    assert ptr.dtype == rows.dtype == np.int32 and ptr.tolist() == [0, 2, 2, 3, 6] and rows.tolist() == [0, 6, 1, 0, 3, 4]
    assert capi.check_candidate_lists([0], [], 0, NI)[1].size == 0
    assert capi.check_candidate_lists([0, 1, 2], [3, 3], 2, NI)[1].tolist() == [3, 3]              # equal across a boundary: two lists
    for bad_ptr, bad_rows, m in (([0, 2], [3, 1], 1), ([0, 2], [1, 1], 1), ([0, 1], [NI], 1), ([0, 1], [-1], 1), ([0, 1], [0.5], 1),
                                 ([0, 2], [0, 1], 2), ([1, 2], [0, 1], 1), ([0, 3], [0, 1], 1), ([0, 2, 1, 2], [0, 1], 3),
                                 ([0, 3, 3], [0, 2, 1], 2), ([[0, 1]], [0], 1), ([0, 1], [True], 1)):
        with pytest.raises(ValueError, match='cand'):
            capi.check_candidate_lists(bad_ptr, bad_rows, m, NI)


# ---- 2. sampled_negatives ----------------------------------------------------------------------------------------------------------
class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _split(seed, n_users=30, n_items=50):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n_users, 600), rng.integers(0, n_items, 600)], 1), axis=0)
    rng.shuffle(pairs)
    r = np.concatenate([pairs[:, :1], pairs[:, 1:] + n_users, rng.integers(0, 2, (len(pairs), 1))], 1).astype(np.int64)
    cut = len(r) * 3 // 4
    train, test = r[:cut], r[cut:]
    test = test[test[:, 0] != 7]                                              # user 7 has no held-out pair at all
    test[test[:, 0] == 8, 2] = 0                                              # user 8 none that is positive
    return _Train(train, n_users, n_items), test


def test_sampled_negatives():
    train, test = _split(1)
    nu, ni = 30, 50
    users, lists = metrics.sampled_negatives(train, test, 9, seed=3)
    assert users.dtype == lists.dtype == np.int64 and (np.diff(users) > 0).all() and lists.shape[0] == len(users)
    positives = {u: set(test[(test[:, 0] == u) & (test[:, 2] == 1), 1].tolist()) for u in range(nu)}
    rated = {u: set(train.ratings[train.ratings[:, 0] == u, 1].tolist()) | set(test[test[:, 0] == u, 1].tolist()) for u in range(nu)}
    assert users.tolist() == [u for u in range(nu) if positives[u]] and 7 not in users and 8 not in users
    for u, row in zip(users.tolist(), lists):
        row = row[row >= 0]
        assert len(set(row.tolist())) == len(row) and ((row >= nu) & (row < nu + ni)).all()
        drawn = set(row.tolist()) - positives[u]
        assert positives[u] <= set(row.tolist()) and not drawn & rated[u]     # never a rated item, whatever its label or split
        assert len(drawn) == min(9, ni - len(rated[u])) == len(row) - len(positives[u])
    assert (lists[:, -1] == -1).any() or len({len(positives[u]) for u in users.tolist()}) == 1
    # seed-stable, and the seed matters
    again = metrics.sampled_negatives(train, test, 9, seed=3)
    assert np.array_equal(again[0], users) and np.array_equal(again[1], lists)
    assert not np.array_equal(metrics.sampled_negatives(train, test, 9, seed=4)[1], lists)
    # a user's draw does not depend on the other users: drop half of them from both splits
    half = users[::2]
    sub_train = _Train(train.ratings[np.isin(train.ratings[:, 0], half)], nu, ni)
    sub_users, sub_lists = metrics.sampled_negatives(sub_train, test[np.isin(test[:, 0], half)], 9, seed=3)
    assert np.array_equal(sub_users, half)
    for u, row in zip(sub_users.tolist(), sub_lists):
        assert np.array_equal(row[row >= 0], lists[users == u][0][lists[users == u][0] >= 0])
    # fewer free items than asked for: all of them, and more negatives change nothing
    everything = metrics.sampled_negatives(train, test, ni, seed=3)
    for u, row in zip(everything[0].tolist(), everything[1]):
        assert set(row[row >= 0].tolist()) == positives[u] | (set(range(nu, nu + ni)) - rated[u])
    assert np.array_equal(metrics.sampled_negatives(train, test, 10 * ni, seed=8)[1], everything[1])
    none = metrics.sampled_negatives(train, test, 0, seed=3)
    assert all(set(row[row >= 0].tolist()) == positives[u] for u, row in zip(none[0].tolist(), none[1]))
    empty = metrics.sampled_negatives(train, np.zeros((0, 3), dtype=np.int64), 9)
    assert empty[0].shape == (0,) and empty[1].shape[0] == 0
    for bad in (dict(n_negatives=-1), dict(n_negatives=2.5), dict(n_negatives=True), dict(n_negatives=3, seed=-1), dict(n_negatives=3, seed='a')):
        with pytest.raises(ValueError):
            metrics.sampled_negatives(train, test, **bad)


# ---- 3. header, binding, library ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    declared = lambda sym: [a.strip() for a in re.search(r'int ' + sym + r'\((.*?)\);', header, re.S).group(1).replace('\n', ' ').split(',')]
    args = declared('amar_recommend_lists_f32')
    assert len(args) == len(capi.SIGNATURES['amar_recommend_lists_f32'][1]) == 22
    assert args[:16] == declared('amar_recommend_f32')[:16]                   # the head, users and the exclusion CSR of every ranker
    assert args[16:] == ['const int32_t *cand_ptr', 'const int32_t *cand_items', 'int32_t k', 'int32_t *out_items', 'float *out_scores',
                         'amar_stream_t stream']
    assert capi.SIGNATURES['amar_recommend_lists_f32'][1][:16] == capi.SIGNATURES['amar_recommend_f32'][1][:16]
    assert int(re.search(r'#define\s+AMAR_RANK_LISTS\s+(\d+)', header).group(1)) == capi.RANK_KINDS['lists'] == 5
    assert 3 not in capi.RANK_KINDS.values() and len(set(capi.RANK_KINDS.values())) == len(capi.RANK_KINDS)
    for name, value in capi.RANK_KINDS.items():
        assert int(re.search(r'#define\s+AMAR_RANK_{}\s+(\d+)'.format(name.upper()), header).group(1)) == value
    lib = capi.load()
    assert hasattr(lib, 'amar_recommend_lists_f32') and lib.amar_recommend_lists_f32.argtypes == capi.SIGNATURES['amar_recommend_lists_f32'][1]
    names = list(capi.SIGNATURES)                                             # ... in the header's order
    order = ('amar_recommend_among_f32', 'amar_recommend_lists_f32', 'amar_recommend_after_f32')
    at = [header.index(' ' + n + '(') for n in order]
    assert at == sorted(at) and [names.index(n) for n in order] == sorted(names.index(n) for n in order)
    makefile = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_rank_lists.hip' in re.search(r'^SRCS\s*=(.*)$', makefile, flags=re.M).group(1).split()
    doc = header[header.index('Top-k over PER-USER candidate lists'):header.index('int amar_recommend_lists_f32(')]
    for stated in ('strictly', 'bit for bit', 'only workgroup barrier', 'no slices', 'AMAR_RANK_LISTS'):
        assert stated in doc, stated


# ---- 4. the route query for kind 'lists' -------------------------------------------------------------------------------------------
def lists_lds_bytes(dims):
    """The formula of the issue, from the restated geometry: the stack, four gather buffers of 16 pt rows, four selectors of two
    64-entry lists, two 64-entry candidate buffers and four state words."""
    r = rf.route('recommend', dims)[1]
    return ((r['wpack_floats'] + 3) & ~3) * 4 + 4 * (16 * r['pt'] * r['tile_stride']) * 4 + 4 * (2 * 64 + 2 * 64 + 4) * 4


def test_lds_sum_has_no_item_tile():
    seen = set()
    for dims in [[16, 16, 1], [32, 32, 1], [64, 64, 1], [128, 128, 1]] + [rf.dims_of(f) for f in rf.FORMS]:
        a, r = capi.rank_route('lists', dims), capi.rank_route('recommend', dims)
        assert a['lds_bytes'] == lists_lds_bytes(dims), dims
        assert a['lds_bytes'] == r['lds_bytes'] - r['tile_items'] * r['tile_stride'] * 4 - rf.SELECT_BYTES + 4 * 16 * r['pt'] * r['tile_stride'] * 4 + 4160
        assert a['lds_bytes'] < r['lds_bytes']
        assert {k: a[k] for k in a if k not in ('lds_bytes', 'fits', 'large_lds')} == {k: r[k] for k in r if k not in ('lds_bytes', 'fits', 'large_lds')}
        assert a['fits'] == (a['lds_bytes'] <= 160 * 1024) and a['large_lds'] == (a['lds_bytes'] > 64 * 1024)
        seen.add(a['maxt'])
    assert seen == {1, 2, 4, 8}
    for dims in ([16, 1], [18, 16, 1], [132, 16, 1], [16, 16, 4], [16, 0, 1], [16, 1, 16, 1], [16, 129, 1]):
        assert capi.rank_route('lists', dims, code=True)['code'] == capi.rank_route('recommend', dims, code=True)['code'] != 0
    info = capi.RankRouteInfo()
    dims = (ctypes.c_int32 * 3)(16, 16, 1)
    assert capi.load().amar_rank_route(3, dims, 2, ctypes.byref(info)) == rf.EINVAL       # 3 stays unknown, 6 is not known yet
    assert capi.load().amar_rank_route(6, dims, 2, ctypes.byref(info)) == rf.EINVAL
    assert capi.load().amar_rank_route(5, dims, 2, ctypes.byref(info)) == 0 and info.lds_bytes == lists_lds_bytes([16, 16, 1])


def test_capacity_walk():
    """Without the tile 'lists' takes heads 'recommend' refuses; both walks end on either side of 160 KB."""
    ref_fits = lambda d: rf.route('recommend', d)[0] == 0 and lists_lds_bytes(d) <= rf.LDS_LIMIT
    largest, past = rf.capacity_heads(lambda d: capi.rank_fits('lists', d))
    assert (largest, past) == rf.capacity_heads(ref_fits)
    a, b = capi.rank_route('lists', largest), capi.rank_route('lists', past)
    assert a['fits'] and a['large_lds'] and not b['fits'] and a['lds_bytes'] <= 160 * 1024 < b['lds_bytes']
    assert not capi.rank_fits('recommend', largest)                           # ... and the largest one is such a head
    assert capi.chain_supported(past, 128, 128, sum_inputs=True)              # predict() scores it: the pair route must rank it
    assert not capi.rank_fits('lists', [128, 128, 128, 1])


# ---- 5. the mixin's route decision -------------------------------------------------------------------------------------------------
def test_ranker_plan_asks_for_lists(monkeypatch):
    from tests.test_rank_forms_cpu import _patched, _rs
    model = _rs([16, 16])
    asked = _patched(monkeypatch, {'recommend': True, 'lists': False})
    assert model._ranker_plan(8, 8, 'lists') == (None, False)
    assert model._ranker_plan(8, 8, 'recommend')[0] is not None
    assert asked == [('lists', [16, 16, 1]), ('recommend', [16, 16, 1])]
    monkeypatch.undo()
    assert model._ranker_plan(8, 8, 'lists')[0] is not None
    assert _rs([128, 128, 128])._ranker_plan(8, 8, 'lists') == (None, False)
    wide = _rs([128, 128, 112])                                               # a head only 'lists' has room for
    assert wide._ranker_plan(8, 8, 'recommend') == (None, False) and wide._ranker_plan(8, 8, 'lists')[0] is not None


def test_recommend_from_routes(monkeypatch):
    """SimilarSearch.recommend_from goes where _group_route(kind='lists') says, with the CSR of its lists; the arguments are checked
    before any route is asked."""
    calls = []

    class Model(rec.SimilarSearch):
        def _group_route(self, trainset, kind='group'):
            calls.append(('route', kind))
            return self.answer

    class Train:
        users, items, ratings = np.arange(NU), np.arange(NI), np.zeros((0, 3), dtype=np.int64)

    csr = lambda c: (c[0].tolist(), c[1].tolist())
    monkeypatch.setattr(rec, 'lists_fused', lambda towers, plan, train, lists, k, users, excl: calls.append(('fused', towers, plan, csr(lists), k, users, excl)) or 'fused')
    monkeypatch.setattr(rec, 'pairs', lambda fn, train, k, users, excl, device=None, keep_items=None: calls.append(('pairs', fn, k, users, excl, device, csr(keep_items))) or 'pairs')
    model = Model()
    model.answer = ('fused', 'towers', 'plan')
    assert model.recommend_from(Train(), [[6, 5], [11]], k=3, users=[1, 0]) == 'fused'
    assert calls == [('route', 'lists'), ('fused', 'towers', 'plan', ([0, 2, 3], [0, 1, 6]), 3, [1, 0], True)]
    del calls[:]
    model.answer = ('pairs', 'score_fn', 'dev')
    assert model.recommend_from(Train(), np.array([[6, 5], [11, -1]]), k=3, users=[4, 4], exclude_seen=False) == 'pairs'
    assert calls == [('route', 'lists'), ('pairs', 'score_fn', 3, [4, 4], False, 'dev', ([0, 2, 3], [0, 1, 6]))]
    del calls[:]
    for bad in (dict(candidates=[[4]] * NU), dict(candidates=[[5]] * NU, k=65), dict(candidates=[[5]], users=[NU]), dict(candidates=[[5]], users=[0, 1]),
                dict(candidates=[5, 6, 7, 8, 9])):
        with pytest.raises(ValueError):
            model.recommend_from(Train(), **bad)
    assert calls == []
    u, i, s = model.recommend_from(Train(), [], k=4, users=[])
    assert u.shape == (0,) and i.shape == (0, 4) and s.shape == (0, 4) and calls == []
