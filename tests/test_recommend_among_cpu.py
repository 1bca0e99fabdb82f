"""Host side of recommendation among candidates (no GPU): `check_candidates` on every form it takes and every refusal,
`items_with_properties` against the loop restatement of tests/among_ref.py, the header / binding / library agreement on
amar_recommend_among_f32 and AMAR_RANK_AMONG, the route query's byte count and capacity for kind 'among', and the models' route
decision with the query monkeypatched."""
import os
import re

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from deep_cbrs_amar_renaissance_amd import recommend as rec
from tests import among_ref
from tests import helpers
from tests import rank_forms_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, NI = 5, 7


# ---- 1. check_candidates -------------------------------------------------------------------------------------------------------
def test_check_candidates_accepts_every_form():
    import torch
    want = np.array([0, 2, 6], dtype=np.int64)
    for ids in ([11, 5, 7, 5], (7, 11, 5), np.array([5, 7, 11], dtype=np.int32), torch.tensor([11, 7, 5]), range(5, 12, 2)):
        ids = [5, 7, 11] if isinstance(ids, range) else ids
        got = rec.check_candidates(ids, NU, NI)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)       # rows, sorted, distinct
    mask = np.zeros(NI, dtype=bool)
    mask[[0, 2, 6]] = True
    for m in (mask, mask.tolist(), torch.from_numpy(mask)):
        assert np.array_equal(rec.check_candidates(m, NU, NI), want)
    assert rec.check_candidates([], NU, NI).size == 0 and rec.check_candidates(np.zeros(NI, dtype=bool), NU, NI).size == 0
    assert np.array_equal(rec.check_candidates(np.ones(NI, dtype=bool), NU, NI), np.arange(NI))
    # per user: one sequence per listed user, ids or masks, empty ones allowed
    ptr, rows = rec.check_candidates([[11, 5], [], mask, np.array([6, 6, 6])], NU, NI, n_listed=4)
    assert ptr.tolist() == [0, 2, 2, 5, 6] and rows.tolist() == [0, 6, 0, 2, 6, 1] and ptr.dtype == rows.dtype == np.int64
    ptr, rows = rec.check_candidates(np.array([[5, 6], [6, 5], [7, 7]]), NU, NI, n_listed=3)
    assert ptr.tolist() == [0, 2, 4, 5] and rows.tolist() == [0, 1, 0, 1, 2]


@pytest.mark.parametrize('bad', [
    None, 'abc', 7, {5: 1},
    [5.0, 6.0], np.array([5.5]),                       # dtype
    [4], [12], [-1], [5, 12],                          # out of range: node ids are |U|..|U|+|I|-1
    np.zeros(NI - 1, dtype=bool), np.ones(NI + 1, dtype=bool), np.ones((2, NI + 1), dtype=bool),      # masks of the wrong length
    [[5, 6], [4]], [[5], [6.5]], [[5], 'ab'], [[[5]], [[6]]],
])
def test_check_candidates_refusals(bad):
    with pytest.raises(ValueError, match='candidates'):
        rec.check_candidates(bad, NU, NI, n_listed=2)


def test_check_candidates_per_user_length():
    with pytest.raises(ValueError, match='candidates.*3 users, 2 sequences'):
        rec.check_candidates([[5], [6]], NU, NI, n_listed=3)
    with pytest.raises(ValueError, match='candidates'):
        rec.check_candidates([[5]], NU, NI, n_listed=0)
    assert rec.check_candidates([[5], [6]], NU, NI, n_listed=2)[0].tolist() == [0, 1, 2]


def test_binding_checks_the_kernels_precondition():
    """capi.check_candidate_rows is what stands between Python and the kernel: ascending, distinct, in range."""
    assert capi.check_candidate_rows([0, 3, 4], 5).dtype == np.int32 and capi.check_candidate_rows([], 5).size == 0
    for bad in ([3, 1], [1, 1], [0, 5], [-1, 2], [0.5], [[0, 1]], [True, False]):
        with pytest.raises(ValueError, match='cand'):
            capi.check_candidate_rows(bad, 5)


# ---- 2. items_with_properties --------------------------------------------------------------------------------------------------
class _Train:
    def __init__(self, adj, n_users, n_items):
        self.adj_matrix, self.users, self.items = adj, np.arange(n_users), np.arange(n_items)


def _property_cases(kind):
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    g = helpers.tiny_graph(n_users=9, n_items=23, n_ratings=80, seed=4, n_props=6, n_links=40)
    triples = g['triples'].copy()
    # item 0 has exactly the properties 0, 1, 2; item 1 all of them but 2; item 2 none at all
    triples = triples[~np.isin(triples[:, 0], [0, 1, 2])]
    extra = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    triples = np.concatenate([triples, np.array([[i, p + 23, 1] for i, p in extra], dtype=np.int64)])
    adj = build_adjacency_matrix(g['ratings'], g['users'], g['items'], triples, g['props'], type_adjacency=kind)
    has = among_ref.item_properties(23, [(i, p - 23) for i, p, _ in triples.tolist()])
    return _Train(adj, 9, 23), has


@pytest.mark.parametrize('kind', ['unary-uip', 'unary-kg'])
def test_items_with_properties(kind):
    train, has = _property_cases(kind)
    assert isinstance(train.adj_matrix, (tuple, list)) == (kind == 'unary-kg')
    nu = 9
    rng = np.random.default_rng(2)
    cases = [dict(), dict(any_of=[0]), dict(all_of=[0, 1, 2]), dict(none_of=[0, 1, 2, 3, 4, 5]), dict(none_of=[3]), dict(any_of=[]),
             dict(all_of=[]), dict(none_of=[]), dict(any_of=[1, 1, 4]), dict(any_of=[0, 1], all_of=[2], none_of=[5]),
             dict(all_of=[0, 1, 2, 3, 4, 5], none_of=[0]), dict(any_of=np.array([5, 2]), none_of=(0,))]
    for _ in range(20):
        pick = lambda: None if rng.random() < 0.3 else rng.choice(6, size=int(rng.integers(0, 4)), replace=False).tolist()
        cases.append(dict(any_of=pick(), all_of=pick(), none_of=pick()))
    sizes = []
    for kw in cases:
        got = rec.items_with_properties(train, **kw)
        want = among_ref.items_with_properties(has, **kw)
        assert got.dtype == np.int64 and got.tolist() == [nu + r for r in want], kw
        sizes.append(len(want))
    assert rec.items_with_properties(train).tolist() == list(range(nu, nu + 23))                  # nothing constrains
    all3 = rec.items_with_properties(train, all_of=[0, 1, 2]).tolist()
    assert nu + 0 in all3 and nu + 1 not in all3                                                  # all but one is not all
    assert nu + 2 in rec.items_with_properties(train, none_of=[0, 1, 2, 3, 4, 5]).tolist()         # none_of alone
    assert rec.items_with_properties(train, any_of=[]).size == 0 and 0 in sizes and 23 in sizes   # empty results are results
    for bad in (dict(any_of=[6]), dict(all_of=[-1]), dict(none_of=[0.5]), dict(any_of=[[0]]), dict(any_of='01'), dict(all_of=3)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            rec.items_with_properties(train, **bad)


def test_items_with_properties_needs_properties():
    g = helpers.tiny_graph(n_users=9, n_items=23, n_ratings=80, seed=4)
    with pytest.raises(ValueError, match='properties'):
        rec.items_with_properties(_Train(g['adj'], 9, 23), any_of=[0])
    with pytest.raises(ValueError, match='properties'):
        rec.items_with_properties(_Train(None, 9, 23))


# ---- 3. header, binding, library -------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    decl = re.search(r'int amar_recommend_among_f32\((.*?)\);', header, re.S)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
    assert len(args) == len(capi.SIGNATURES['amar_recommend_among_f32'][1]) == 25
    assert args[16] == 'const int32_t *cand_items' and args[17] == 'int32_t n_cand' and args[-1] == 'amar_stream_t stream'
    assert int(re.search(r'#define\s+AMAR_RANK_AMONG\s+(\d+)', header).group(1)) == capi.RANK_KINDS['among']
    assert len(set(capi.RANK_KINDS.values())) == len(capi.RANK_KINDS)
    assert hasattr(capi.load(), 'amar_recommend_among_f32')                                       # the library exports the symbol
    names = list(capi.SIGNATURES)                                                                 # ... in the header's order
    at = [header.index(' ' + n + '(') for n in ('amar_recommend_group_f32', 'amar_recommend_among_f32', 'amar_nearest_slices')]
    assert at == sorted(at) and names.index('amar_recommend_group_f32') < names.index('amar_recommend_among_f32') < names.index('amar_nearest_slices')
    srcs = open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_rank_among.hip' in srcs


# ---- 4. the route query for kind 'among' -----------------------------------------------------------------------------------------
FOUR_FORMS = ([16, 16, 1], [32, 32, 1], [64, 64, 1], [128, 128, 1])        # MAXT 1, 2, 4, 8


def test_lds_sum_is_recommends_plus_the_id_array():
    seen = set()
    for dims in FOUR_FORMS + tuple(rf.dims_of(f) for f in rf.FORMS):
        a, r = capi.rank_route('among', dims), capi.rank_route('recommend', dims)
        assert a['lds_bytes'] == r['lds_bytes'] + 4 * r['tile_items'], dims
        assert {k: a[k] for k in a if k not in ('lds_bytes', 'fits', 'large_lds')} == {k: r[k] for k in r if k not in ('lds_bytes', 'fits', 'large_lds')}
        assert a['fits'] == (a['lds_bytes'] <= 160 * 1024) and a['large_lds'] == (a['lds_bytes'] > 64 * 1024)
        assert a['lds_bytes'] == rf.route('recommend', dims)[1]['lds_bytes'] + 4 * rf.route('recommend', dims)[1]['tile_items']
        seen.add(a['maxt'])
    assert seen == {1, 2, 4, 8} and [capi.rank_route('among', d)['maxt'] for d in FOUR_FORMS] == [1, 2, 4, 8]
    # the refusals of the query are those of its siblings
    for dims in ([16, 1], [18, 16, 1], [132, 16, 1], [16, 16, 4], [16, 0, 1], [16, 1, 16, 1], [16, 129, 1]):
        assert capi.rank_route('among', dims, code=True)['code'] == capi.rank_route('recommend', dims, code=True)['code'] != 0


def test_capacity_walk():
    """The largest head 'among' takes and the first it refuses sit on either side of 160 KB; the id array (192 B beside a 128-wide
    c1) costs the last hidden layer at most a unit or two against amar_recommend_f32."""
    ref_fits = lambda d: rf.route('recommend', d)[0] == 0 and \
        rf.route('recommend', d)[1]['lds_bytes'] + 4 * rf.route('recommend', d)[1]['tile_items'] <= rf.LDS_LIMIT
    largest, past = rf.capacity_heads(lambda d: capi.rank_fits('among', d))
    assert (largest, past) == rf.capacity_heads(ref_fits)
    a, b = capi.rank_route('among', largest), capi.rank_route('among', past)
    assert a['fits'] and a['large_lds'] and not b['fits'] and a['lds_bytes'] <= 160 * 1024 < b['lds_bytes']
    assert capi.chain_supported(past, 128, 128, sum_inputs=True)               # predict() scores it: the pair route must rank it
    rec_largest = rf.capacity_heads(lambda d: capi.rank_fits('recommend', d))[0]
    assert largest[:-2] == rec_largest[:-2] and 0 <= rec_largest[-2] - largest[-2] <= 2
    assert not capi.rank_fits('among', [128, 128, 128, 1]) and capi.rank_fits('among', [128, 128, 64, 1])


# ---- 5. the models' route decision -------------------------------------------------------------------------------------------------
def test_ranker_plan_asks_for_among(monkeypatch):
    from tests.test_rank_forms_cpu import _patched, _rs
    model = _rs([16, 16])
    asked = _patched(monkeypatch, {'recommend': True, 'among': False})
    assert model._ranker_plan(8, 8, 'among') == (None, False)                  # a refusal: the pair route
    plan, split = model._ranker_plan(8, 8, 'recommend')
    assert plan is not None and split
    assert asked == [('among', [16, 16, 1]), ('recommend', [16, 16, 1])]
    monkeypatch.undo()
    asked = _patched(monkeypatch, {'among': True})
    plan, split = model._ranker_plan(8, 8, 'among')
    assert plan is not None and split and plan['rest'][1] == [16, 16, 1] and asked == [('among', [16, 16, 1])]
    monkeypatch.undo()
    assert model._ranker_plan(8, 8, 'among')[0] is not None                    # the real query takes the small head
    assert _rs([128, 128, 128])._ranker_plan(8, 8, 'among') == (None, False)   # ... and refuses the one past every ranker


def test_recommend_among_routes(monkeypatch):
    """SimilarSearch.recommend_among: one candidate set goes where _group_route(kind='among') says; per-user candidates go to the
    model's pair route without asking; the arguments are checked before any route is asked."""
    calls = []

    class Model(rec.SimilarSearch):
        def _group_route(self, trainset, kind='group'):
            calls.append(('route', kind))
            return self.answer

        def _recommend_pairs(self, trainset, k=10, users=None, exclude_seen=True, towers=None, keep_items=None):
            calls.append(('model_pairs', k, users, exclude_seen, keep_items))
            return 'by the model'

    class Train:
        users, items, ratings = np.arange(NU), np.arange(NI), np.zeros((0, 3), dtype=np.int64)

    monkeypatch.setattr(rec, 'among_fused', lambda towers, plan, train, cand, k, users, excl: calls.append(('fused', towers, plan, cand.tolist(), k, users, excl)) or 'fused')
    monkeypatch.setattr(rec, 'pairs', lambda fn, train, k, users, excl, device=None, keep_items=None: calls.append(('pairs', fn, k, users, excl, device, keep_items.tolist())) or 'pairs')
    model = Model()
    model.answer = ('fused', 'towers', 'plan')
    assert model.recommend_among(Train(), [6, 5], k=3, users=[1, 0]) == 'fused'
    assert calls == [('route', 'among'), ('fused', 'towers', 'plan', [0, 1], 3, [1, 0], True)]
    del calls[:]
    model.answer = ('pairs', 'score_fn', 'dev')
    assert model.recommend_among(Train(), [6, 5], k=3, exclude_seen=False) == 'pairs'
    assert calls == [('route', 'among'), ('pairs', 'score_fn', 3, None, False, 'dev', [0, 1])]
    del calls[:]
    model.answer = ('fused', 'towers', 'plan')
    assert model.recommend_among(Train(), [[6], [5, 7]], k=2, users=[4, 4]) == 'by the model'
    assert len(calls) == 1 and calls[0][:4] == ('model_pairs', 2, [4, 4], True)
    assert calls[0][4][0].tolist() == [0, 1, 3] and calls[0][4][1].tolist() == [1, 0, 2]
    del calls[:]
    for bad in (dict(candidates=[4]), dict(candidates=[5], k=65), dict(candidates=[5], users=[NU]), dict(candidates=[[5]], users=[0, 1])):
        with pytest.raises(ValueError):
            model.recommend_among(Train(), **bad)
    assert calls == []
    u, i, s = model.recommend_among(Train(), [5], k=4, users=[])
    assert u.shape == (0,) and i.shape == (0, 4) and s.shape == (0, 4) and calls == []
