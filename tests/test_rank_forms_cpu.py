"""Host side of the fused rankers' form tests (no GPU): amar_rank_route against the Python restatement of tests/rank_forms_ref.py,
the models' per-kernel route decisions with the query monkeypatched, and the condition that keeps the GPU value check honest —
the float32 and the float64 restatement agree on every exactly-zero score of the grid at the sizes the GPU tests use."""
import ctypes

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from tests import helpers
from tests import rank_forms_ref as rf

KINDS = ('recommend', 'group', 'rank_of')
FIELDS = ('maxt', 'pt', 'tile_items', 'tile_stride', 'wpack_floats', 'lds_bytes', 'fits', 'large_lds')


def _query(kind, dims):
    got = capi.rank_route(kind, dims, code=True)
    return got.pop('code'), got


def _agree(kind, dims):
    code, want = rf.route(kind, dims)
    got_code, got = _query(kind, dims)
    assert got_code == code, (kind, dims, got_code, code)
    if code == 0:
        assert got == want, (kind, dims, got, want)
        assert sorted(got) == sorted(FIELDS)
    else:
        assert not any(got.values()), (kind, dims, got)                  # a refusal leaves the struct zeroed


# ---- 1. the route query --------------------------------------------------------------------------------------------------------
def test_grid_is_what_the_issue_asks_for():
    names = rf.FORM_NAMES
    assert len(set(names)) == len(names) and 18 <= len(names) <= 24 and all(f.what for f in rf.FORMS)
    c1s = {f.c1 for f in rf.FORMS}
    assert {4, 20, 36, 48, 52, 100, 124} <= c1s
    assert {2, 3, 17, 33, 65, 127} <= {w for f in rf.FORMS for w in f.hidden}
    assert any(f.c1 == 4 and f.hidden == [128] for f in rf.FORMS) and any(f.c1 == 128 and f.hidden == [2] for f in rf.FORMS)
    assert any(len(f.hidden) == rf.RANK_MAX_LAYERS and set(f.hidden) == {16} for f in rf.FORMS)
    assert {f.in_act for f in rf.FORMS} == {None, 'relu', 'sigmoid'} == {f.dot_act for f in rf.FORMS}
    assert any('sigmoid' in f.acts and any(w % 16 for w in f.hidden) for f in rf.FORMS)
    assert any(f.dot_act == 'relu' and f.dot_bias for f in rf.FORMS)
    assert {f.ld for f in rf.FORMS} == {'c1', '+4', 'x2'}


@pytest.mark.parametrize('kind', KINDS)
def test_route_query_on_the_form_grid(kind):
    for form in rf.FORMS:
        _agree(kind, rf.dims_of(form))
    heads = {tuple(rf.dims_of(f)): _query(kind, rf.dims_of(f))[1] for f in rf.FORMS}
    assert {r['maxt'] for r in heads.values()} == {1, 2, 4, 8}               # every kernel form is in the grid
    assert all(r['fits'] for r in heads.values())
    assert heads[(4, 128, 1)]['maxt'] == 8 and heads[(4, 128, 1)]['tile_stride'] == 20 and heads[(4, 128, 1)]['tile_items'] == 256
    assert heads[(128, 2, 1)]['tile_stride'] == 132 and heads[(128, 2, 1)]['tile_items'] == 48
    assert max(max(rf.item_counts(r)) for r in heads.values()) <= 330


@pytest.mark.parametrize('kind', KINDS)
def test_route_query_on_random_heads(kind):
    rng = np.random.default_rng(5 + helpers.seed_offset())
    seen = set()
    for _ in range(400):
        n_hidden = int(rng.integers(1, rf.RANK_MAX_LAYERS + 1))
        dims = [int(rng.integers(1, 33)) * 4] + [int(rng.integers(2, 129)) for _ in range(n_hidden)] + [1]
        _agree(kind, dims)
        seen.add(_query(kind, dims)[1]['fits'])
    assert seen == {True, False}


def test_route_refusals():
    lib = capi.load()
    info = capi.RankRouteInfo()
    dims = (ctypes.c_int32 * 3)(16, 16, 1)
    assert lib.amar_rank_route(0, None, 2, ctypes.byref(info)) == rf.EINVAL and lib.amar_rank_route(0, dims, 2, None) == rf.EINVAL
    assert lib.amar_rank_route(3, dims, 2, ctypes.byref(info)) == rf.EINVAL and lib.amar_rank_route(-1, dims, 2, ctypes.byref(info)) == rf.EINVAL
    assert lib.amar_rank_route(0, dims, 2, ctypes.byref(info)) == 0 and info.fits == 1 and info.reserved == 0
    for kind in KINDS:
        for dims in ([16, 1], [16] + [16] * (rf.RANK_MAX_LAYERS + 1) + [1], [2, 16, 1], [18, 16, 1], [0, 16, 1], [132, 16, 1], [16, 16, 4],
                     [16, 0, 1], [16, -3, 16, 1], [16, 1, 16, 1], [16, 129, 1], [16, 16, 200, 1]):
            _agree(kind, dims)
    assert [_query('recommend', d)[0] for d in ([16, 1], [18, 16, 1], [132, 16, 1], [16, 16, 4], [16, 0, 1], [16, 1, 16, 1], [16, 129, 1])] \
        == [-2, -1, -2, -2, -1, -2, -2]
    with pytest.raises(capi.AmarError):
        capi.rank_route('recommend', [16, 129, 1])
    with pytest.raises(ValueError):
        capi.rank_route('recommend', [18, 16, 1])
    assert capi.rank_fits('recommend', [16, 16, 1]) and not capi.rank_fits('recommend', [16, 129, 1])


def test_worked_byte_counts():
    """The two heads of the capacity bug, to the byte: 128 -> 128 -> 128 -> 1 packs to 132 624 B, which amar_chain_f32 takes (<= 150 KB)
    and no ranker does; 128 -> 128 -> 64 -> 1 (99 344 B) fits recommend / group and not rank_of."""
    tile, select, gather, counters = 48 * 132 * 4, 16640, 4 * 16 * 132 * 4, 16 * 386 * 4
    assert (tile, gather, counters) == (25344, 33792, 24704)
    wide, narrow = [128, 128, 128, 1], [128, 128, 64, 1]
    for dims, stack in ((wide, 132624), (narrow, 99344)):
        assert 4 * capi.load().amar_chain_pack_floats((ctypes.c_int32 * 4)(*dims), 3) == stack
        assert capi.chain_supported(dims, 128, 128, sum_inputs=True)
        for kind in KINDS:
            r = capi.rank_route(kind, dims)
            assert 4 * r['wpack_floats'] == stack
            assert r['lds_bytes'] == stack + tile + (select if kind != 'rank_of' else gather + counters)
    assert capi.rank_route('recommend', wide)['lds_bytes'] == 174608 and not capi.rank_route('recommend', wide)['fits']
    assert capi.rank_route('recommend', narrow)['lds_bytes'] == 141328 and capi.rank_route('group', narrow)['fits']
    assert capi.rank_route('rank_of', narrow)['lds_bytes'] == 183184 and not capi.rank_route('rank_of', narrow)['fits']
    assert capi.rank_route('rank_of', [128, 128, 1])['lds_bytes'] == 150416 and capi.rank_route('rank_of', [128, 128, 1])['fits']


def test_capacity_walk():
    """The largest head each kernel takes and the first one past it, found by walking the query (the GPU file runs the one and has the
    other refused): the restatement walks to the same heads, and they sit on either side of 160 KB."""
    for kind in KINDS:
        largest, past = rf.capacity_heads(lambda d: capi.rank_fits(kind, d))
        assert (largest, past) == rf.capacity_heads(lambda d: rf.route(kind, d)[1]['fits'])
        a, b = capi.rank_route(kind, largest), capi.rank_route(kind, past)
        assert a['fits'] and a['large_lds'] and not b['fits'] and a['lds_bytes'] <= 160 * 1024 < b['lds_bytes']
        assert capi.chain_supported(past, 128, 128, sum_inputs=True)           # predict() scores it: the pair route must rank it
    assert rf.capacity_heads(lambda d: capi.rank_fits('recommend', d))[0] == [128, 128, 96, 1]
    assert rf.capacity_heads(lambda d: capi.rank_fits('rank_of', d))[0] == [128, 128, 16, 1]


def test_header_binding_and_docs_agree():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'amar_hip.h')).read()
    for name, value in capi.RANK_KINDS.items():
        assert int(re.search(r'#define\s+AMAR_RANK_{}\s+(\d+)'.format(name.upper()), header).group(1)) == value
    struct = re.search(r'typedef struct amar_rank_route_info \{(.*?)\} amar_rank_route_info;', header, re.S).group(1)
    fields = [n.strip() for line in struct.split(';') if line.strip() for n in line.strip().split(None, 1)[1].split(',')]
    assert fields == [n for n, _ in capi.RankRouteInfo._fields_]
    assert ctypes.sizeof(capi.RankRouteInfo) == 40


# ---- 2. the models' route decisions --------------------------------------------------------------------------------------------
def _rs(clf_units):
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(3)
    model = basic.BasicRS(dense_units=[32, 16], clf_units=clf_units)
    model.build_head(8, 8)
    return model


def _patched(monkeypatch, fits_by_kind):
    asked = []

    def fake(kind, dims, code=False):
        asked.append((kind, list(dims)))
        return {'fits': fits_by_kind[kind], 'code': 0}
    monkeypatch.setattr(capi, 'rank_route', fake)
    return asked


def test_route_decision_is_per_kernel(monkeypatch):
    """_ranker_plan is where every consumer decides (_recommend_split, _group_route, _recommend_route, rank_of_route through
    _group_route(kind='rank_of')): it asks the query for ITS kernel with the rest stack's widths and falls to the pair route on
    'does not fit'."""
    model = _rs([16, 16])
    asked = _patched(monkeypatch, {'recommend': True, 'group': False, 'rank_of': False})
    plan, split = model._ranker_plan(8, 8, 'recommend')
    assert plan is not None and split and plan['rest'][1] == [16, 16, 1]
    assert model._ranker_plan(8, 8, 'group') == (None, False) and model._ranker_plan(8, 8, 'rank_of') == (None, False)
    assert asked == [(k, [16, 16, 1]) for k in KINDS]
    # without a monkeypatch: the real query; a head without a classifier hidden layer has no plan and the query is not asked
    monkeypatch.undo()
    assert all(model._ranker_plan(8, 8, k)[0] is not None for k in KINDS)
    flat = _rs([16])
    asked = _patched(monkeypatch, {k: True for k in KINDS})
    assert all(flat._ranker_plan(8, 8, k) == (None, False) for k in KINDS) and asked == []


def test_capacity_heads_route_per_kernel():
    """The two heads of the bug through the real query: both have a split plan (predict() scores them through amar_chain_f32);
    128 -> 128 -> 128 -> 1 ranks by pairs everywhere, 128 -> 128 -> 64 -> 1 fused in recommend / group and by pairs in rank_of; the
    default head stays fused everywhere."""
    want = {(128, 128, 128): (False, False, False), (128, 128, 64): (True, True, False), (48, 48): (True, True, True)}
    for clf_units, fused in want.items():
        model = _rs(list(clf_units))
        assert model._split_plan(8, 8) is not None
        assert tuple(model._ranker_plan(8, 8, k)[0] is not None for k in KINDS) == fused, clf_units


def test_a_rest_stack_the_packer_cannot_pack_has_no_rank_plan():
    """The rankers take RANK_MAX_LAYERS MFMA layers plus the dot (nine layers); amar_chain_pack_f32 packs eight.  A classifier with
    nine layers after the first has no packed form, so it has no rank plan (it used to reach chain_pack and raise) and ranks by pairs."""
    assert rf.RANK_MAX_LAYERS + 1 == capi.CHAIN_MAX_LAYERS + 1
    assert capi.rank_route('recommend', [16] * 9 + [1])['fits']
    with pytest.raises(ValueError):
        capi.chain_pack([np.zeros((16, 16), np.float32)] * 8 + [np.zeros((16, 1), np.float32)], [np.zeros(16, np.float32)] * 8 + [np.zeros(1, np.float32)])
    deep, deepest = _rs([16] * 8), _rs([16] * 9)                              # 8 and 9 layers after the first
    assert deep._rank_plan() is not None and deep._rank_plan()['rest'][1] == [16] * 8 + [1]
    assert deepest._rank_plan() is None and deepest._split_plan(8, 8) is None
    assert all(deepest._ranker_plan(8, 8, k) == (None, False) for k in KINDS)


def test_consumers_pass_their_kind(monkeypatch):
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    import inspect
    for cls in (basic.BasicRS, basic.BasicGNN, hybrid.HybridCBRS, hybrid.HybridBertGNN, rec.SimilarSearch):
        assert inspect.signature(cls._group_route).parameters['kind'].default == 'group', cls.__name__
    assert inspect.signature(basic.BasicRS._recommend_split).parameters['kind'].default == 'recommend'
    seen = []

    class Model:
        def _group_route(self, trainset, kind='group'):
            seen.append(kind)
            raise KeyError('stop')
    with pytest.raises(KeyError):
        rec.rank_of_route(Model(), None, None, None, True)
    assert seen == ['rank_of']


# ---- 3. the condition that keeps the GPU value check honest --------------------------------------------------------------------
@pytest.mark.parametrize('name', rf.FORM_NAMES)
def test_float32_and_float64_agree_on_exact_zeros(name):
    """The GPU test bounds |kernel - float64| by 8 x the float32 restatement's error, and a relu dot makes 'exactly 0' part of the
    ranking.  For every form and every size of the GPU grid: the float32 restatement is finite, its zero set is the float64 one's,
    and no pre-activation of a relu dot lies within the bound of zero — so a kernel inside the bound has the same zero set, and the
    exact layer of the GPU test (order and counts on the kernel's own bits) needs no allowance."""
    form = rf.FORMS[rf.FORM_NAMES.index(name)]
    code, r = rf.route('recommend', rf.dims_of(form))
    assert code == 0
    for n_items in rf.item_counts(r):
        case = rf.build(form, n_items)
        args = (case['tu'], case['ti'], case['layers'], case['acts'], case['in_act'])
        s32, s64 = rf.scores(*args, np.float32), rf.scores(*args, np.float64)
        assert np.isfinite(s32).all() and np.isfinite(s64).all()
        assert np.array_equal(s32 == 0, s64 == 0), (name, n_items)
        tol = rf.bound(s32, s64)
        assert tol < 1e-4, (name, n_items, tol)
        if form.dot_act == 'relu':
            pre = rf.pre_scores(*args, np.float64)
            share = float((s64 == 0).mean())
            assert np.abs(pre).min() > tol and (n_items == 1 or 0.25 <= share <= 0.55), (name, n_items, share)
        if form.dot_act is None and n_items > 1:
            assert (s64 < 0).any() and (s64 > 0).any()
        if n_items > 4:                                                   # three items share one vector: exact ties on the GPU
            a, b, c = rf.TIE_ROWS(n_items)
            assert np.array_equal(case['ti'][a], case['ti'][b]) and np.array_equal(case['ti'][a], case['ti'][c])
