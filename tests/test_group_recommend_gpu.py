"""GPU: group recommendation (`recommend_group()`, amar_recommend_group_f32) against the numpy reference of
tests/group_recommend_ref.py — the kernel on every template form, the selector's edges, the models' two routes and the opt-in
experiment surface (pytest -m gpu).

Every comparison is exact (np.array_equal on the items and on the scores' bits).  The members' scores S come bitwise from code
that group recommendation does not touch: capi.recommend over windows of at most 64 items (k = 64, no exclusion), or a model's own
recommend() over a catalogue of at most 64 items."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import group_recommend_ref as ref
from tests import helpers

pytestmark = pytest.mark.gpu

STRATEGIES = ('mean', 'min', 'max')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got_items, got_scores, want_items, want_scores):
    return np.array_equal(np.asarray(got_items, dtype=np.int64), want_items) and np.array_equal(_bits(got_scores), _bits(want_scores))


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _score_matrix(capi, tu_d, ti_d, blob, dims, acts):
    """S [n_users, n_items]: every pair's score as amar_recommend_f32 returns it, gathered over windows of 64 items."""
    n_users, n_items = int(tu_d.shape[0]), int(ti_d.shape[0])
    S = np.full((n_users, n_items), np.nan, dtype=np.float32)
    for w in range(0, n_items, 64):
        it, sc = capi.recommend(tu_d, ti_d[w:w + 64], blob, dims, acts, 'relu', k=64)
        it, sc = it.cpu().numpy(), sc.cpu().numpy()
        r, c = np.nonzero(it >= 0)
        S[r, w + it[r, c]] = sc[r, c]
    assert not np.isnan(S).any()
    return S


def _csr(segments):
    ptr = np.cumsum([0] + [len(s) for s in segments])
    flat = np.array([i for s in segments for i in sorted(s)], dtype=np.int32)
    return ptr.astype(np.int32), flat


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items', [1, 17, 1100])
@pytest.mark.parametrize('c1,hidden', [(16, [16]), (32, [32, 40, 32]), (64, [64, 24]), (128, [128])])      # MAXT 1, 2, 4, 8
def test_kernel_against_reference(hip, c1, hidden, n_items):
    import torch
    capi = hip
    rng = np.random.default_rng(7000 * c1 + n_items + helpers.seed_offset())
    n_users = 37
    widths = [c1] + hidden
    layers = [(rng.normal(0, 1 / np.sqrt(a), size=(a, b)).astype(np.float32), rng.uniform(-0.1, 0.1, size=b).astype(np.float32))
              for a, b in zip(widths[:-1], widths[1:])]
    layers.append(((rng.normal(0, 4 / np.sqrt(widths[-1]), size=(widths[-1], 1))).astype(np.float32),
                   rng.uniform(-0.1, 0.1, size=1).astype(np.float32)))
    dims = widths + [1]
    acts = ['relu'] * (len(dims) - 2) + ['sigmoid']
    tu = rng.normal(0, 1, size=(n_users, c1)).astype(np.float32)
    ti = rng.normal(0, 1, size=(n_items, c1)).astype(np.float32)
    if n_items > 4:
        ti[n_items // 2] = ti[1]                          # duplicated rows: exact ties, ordered by item id
        ti[n_items - 1] = ti[1]
    blob, _ = capi.chain_pack([w for w, _ in layers], [b for _, b in layers])
    blob, tu_d, ti_d = torch.from_numpy(blob).cuda(), torch.from_numpy(tu).cuda(), torch.from_numpy(ti).cuda()
    S = _score_matrix(capi, tu_d, ti_d, blob, dims, acts)

    groups = [[4], [9], [3, 20], [1, 7, 30], [0, 5, 11, 19, 33], list(range(2, 34, 2)), list(range(n_users)), [],
              [3, 20], [4, 7, 20], [6, 8], [10, 12, 14]]
    assert len(groups[5]) == 16
    excl = [set(rng.choice(n_items, size=min(n_items, int(rng.integers(0, 40))), replace=False).tolist()) for _ in groups]
    excl[8] = set(excl[2])                                # the same members and segment: identical rows
    excl[10] = set(range(n_items))                        # nothing left
    excl[11] = set(range(3, n_items))                     # 3 items left (fewer than k for k >= 10)
    g_ptr, g_users = _csr(groups)
    e_ptr, e_items = _csr(excl)
    gp_d, gu_d, ep_d, ei_d = _dev(g_ptr), _dev(g_users), _dev(e_ptr), _dev(e_items)
    # the per-user exclusion CSR that gives users 4 and 9 the segments of the size-1 groups 0 and 1
    u_ptr, u_items = _csr([excl[0] if u == 4 else (excl[1] if u == 9 else set()) for u in range(n_users)])
    up_d, ui_d = _dev(u_ptr), _dev(u_items)
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    lib = capi.load()
    median = float(np.median(S).astype(np.float32))
    subset = rng.permutation(len(groups))[:7]
    sub_ptr, sub_users = _csr([groups[j] for j in subset])
    sub_eptr, sub_eitems = _csr([excl[j] for j in subset])

    def call(k, strategy, min_score=None, n_slices=0, **csr):
        a = dict(grp_ptr=gp_d, grp_users=gu_d, excl_ptr=ep_d, excl_items=ei_d)
        a.update(csr)
        i, s = capi.recommend_group(tu_d, ti_d, blob, dims, acts, 'relu', k, a['grp_ptr'], a['grp_users'], strategy=strategy,
                                    min_score=min_score, excl_ptr=a['excl_ptr'], excl_items=a['excl_items'], n_slices=n_slices)
        return i.cpu().numpy(), s.cpu().numpy()

    for k in (1, 10, 64):
        one_i, one_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k, users=_dev([4, 9]), excl_ptr=up_d, excl_items=ui_d)
        one_i, one_s = one_i.cpu().numpy(), one_s.cpu().numpy()
        for strategy in STRATEGIES:
            for min_score in (None, median, 2.0):
                got_i, got_s = call(k, strategy, min_score)
                want_i, want_s = ref.groups_topk(S, groups, excl, k, strategy, min_score)
                assert _same(got_i, got_s, want_i, want_s), (k, strategy, min_score)
                if min_score == 2.0:
                    assert (got_i == -1).all() and np.isneginf(got_s).all()
            got_i, got_s = call(k, strategy)
            assert np.array_equal(got_i[2], got_i[8]) and np.array_equal(_bits(got_s[2]), _bits(got_s[8]))
            assert (got_i[7] == -1).all() and (got_i[10] == -1).all() and (got_i[11] >= 0).sum() == min(k, 3, n_items)
            inf_i, inf_s = call(k, strategy, float('-inf'))                         # None is -inf
            assert _same(inf_i, inf_s, got_i, got_s)
            # a group of one is the member's own list, under every strategy
            assert np.array_equal(got_i[:2], one_i) and np.array_equal(_bits(got_s[:2]), _bits(one_s)), (k, strategy)
            # any item slicing gives the same bits
            for slices in (1, 2, 5):
                if lib.amar_recommend_group_slices(len(groups), len(g_users), n_items, dims_c, len(dims) - 1, slices) != slices:
                    continue
                s_i, s_s = call(k, strategy, n_slices=slices)
                assert _same(s_i, s_s, got_i, got_s), (k, strategy, slices)
            # a shuffled subset of the groups: bitwise the rows of the full call
            sub_i, sub_s = call(k, strategy, grp_ptr=_dev(sub_ptr), grp_users=_dev(sub_users), excl_ptr=_dev(sub_eptr),
                                excl_items=_dev(sub_eitems))
            assert _same(sub_i, sub_s, got_i[subset], got_s[subset]), (k, strategy)
        # exclusion off: every item ranks
        all_i, _ = call(k, 'mean', excl_ptr=None, excl_items=None)
        assert (all_i[10] >= 0).sum() == min(k, n_items)
    # no groups: nothing is launched
    none_i, none_s = capi.recommend_group(tu_d, ti_d, blob, dims, acts, 'relu', 5, _dev([0]), _dev([]))
    assert tuple(none_i.shape) == (0, 5) and tuple(none_s.shape) == (0, 5)


def test_refusals(hip):
    import torch
    capi = hip
    blob, _ = capi.chain_pack([np.eye(16, dtype=np.float32), np.ones((16, 1), dtype=np.float32)],
                              [np.zeros(16, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    blob = torch.from_numpy(blob).cuda()
    tu, ti = torch.zeros((4, 16), device='cuda'), torch.zeros((9, 16), device='cuda')
    ptr, users = _dev([0, 2]), _dev([0, 1])
    args = (tu, ti, blob, [16, 16, 1], ['relu', 'sigmoid'], 'relu')
    with pytest.raises(ValueError):
        capi.recommend_group(*args, 3, ptr, users, min_score=float('nan'))
    with pytest.raises(ValueError):
        capi.recommend_group(*args, 0, ptr, users)
    with pytest.raises(capi.AmarError):
        capi.recommend_group(*args, 65, ptr, users)
    with pytest.raises(ValueError):
        capi.recommend_group(*args, 3, ptr, users, excl_ptr=_dev([0, 0, 0]), excl_items=_dev([]))


# ---- 2. the selector's edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 63, 64])
def test_selector_adversarial_orders(hip, k):
    """The selection case of the single-user ranker (197 items, 19 queries, exclusions on group and tile edges, scores ascending and
    reversed) with a group of two per query: member 2q has Tu = 0, member 2q + 1 shifts feature 0 by 0.5, through an identity
    Dense(16, relu) and Dense(1, sigmoid) on feature 0.  The second member scores every item higher and both are monotone in the
    item's value, so 'min' and 'max' lists are known in closed form; all three are held against the reference on S."""
    import torch
    capi = hip
    n, m, c1, shift = helpers.SELECT_ROWS, helpers.SELECT_QUERIES, 16, np.float32(0.5)
    excl = helpers.select_case_exclusions(k, tile_rows=256)                              # c1 = 16 stages 256-item tiles
    e_ptr, e_items = _csr([excl[q] for q in range(m)])
    groups = [[2 * q, 2 * q + 1] for q in range(m)]
    g_ptr, g_users = _csr(groups)
    dot = np.zeros((c1, 1), dtype=np.float32)
    dot[0, 0] = 1.0
    blob, _ = capi.chain_pack([np.eye(c1, dtype=np.float32), dot], [np.zeros(c1, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    blob, dims, acts = torch.from_numpy(blob).cuda(), [c1, c1, 1], ['relu', 'sigmoid']
    tu = np.zeros((2 * m, c1), dtype=np.float32)
    tu[1::2, 0] = shift
    tu_d = torch.from_numpy(tu).cuda()
    dims_c = (ctypes.c_int32 * 3)(*dims)
    for reverse in (False, True):
        value = np.arange(n)[::-1] if reverse else np.arange(n)                          # item i has feature 0 = value[i] / 197
        ti = np.zeros((n, c1), dtype=np.float32)
        ti[:, 0] = value / np.float32(n)
        ti_d = torch.from_numpy(ti).cuda()
        S = _score_matrix(capi, tu_d, ti_d, blob, dims, acts)
        want_i = helpers.select_case_expected(excl, k, np.argsort(-value, kind='stable').tolist())
        x = ti[np.maximum(want_i, 0), 0]
        closed = {'min': 1.0 / (1.0 + np.exp(-x.astype(np.float64))), 'max': 1.0 / (1.0 + np.exp(-(x + shift).astype(np.float64)))}
        for strategy in STRATEGIES:
            ref_i, ref_s = ref.groups_topk(S, groups, [excl[q] for q in range(m)], k, strategy)
            for slices in (1, 2, 3):
                if capi.load().amar_recommend_group_slices(m, 2 * m, n, dims_c, 2, slices) != slices:
                    continue
                got_i, got_s = capi.recommend_group(tu_d, ti_d, blob, dims, acts, 'relu', k, _dev(g_ptr), _dev(g_users), strategy=strategy,
                                                    excl_ptr=_dev(e_ptr), excl_items=_dev(e_items), n_slices=slices)
                got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
                assert _same(got_i, got_s, ref_i, ref_s), (k, reverse, strategy, slices)
                if strategy in closed:
                    assert np.array_equal(got_i, want_i), (k, reverse, strategy, slices)
                    assert np.array_equal(np.isneginf(got_s), want_i < 0)
                    assert np.abs(got_s[want_i >= 0] - closed[strategy][want_i >= 0]).max() <= 1e-6


# ---- 3. the models ---------------------------------------------------------------------------------------------------------------
class _Train:
    """The parts of a training Sequence recommend() reads."""

    def __init__(self, ratings, n_users, n_items, **tables):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)
        self.__dict__.update(tables)


def _model_case(name):
    import torch
    from deep_cbrs_amar_renaissance_amd.data.datasets import HybridUserItemEmbeddings, UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    set_seed(21)
    g = helpers.tiny_graph(n_users=40, n_items=60, n_ratings=500, seed=14)
    nu, ni = g['n_users'], g['n_items']
    rng = np.random.default_rng(8)
    if name == 'BasicGCN':
        model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48])
        train, route = _Train(g['ratings'], nu, ni), 'fused'
    elif name == 'BasicRS':
        model = basic.BasicRS(dense_units=[512, 256, 128], clf_units=[64, 64])      # the basic-kge head: fused through _rank_plan
        model.build_head(32, 32)
        train = UserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 32)).astype(np.float32))
        route = 'fused'
    elif name == 'HybridCBRS':
        model = hybrid.HybridCBRS(feature_based=False, dense_units=[[32, 16], [64, 16], [32, 8]], clf_units=[16])
        model.build_head(16, 40)
        train = HybridUserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 16)).astype(np.float32),
                                         rng.normal(0, 1, size=(nu + ni, 40)).astype(np.float32))
        route = 'pairs'
    else:
        model = hybrid.HybridBertGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [32, 16], [16, 16]],
                                     clf_units=[16, 16], feature_based=True, fusion_method='concatenate')
        model.set_bert_table(rng.normal(0, 1, size=(nu + ni, 48)).astype(np.float32))
        model.rs.build_head(model.gnn.output_dim(), 48)
        train, route = _Train(g['ratings'], nu, ni), 'pairs'
    helpers.randomize_biases(model, seed=2)
    with torch.no_grad():
        (model.rs if hasattr(model, 'rs') else model).clf.layers[-1].kernel.mul_(10.0)
    return model, train, g, route


@pytest.mark.parametrize('name', ['BasicGCN', 'BasicRS', 'HybridCBRS', 'HybridBertGCN'])
def test_models_against_reference(hip, name, monkeypatch):
    capi = hip
    model, train, g, route = _model_case(name)
    nu, ni = g['n_users'], g['n_items']
    assert model._recommend_route(train) == route
    before = model.recommend(train, k=ni, exclude_seen=False)
    users, items, scores = before
    assert np.array_equal(users, np.arange(nu)) and (items >= nu).all()
    S = np.zeros((nu, ni), dtype=np.float32)
    S[users[:, None], items - nu] = scores
    seen = {u: set() for u in range(nu)}
    for u, i, _ in g['ratings'].tolist():
        seen[u].add(i - nu)
    groups = [[0], [5, 3], [7, 8, 9, 30], [], list(range(0, 40, 3)), [3, 5], list(range(nu))]
    union = [set().union(*[seen[u] for u in m]) if m else set() for m in groups]
    calls = {'fused': 0, 'pairs': 0}
    fused, topk = capi.recommend_group, capi.topk_segmented
    monkeypatch.setattr(capi, 'recommend_group', lambda *a, **kw: (calls.__setitem__('fused', calls['fused'] + 1), fused(*a, **kw))[1])
    monkeypatch.setattr(capi, 'topk_segmented', lambda *a, **kw: (calls.__setitem__('pairs', calls['pairs'] + 1), topk(*a, **kw))[1])
    median = float(np.median(S).astype(np.float32))
    for strategy in STRATEGIES:
        for k, min_score in ((10, None), (10, median), (60, None)):
            got_i, got_s, per = model.recommend_group(train, groups, k=k, strategy=strategy, min_score=min_score, member_scores=True)
            assert got_i.dtype == np.int64 and got_s.dtype == np.float32 and got_i.shape == (len(groups), k)
            want_i, want_s = ref.groups_topk(S, groups, union, k, strategy, min_score)
            rows = np.where(got_i >= 0, got_i - nu, -1)
            assert _same(rows, got_s, want_i, want_s), (name, strategy, k, min_score)
            for j, members in enumerate(groups):                             # nothing any member has rated comes back
                assert not (set(rows[j][rows[j] >= 0].tolist()) & union[j])
                ms = per[j]
                assert ms.dtype == np.float32 and ms.shape == (len(members), k)
                assert np.array_equal(np.isnan(ms), np.broadcast_to(rows[j] < 0, ms.shape))
                if members and (rows[j] >= 0).any():
                    v = rows[j] >= 0
                    agg = ref.aggregate(ms[:, v], range(len(members)), strategy)
                    assert np.array_equal(_bits(agg), _bits(got_s[j][v])), (name, strategy, j)
                    assert np.array_equal(_bits(ms[:, v]), _bits(S[sorted(members)][:, rows[j][v]]))
    # nine calls: the fused heads launch amar_recommend_group_f32 for the lists and once more for the member scores (7 groups: one
    # chunk) and rank no pairs; the others rank pairs, once per call — a head that silently fell back would show up here
    assert calls == ({'fused': 18, 'pairs': 0} if route == 'fused' else {'fused': 0, 'pairs': 9}), calls
    # exclude_seen=False ranks every item; the order a caller lists the members in does not matter
    a_i, a_s = model.recommend_group(train, [[30, 7, 9, 8]], k=60, exclude_seen=False)
    w_i, w_s = ref.groups_topk(S, [groups[2]], [set()], 60, 'mean')
    assert _same(a_i - nu, a_s, w_i, w_s)
    e_i, e_s = model.recommend_group(train, [], k=4)
    assert e_i.shape == (0, 4) and e_s.shape == (0, 4)
    for bad in (dict(groups=[[0, 0]]), dict(groups=[[nu]]), dict(groups=[[0]], strategy='median'), dict(groups=[[0]], k=65),
                dict(groups=[[0]], min_score=float('nan'))):
        with pytest.raises(ValueError):
            model.recommend_group(train, **bad)
    # no side effects: recommend() returns the bits it returned before
    after = model.recommend(train, k=ni, exclude_seen=False)
    assert np.array_equal(before[1], after[1]) and np.array_equal(_bits(before[2]), _bits(after[2]))


# ---- 4. the experiment surface -----------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, group_key, paths):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(paths)
    cfg['parameters']['epochs'] = 1
    if group_key:
        cfg['parameters']['group_recommend'] = group_key
    (tmp_path / (name + '.yaml')).write_text(yaml.safe_dump(cfg))
    (tmp_path / (name + '_exps.yaml')).write_text(
        "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
        "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
    run_log = setup_mlflow(name, str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / (name + '.yaml')), str(tmp_path / (name + '_exps.yaml')), run_log)
    assert all(v is not None for v in multi.run().values())
    runs = glob.glob(str(tmp_path / 'mlruns' / name / '*'))
    assert len(runs) == 1
    return runs[0]


def test_experiment_group_recommend_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    capture = {}
    original = experiment.Experimenter.write_group_recommend

    def spy(self, **kw):
        capture['exp'] = self
        return original(self, **kw)

    monkeypatch.setattr(experiment.Experimenter, 'write_group_recommend', spy)
    monkeypatch.chdir(tmp_path)
    spec = {'size': 3, 'count': 7, 'seed': 1}
    run_on = _run_experiment(tmp_path, 'with_key', {'k': 5, 'strategy': 'min', 'groups': spec}, paths)
    exp = capture.pop('exp')
    tsv = os.path.join(run_on, 'artifacts', 'predictions', 'group_top_5.tsv')
    top = pd.read_csv(tsv, sep='\t', header=None)
    assert top.shape == (35, 4)
    ids, members = exp.group_members(spec)
    assert ids == list(range(7)) and all(len(set(m.tolist())) == 3 for m in members)
    items, scores = exp.model.recommend_group(exp.trainset, members, k=5, strategy='min')
    assert (items >= 0).all()
    assert top[0].tolist() == np.repeat(np.arange(7), 5).tolist() and top[1].tolist() == np.tile(np.arange(1, 6), 7).tolist()
    assert np.array_equal(top[2].to_numpy(), np.asarray(exp.trainset.items)[items.reshape(-1) - len(exp.trainset.users)])
    assert np.array_equal(_bits(top[3].to_numpy().astype(np.float32)), _bits(scores.reshape(-1)))
    run_off = _run_experiment(tmp_path, 'without_key', None, paths)
    assert 'exp' not in capture
    assert not glob.glob(os.path.join(run_off, '**', 'group_top_*'), recursive=True)
