"""GPU: full-catalogue top-k (`recommend()`): the fused kernel against float64, the models' two routes against each other and the
oracle, invariance, and the opt-in experiment surface (pytest -m gpu)."""
import glob
import json
import os

import numpy as np
import pytest
import yaml

from oracle import models as om
from tests import helpers

pytestmark = pytest.mark.gpu

MAX_NEAR_TIE_USERS = 3          # users whose list may differ from the float64 ranking by a swap of near-tied items


class _Train:
    """The parts of a training Sequence recommend() reads."""

    def __init__(self, ratings, n_users, n_items, **tables):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)
        self.__dict__.update(tables)


# ---- host float64 restatement of the split head -------------------------------------------------------------------
def _rest64(x, layers, in_act='relu'):
    """score = sigmoid(dot(act(... act(in_act(x) W_0 + b_0) ...))) on float64; x = Tu[u] + Ti[i]."""
    x = np.maximum(x, 0.0) if in_act == 'relu' else x
    for w, b in layers[:-1]:
        x = np.maximum(x @ w.astype(np.float64) + b.astype(np.float64), 0.0)
    w, b = layers[-1]
    return 1.0 / (1.0 + np.exp(-(x @ w.astype(np.float64) + b.astype(np.float64))[..., 0]))


def _grid64(tu, ti, layers):
    return np.stack([_rest64(tu[u].astype(np.float64)[None, :] + ti.astype(np.float64), layers) for u in range(len(tu))])


def _check_lists(users, items, scores, want64, excl, k, n_users, label, score_tol=1e-6):
    """items: node ids (offset n_users) or item rows when n_users == 0.  Returns the number of users whose list differs from the
    float64 ranking (each one only by near-tied items)."""
    users, items, scores = np.asarray(users), np.asarray(items), np.asarray(scores)
    n_items = want64.shape[1]
    rows = np.where(items >= 0, items - n_users, -1)
    valid = rows >= 0
    picked = want64[users[:, None], np.maximum(rows, 0)]
    err = float(np.abs(scores[valid] - picked[valid]).max()) if valid.any() else 0.0
    assert err <= score_tol, "{}: scores {} from float64".format(label, err)
    tol = 2 * err + 1e-12
    differing = 0
    for r, u in enumerate(users.tolist()):
        ex = excl.get(u, set())
        avail = np.array([i for i in range(n_items) if i not in ex], dtype=np.int64)
        n_valid = min(k, len(avail))
        assert valid[r, :n_valid].all() and not valid[r, n_valid:].any(), "{}: user {} padding".format(label, u)
        assert np.all(np.isneginf(scores[r, n_valid:])), label
        got = rows[r, :n_valid]
        assert len(set(got.tolist())) == n_valid and not (set(got.tolist()) & ex), "{}: duplicate or excluded item".format(label)
        s = scores[r, :n_valid]
        assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (got[:-1] < got[1:]))), "{}: order".format(label)
        if n_valid == 0:
            continue
        sc = want64[u, avail]
        order = np.lexsort((avail, -sc))
        o_rows, o_s = avail[order], sc[order]
        assert np.abs(want64[u, got] - o_s[:n_valid]).max() <= tol, "{}: user {} differs beyond near-ties".format(label, u)
        gaps = -np.diff(o_s[:min(k + 1, len(o_s))])
        near = np.any((gaps > 0) & (gaps <= tol))
        if not near:
            assert np.array_equal(got, o_rows[:n_valid]), "{}: user {} without near-tie differs".format(label, u)
        elif not np.array_equal(got, o_rows[:n_valid]):
            differing += 1
    return differing


# ---- 1. the kernel against float64 ---------------------------------------------------------------------------------
HIDDEN = {1: lambda c1: [c1], 2: lambda c1: [c1, 24], 3: lambda c1: [c1, 40, c1]}


@pytest.mark.parametrize('n_items', [1, 17, 3191])
@pytest.mark.parametrize('c1,n_layers', [(16, 1), (16, 2), (32, 3), (32, 1), (64, 1), (64, 2), (128, 1)])
def test_kernel_against_float64(hip, c1, n_layers, n_items):
    import torch
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    rng = np.random.default_rng(1000 * c1 + 10 * n_layers + n_items + helpers.seed_offset())
    n_users = 37
    dims = [c1] + HIDDEN[n_layers](c1)[1:] + [1]
    widths = [c1] + HIDDEN[n_layers](c1)
    layers = [(rng.normal(0, 1 / np.sqrt(a), size=(a, b)).astype(np.float32), rng.uniform(-0.1, 0.1, size=b).astype(np.float32))
              for a, b in zip(widths[:-1], widths[1:])]
    layers.append(((rng.normal(0, 4 / np.sqrt(widths[-1]), size=(widths[-1], 1))).astype(np.float32),
                   rng.uniform(-0.1, 0.1, size=1).astype(np.float32)))
    dims = widths + [1]
    tu = rng.normal(0, 1, size=(n_users, c1)).astype(np.float32)
    ti = rng.normal(0, 1, size=(n_items, c1)).astype(np.float32)
    if n_items > 4:
        ti[n_items // 2] = ti[1]                          # duplicated rows: exact ties, ordered by item id
        ti[n_items - 1] = ti[1]
    want64 = _grid64(tu, ti, layers)
    # exclusions: random training pairs; user 0 has seen everything, user 1 all but 3 items (fewer than k for k >= 10)
    pairs = [(u, i) for u in range(2, n_users) for i in rng.choice(n_items, size=min(n_items, rng.integers(0, 40)), replace=False)]
    pairs += [(0, i) for i in range(n_items)] + [(1, i) for i in range(3, n_items)]
    ratings = np.array([(u, i + n_users, 1) for u, i in pairs] + [(u, i + n_users, 0) for u, i in pairs[:5]], dtype=np.int64)
    ptr, ex_items = rec.exclusion_csr(ratings, n_users, n_items)
    excl = {u: set(ex_items[ptr[u]:ptr[u + 1]].tolist()) for u in range(n_users)}
    blob, _ = capi.chain_pack([w for w, _ in layers], [b for _, b in layers])
    dev = torch.device('cuda')
    blob, tu_d, ti_d = torch.from_numpy(blob).to(dev), torch.from_numpy(tu).to(dev), torch.from_numpy(ti).to(dev)
    ptr_d = torch.from_numpy(ptr.astype(np.int32)).to(dev)
    ex_d = torch.from_numpy(ex_items.astype(np.int32)).to(dev)
    acts = ['relu'] * (len(dims) - 2) + ['sigmoid']
    subset = rng.permutation(n_users)[:11]
    for k in (1, 10, 64):
        got_i, got_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k, excl_ptr=ptr_d, excl_items=ex_d)
        got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
        differing = _check_lists(np.arange(n_users), got_i, got_s, want64, excl, k, 0, 'c1={} k={}'.format(c1, k))
        assert differing <= MAX_NEAR_TIE_USERS
        # a shuffled subset: rows in the given order, bitwise the rows of the full call
        sub_i, sub_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k, users=torch.from_numpy(subset.astype(np.int32)).to(dev),
                                      excl_ptr=ptr_d, excl_items=ex_d)
        assert np.array_equal(sub_i.cpu().numpy(), got_i[subset]) and np.array_equal(sub_s.cpu().numpy(), got_s[subset])
        # any item slicing gives the same bits
        for slices in (1, 2, 5):
            if slices > 1 and hip.load().amar_recommend_slices(n_users, n_items, (ctypes_dims(dims)), len(dims) - 1, slices) != slices:
                continue
            s_i, s_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k, excl_ptr=ptr_d, excl_items=ex_d, n_slices=slices)
            assert np.array_equal(s_i.cpu().numpy(), got_i) and np.array_equal(s_s.cpu().numpy(), got_s), slices
        # exclusion off: every item ranks
        all_i, _ = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k)
        assert (all_i.cpu().numpy()[0] >= 0).sum() == min(k, n_items)
    if n_items > 4:
        big_i, big_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', 64)
        row = big_i.cpu().numpy()[5].tolist()
        dup = [i for i in (1, n_items // 2, n_items - 1) if i in row]
        assert [i for i in row if i in dup] == sorted(dup)  # tied duplicates in item order


@pytest.mark.parametrize('k', [1, 63, 64])
def test_selector_adversarial_orders(hip, k):
    """The shared selector where it merges most and least: 197 items, 19 users, scores strictly ascending in the item row (every
    item beats the threshold: a merge per full buffer) and the table reversed (nothing after the first k passes), exclusions on
    group and tile edges, one user with nothing left and one with k - 1 items left.  Tu = 0, Ti[i, 0] = i / 197 through an identity
    Dense(16, relu) and Dense(1, sigmoid) on feature 0: sigmoid(i / 197), about 1e-3 apart, so the lists are known exactly."""
    import torch
    from deep_cbrs_amar_renaissance_amd import capi
    n, m, c1 = helpers.SELECT_ROWS, helpers.SELECT_QUERIES, 16
    dev = torch.device('cuda')
    excl = helpers.select_case_exclusions(k, tile_rows=256)                              # c1 = 16 stages 256-item tiles
    ptr = np.cumsum([0] + [len(excl[u]) for u in range(m)])
    ptr_d = torch.from_numpy(ptr.astype(np.int32)).to(dev)
    ex_d = torch.from_numpy(np.array([i for u in range(m) for i in sorted(excl[u])], dtype=np.int32)).to(dev)
    dot = np.zeros((c1, 1), dtype=np.float32)
    dot[0, 0] = 1.0
    blob, _ = capi.chain_pack([np.eye(c1, dtype=np.float32), dot], [np.zeros(c1, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    blob, dims, acts = torch.from_numpy(blob).to(dev), [c1, c1, 1], ['relu', 'sigmoid']
    tu_d = torch.zeros((m, c1), dtype=torch.float32, device=dev)
    for reverse in (False, True):
        value = np.arange(n)[::-1] if reverse else np.arange(n)                          # item i scores sigmoid(value[i] / 197)
        ti = np.zeros((n, c1), dtype=np.float32)
        ti[:, 0] = value / np.float32(n)
        want_i = helpers.select_case_expected(excl, k, np.argsort(-value, kind='stable').tolist())
        want_s = np.where(want_i >= 0, 1.0 / (1.0 + np.exp(-ti[np.maximum(want_i, 0), 0].astype(np.float64))), -np.inf)
        ti_d = torch.from_numpy(ti).to(dev)
        first = None
        for slices in (1, 2, 3):
            if hip.load().amar_recommend_slices(m, n, ctypes_dims(dims), len(dims) - 1, slices) != slices:
                continue
            got_i, got_s = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', k, excl_ptr=ptr_d, excl_items=ex_d, n_slices=slices)
            got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
            assert np.array_equal(got_i, want_i), (k, reverse, slices)
            assert np.array_equal(np.isneginf(got_s), want_i < 0) and np.abs(got_s[want_i >= 0] - want_s[want_i >= 0]).max() <= 1e-6
            first = got_s if first is None else first
            assert np.array_equal(got_s.view(np.int32), first.view(np.int32)), (k, reverse, slices)


def ctypes_dims(dims):
    import ctypes
    return (ctypes.c_int32 * len(dims))(*dims)


# ---- 2. models: fused route against the pair route and the oracle --------------------------------------------------
GRID1 = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48],
             l2_regularizer=1e-4, final_node='concatenation', aggregate='mean', dropout_rate=0.0, activation='relu')


def _excl_sets(ratings, n_users):
    out = {}
    for u, i in zip(ratings[:, 0].tolist(), ratings[:, 1].tolist()):
        out.setdefault(int(u), set()).add(int(i) - n_users)
    return out


def _grid_ids(n_users, n_items, users=None):
    users = np.arange(n_users) if users is None else np.asarray(users)
    return np.repeat(users, n_items), np.tile(np.arange(n_items) + n_users, len(users))


def _basic_oracle_grid(model, kind, g):
    nu, ni = g['n_users'], g['n_items']
    head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in v] for k, v in helpers.basic_head_to_oracle(model.rs).items()}
    if kind == 'TS':
        e = om.two_step((g['adj_ui'], g['adj_ip']), helpers.two_step_to_oracle(model.gnn), nu, ni, np.float64)
    elif kind == 'TW':
        e = om.two_way((g['adj_ui'], g['adj_ip'], g['adj_up']), helpers.two_way_to_oracle(model.gnn), nu, ni, np.float64)
    else:
        u, i = _grid_ids(nu, ni)
        return om.basic_gnn_scores(g['adj'], helpers.gnn_to_oracle(model.gnn), head, u, i, dtype=np.float64).reshape(nu, ni)
    u, i = _grid_ids(nu, ni)
    return om.basic_rs(e[u], e[i], head).reshape(nu, ni)


def _compare_routes(model, train, want64, n_users, label, k_list=(5, 10, 25)):
    excl = _excl_sets(train.ratings, n_users)
    for k in k_list:
        fu, fi, fs = model.recommend(train, k=k)
        pu, pi, ps = model._recommend_pairs(train, k=k)
        assert np.array_equal(fu, pu) and fu.dtype == np.int64 and fi.dtype == np.int64 and fs.dtype == np.float32
        assert fi.shape == (n_users, k) and fs.shape == (n_users, k)
        fin = np.isfinite(fs)
        assert np.array_equal(fin, np.isfinite(ps)) and (not fin.any() or np.abs(fs[fin] - ps[fin]).max() <= 2e-6), label
        for (i_, s_), route in (((fi, fs), 'fused'), ((pi, ps), 'pairs')):
            d = _check_lists(fu, i_, s_, want64, excl, k, n_users, '{} {} k={}'.format(label, route, k), score_tol=1e-5)
            assert d <= MAX_NEAR_TIE_USERS
        for r, u in enumerate(fu.tolist()):                               # no training item comes back
            assert not (set(fi[r][fi[r] >= 0].tolist()) & {i + n_users for i in excl.get(u, set())})


@pytest.mark.parametrize('name', ['BasicGCN', 'BasicLightGCN', 'BasicGraphSage', 'BasicGAT', 'BasicDGCF', 'BasicTSGCN', 'BasicTWGraphSage'])
def test_models_fused_against_pairs_and_oracle(hip, name):
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(11)
    kind = 'TS' if name.startswith('BasicTS') else ('TW' if name.startswith('BasicTW') else '')
    if kind:
        g = helpers.kg_graph(seed=3)
        adjs = (g['adj_ui'], g['adj_ip']) if kind == 'TS' else (g['adj_ui'], g['adj_ip'], g['adj_up'])
        model = getattr(basic, name)(g['n_users'], g['n_items'], adjs, **GRID1)
    else:
        g = helpers.tiny_graph(seed=5)
        model = getattr(basic, name)(g['adj'], **GRID1)
    helpers.randomize_biases(model, seed=2)
    helpers.spread_scores(model, 10.0)
    train = _Train(g['ratings'], g['n_users'], g['n_items'])
    assert model._recommend_route(train) == 'fused'
    _compare_routes(model, train, _basic_oracle_grid(model, kind, g), g['n_users'], name)


def test_basic_gcn_default_head_ml1m(hip, ml1m_s1):
    """The default GNN head (rest = 16 -> 16 -> 1) at ml1m(s=1): the fused route and the pair route run the same product routine, so
    their lists and scores are bitwise equal; a sample of users is held against the float64 oracle."""
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(5)
    d = ml1m_s1
    nu, ni = len(d['users']), len(d['items'])
    model = basic.BasicGCN(d['adj_ui'], embedding_dim=16, n_hiddens=[16, 16], l2_regularizer=1e-4)
    helpers.randomize_biases(model, seed=3)
    helpers.spread_scores(model)
    train = _Train(d['train'], nu, ni)
    fu, fi, fs = model.recommend(train, k=10)
    pu, pi, ps = model._recommend_pairs(train, k=10)
    assert np.array_equal(fi, pi) and np.array_equal(fs.view(np.int32), ps.view(np.int32))
    sample = np.random.default_rng(0).choice(nu, size=200, replace=False)
    u, i = _grid_ids(nu, ni, sample)
    head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in v] for k, v in helpers.basic_head_to_oracle(model.rs).items()}
    want = np.zeros((nu, ni))
    want[sample] = om.basic_gnn_scores(d['adj_ui'], helpers.gnn_to_oracle(model.gnn), head, u, i, dtype=np.float64).reshape(len(sample), ni)
    excl = _excl_sets(d['train'], nu)
    diff = _check_lists(sample, fi[sample], fs[sample], want, excl, 10, nu, 'ml1m BasicGCN', score_tol=1e-5)
    assert diff <= MAX_NEAR_TIE_USERS
    # predict() scores the same pairs with the same bits
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    top = np.stack([np.repeat(fu[:50], 10), fi[:50].reshape(-1), np.ones(500, dtype=np.int64)], axis=1)
    pred = model.predict(UserItemGraph(top, d['users'], d['items'], d['adj_ui'], batch_size=512)).reshape(-1)
    assert np.array_equal(pred.astype(np.float32).view(np.int32), fs[:50].reshape(-1).view(np.int32))


# ---- 3. embedding-table and hybrid models --------------------------------------------------------------------------
@pytest.mark.parametrize('dense_units', [[64, 32], [512, 256, 128]])
def test_basic_rs_kge_head_fused(hip, dense_units):
    import torch
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(7)
    g = helpers.tiny_graph(n_users=45, n_items=70, n_ratings=900, seed=9)
    nu, ni = g['n_users'], g['n_items']
    table = np.random.default_rng(4).normal(0, 1, size=(nu + ni, 32)).astype(np.float32)
    model = basic.BasicRS(dense_units=dense_units, clf_units=[64, 64])      # [512, 256, 128]: the basic-kge head
    model.build_head(32, 32)
    helpers.randomize_biases(model, seed=1)
    with torch.no_grad():
        model.clf.layers[-1].kernel.mul_(10.0)
    train = UserItemEmbeddings(g['ratings'], g['users'], g['items'], table)
    assert model._recommend_route(train) == 'fused'
    head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in v] for k, v in helpers.basic_head_to_oracle(model).items()}
    u, i = _grid_ids(nu, ni)
    want = om.basic_rs(table[u].astype(np.float64), table[i].astype(np.float64), head).reshape(nu, ni)
    _compare_routes(model, train, want, nu, 'BasicRS kge {}'.format(dense_units))


def _hybrid_bert_gcn(g, fusion):
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    return hybrid.HybridBertGCN(g['adj'], **dict(GRID1, dense_units=[[24, 24], [32, 16], [16, 16]], clf_units=[16, 16],
                                                  feature_based=True, fusion_method=fusion))


@pytest.mark.parametrize('fusion', ['concatenate', 'attention'])
def test_hybrid_bert_gnn_pair_route(hip, fusion):
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    set_seed(3)
    g = helpers.tiny_graph(seed=6)
    nu, ni = g['n_users'], g['n_items']
    bert = np.random.default_rng(2).normal(0, 1, size=(nu + ni, 48)).astype(np.float32)
    model = _hybrid_bert_gcn(g, fusion)
    model.set_bert_table(bert)
    model.rs.build_head(model.gnn.output_dim(), 48)
    helpers.randomize_biases(model, seed=4)
    helpers.spread_scores(model, 10.0)
    train = _Train(g['ratings'], nu, ni)
    assert model._recommend_route(train) == 'pairs'
    u, i = _grid_ids(nu, ni)
    head = {k: ([(w.astype(np.float64), b.astype(np.float64)) for w, b in v] if isinstance(v, list) else
                {kk: vv.astype(np.float64) for kk, vv in v.items()}) for k, v in helpers.hybrid_head_to_oracle(model.rs).items()}
    want = om.hybrid_gnn_scores(g['adj'], helpers.gnn_to_oracle(model.gnn), head, u, i, bert, dtype=np.float64,
                                feature_based=True).reshape(nu, ni)
    excl = _excl_sets(g['ratings'], nu)
    for k in (5, 25):
        ru, ri, rs = model.recommend(train, k=k)
        assert _check_lists(ru, ri, rs, want, excl, k, nu, 'HybridBertGCN {} k={}'.format(fusion, k), score_tol=1e-5) <= MAX_NEAR_TIE_USERS


def test_hybrid_cbrs_pair_route(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import HybridUserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    set_seed(8)
    g = helpers.tiny_graph(seed=7)
    nu, ni = g['n_users'], g['n_items']
    rng = np.random.default_rng(5)
    ge = rng.normal(0, 1, size=(nu + ni, 16)).astype(np.float32)
    be = rng.normal(0, 1, size=(nu + ni, 40)).astype(np.float32)
    model = hybrid.HybridCBRS(feature_based=False, dense_units=[[32, 16], [64, 16], [32, 8]], clf_units=[16])
    model.build_head(16, 40)
    helpers.randomize_biases(model, seed=6)
    train = HybridUserItemEmbeddings(g['ratings'], g['users'], g['items'], ge, be)
    assert model._recommend_route(train) == 'pairs'
    u, i = _grid_ids(nu, ni)
    head = {k: [(w.astype(np.float64), b.astype(np.float64)) for w, b in v] for k, v in helpers.hybrid_head_to_oracle(model).items()}
    want = om.hybrid_cbrs(ge[u].astype(np.float64), ge[i].astype(np.float64), be[u].astype(np.float64), be[i].astype(np.float64), head,
                          feature_based=False).reshape(nu, ni)
    ru, ri, rs = model.recommend(train, k=10)
    assert _check_lists(ru, ri, rs, want, _excl_sets(g['ratings'], nu), 10, nu, 'HybridCBRS', score_tol=1e-5) <= MAX_NEAR_TIE_USERS


def test_route_taken_by_each_class(hip, monkeypatch):
    """The fused heads really launch amar_recommend_f32 (and no pair ranking); the others rank pairs — a head that silently fell back
    would show up here."""
    from deep_cbrs_amar_renaissance_amd import capi
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.models import basic
    calls = {'fused': 0, 'pairs': 0}
    fused, topk = capi.recommend, capi.topk_segmented
    monkeypatch.setattr(capi, 'recommend', lambda *a, **kw: (calls.__setitem__('fused', calls['fused'] + 1), fused(*a, **kw))[1])
    monkeypatch.setattr(capi, 'topk_segmented', lambda *a, **kw: (calls.__setitem__('pairs', calls['pairs'] + 1), topk(*a, **kw))[1])
    g = helpers.tiny_graph(seed=1)
    nu, ni = g['n_users'], g['n_items']
    table = np.random.default_rng(1).normal(size=(nu + ni, 16)).astype(np.float32)
    bert = np.random.default_rng(2).normal(size=(nu + ni, 48)).astype(np.float32)
    hyb = _hybrid_bert_gcn(g, 'concatenate')
    hyb.set_bert_table(bert)
    cases = [(basic.BasicGCN(g['adj'], **GRID1), _Train(g['ratings'], nu, ni), 'fused'),
             (basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8]), _Train(g['ratings'], nu, ni), 'fused'),
             (basic.BasicRS(dense_units=[32, 16], clf_units=[16, 16]), UserItemEmbeddings(g['ratings'], g['users'], g['items'], table), 'fused'),
             (basic.BasicRS(dense_units=[32, 16], clf_units=[16]), UserItemEmbeddings(g['ratings'], g['users'], g['items'], table), 'pairs'),
             (hyb, _Train(g['ratings'], nu, ni), 'pairs')]
    for model, train, route in cases:
        before = dict(calls)
        assert model._recommend_route(train) == route, type(model).__name__
        model.recommend(train, k=5)
        assert calls[route] == before[route] + 1 and sum(calls.values()) == sum(before.values()) + 1, (type(model).__name__, route)


# ---- 4. invariance ---------------------------------------------------------------------------------------------------
def test_invariance_and_no_side_effects(hip):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.tiny_graph(n_users=300, n_items=500, n_ratings=9000, seed=12)
    nu, ni = g['n_users'], g['n_items']
    model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8])
    helpers.randomize_biases(model, seed=9)
    helpers.spread_scores(model)
    train = _Train(g['ratings'], nu, ni)
    test_seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=256)
    p0, v0 = model.predict(test_seq), model.weights_version
    state0 = (model.gnn.hoist, model.gnn._hoisted, model._towers)
    a = model.recommend(train, k=20)
    b = model.recommend(train, k=20)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.int32) if x.dtype == np.float32 else x,
                              np.asarray(y).view(np.int32) if y.dtype == np.float32 else y)
    assert (model.gnn.hoist, model.gnn._hoisted, model._towers) == state0
    assert model.weights_version == v0
    assert np.array_equal(model.predict(test_seq).view(np.int32), p0.view(np.int32))
    for users in ([123], [299, 0, 17, 123, 5], list(range(nu - 1, -1, -3))):
        su, si, ss = model.recommend(train, k=20, users=users)
        assert np.array_equal(su, users)
        assert np.array_equal(si, a[1][users]) and np.array_equal(ss.view(np.int32), a[2][users].view(np.int32))
    eu, ei, es = model.recommend(train, k=20, users=[])
    assert eu.shape == (0,) and ei.shape == (0, 20) and es.shape == (0, 20)
    with pytest.raises(ValueError):
        model.recommend(train, k=65)
    with pytest.raises(ValueError):
        model.recommend(train, k=3, users=[nu])
    # exclude_seen=False ranks every item: the k best of the grid, seen ones included
    _, ai, _ = model.recommend(train, k=5, exclude_seen=False)
    assert (ai >= 0).all()


# ---- 5. experiment ---------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, full_ks, capture):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(capture['paths'])
    cfg['parameters']['epochs'] = 1
    if full_ks:
        cfg['parameters']['full_ranking_ks'] = full_ks
    (tmp_path / (name + '.yaml')).write_text(yaml.safe_dump(cfg))
    (tmp_path / (name + '_exps.yaml')).write_text(
        "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
        "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
    run_log = setup_mlflow(name, str(tmp_path / 'mlruns'))
    multi = experiment.MultiExperimenter(str(tmp_path / (name + '.yaml')), str(tmp_path / (name + '_exps.yaml')), run_log)
    results = multi.run()
    assert all(v is not None for v in results.values())
    runs = glob.glob(str(tmp_path / 'mlruns' / name / '*'))
    assert len(runs) == 1
    return runs[0], results


def test_experiment_full_ranking_opt_in(hip, tmp_path, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    capture = {'paths': {k: v for k, v in paths.items() if k != 'props_triples_filepath'}}
    original = experiment.Experimenter.evaluate_full_ranking

    def spy(self, ks):
        capture['exp'] = self
        return original(self, ks)

    monkeypatch.setattr(experiment.Experimenter, 'evaluate_full_ranking', spy)
    monkeypatch.chdir(tmp_path)
    run_on, res_on = _run_experiment(tmp_path, 'with_key', [5, 10], capture)
    exp = capture.pop('exp')
    for k in (5, 10):
        tsv = os.path.join(run_on, 'artifacts', 'predictions', 'full_ranking', 'top_{}.tsv'.format(k))
        assert os.path.exists(tsv)
    users, items, scores = exp.model.recommend(exp.trainset, k=10)
    want = full_ranking_metrics(users, items, exp.testset.ratings, [5, 10])
    logged = {}
    for line in open(os.path.join(run_on, 'run.jsonl')):
        rec = json.loads(line)
        if rec['event'] == 'metrics':
            logged.update(rec['metrics'])
    for k in (5, 10):
        for m in ('precision', 'recall', 'ndcg', 'hit'):
            assert logged['full_{}_at_{}'.format(m, k)] == want['{}_at_{}'.format(m, k)]
    import pandas as pd
    top = pd.read_csv(os.path.join(run_on, 'artifacts', 'predictions', 'full_ranking', 'top_10.tsv'), sep='\t', header=None)
    assert top.groupby(0).size().max() == 10 and set(top[1]).issubset(set(ds.train[:, 1]))
    run_off, res_off = _run_experiment(tmp_path, 'without_key', None, capture)
    assert 'exp' not in capture
    rel = lambda root: sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, '**', '*'), recursive=True) if os.path.isfile(p))
    assert rel(run_off) == [p for p in rel(run_on) if 'full_ranking' not in p]
    off_metrics = set()
    for line in open(os.path.join(run_off, 'run.jsonl')):
        rec = json.loads(line)
        if rec['event'] == 'metrics':
            off_metrics.update(rec['metrics'])
    assert not any(m.startswith('full_') for m in off_metrics)
    assert list(list(res_off.values())[0].columns) == list(list(res_on.values())[0].columns) == [5, 10]
