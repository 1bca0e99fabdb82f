"""GPU: calibrated re-ranking (amar_rerank_calibrated_f32, amar_list_calibration_f64, recommend_calibrated / list_calibration /
evaluate_ranking(calibration=...) and the experiment opt-in) against the float64 restatement of tests/calibrate_ref.py (pytest -m gpu).

Tolerances (derived in tests/calibrate_ref.py from the float32 roundings of the contract and logf's documented 1 ulp): tol_C per
candidate, tol_v = (1 - lam) tol_C + 2^-24 (5 lam + 2 (1 - lam) C).  Whole lists equal the float64 greedy except where a float64 step
has another candidate within the two tolerances of the pick; at most MAX_NEAR_TIE_LISTS of the 37 lists may differ that way (the
seeds keep the reference itself within that cap: tests/test_calibrate_cpu.py)."""
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import calibrate_ref as ref
from tests.test_calibrate_cpu import EXACT_CASE

pytestmark = pytest.mark.gpu


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _device_case(case):
    cats, liked, pool, scores, users = case
    d = dict(zip(('cat_ptr', 'cat_ids', 'liked_ptr', 'liked_items', 'pool', 'scores', 'users'),
                 _dev(cats[0], cats[1], liked[0], liked[1], pool, scores, users)))
    d['max_row'] = cats[2]
    return d


def _rerank(hip, d, G, k, lam, alpha, users='given', pool=None, scores=None, **want):
    return hip.rerank_calibrated(d['pool'] if pool is None else pool, d['scores'] if scores is None else scores, d['liked_ptr'],
                                 d['liked_items'], d['cat_ptr'], d['cat_ids'], G, k, trade_off=lam, smoothing=alpha,
                                 users=d['users'] if isinstance(users, str) else users, max_cat_row=d['max_row'], **want)


def _check_case(hip, case, G, settings, label0):
    """check_steps, the targets' bits, the scores' bits and the comparison of whole lists with the float64 greedy; returns the worst
    error / tolerance of out_value and out_kl."""
    cats, liked, pool, scores, users = case
    d = _device_case(case)
    P = pool.shape[1]
    want_p = np.stack([ref.target32(ref.liked_of(liked, int(u)), cats, G)[0] for u in users])
    worst = (0.0, 0.0)
    for lam, alpha, k in settings:
        label = '{} lam={} a={} k={}'.format(label0, lam, alpha, k)
        items, sc, val, kl, target = _rerank(hip, d, G, k, lam, alpha, want_value=True, want_kl=True, want_target=True)
        got_i, got_s, got_v, got_c = items.cpu().numpy(), sc.cpu().numpy(), val.cpu().numpy(), kl.cpu().numpy()
        assert got_i.dtype == np.int32 and got_i.shape == (len(pool), k) and not np.isnan(got_v).any() and not np.isnan(got_c).any()
        assert np.array_equal(_bits(target), want_p.view(np.int32)), label + ': out_target is the float32 loop, bit for bit'
        w = ref.check_steps(pool, scores, users, liked, cats, G, got_i, got_v, got_c, lam, alpha, k, label)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        differing = 0
        for j in range(len(pool)):
            for s in range(k):
                if got_i[j, s] < 0:
                    assert np.isneginf(got_s[j, s])
                else:
                    at = pool[j].tolist().index(got_i[j, s])
                    assert got_s[j, s].view(np.int32) == scores[j, at].view(np.int32), label
            want_i, _, _, _, near = ref.greedy64(pool[j], scores[j], ref.liked_of(liked, int(users[j])), cats, G, lam, alpha, k)
            if not np.array_equal(got_i[j], want_i):
                assert near, '{}: list {} differs from float64 without a near-tie'.format(label, j)
                differing += 1
        print('{}: max err/tol out_value {:.3f} out_kl {:.3f}, lists differing by near-ties {}'.format(label, w[0], w[1], differing))
        assert differing <= ref.MAX_NEAR_TIE_LISTS, label
        if dict(P=P, G=G, lam=lam, alpha=alpha) == EXACT_CASE:
            assert differing == 0, label
    return worst


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', ref.GRID_G)
@pytest.mark.parametrize('P', ref.GRID_P)
def test_rerank_kernel_against_float64(hip, P, G):
    """Every trade-off and smoothing at k < P (k = P where P is 1), every trade-off at k = P with the first smoothing."""
    ks = ref.grid_ks(P)
    settings = [(lam, a, ks[0]) for lam in ref.GRID_LAMBDA for a in ref.GRID_ALPHA]
    settings += [(lam, ref.GRID_ALPHA[0], P) for lam in ref.GRID_LAMBDA if P != ks[0]]
    worst = (0.0, 0.0)
    for short in sorted({lam == 0 and (P, G) in ref.LIST_LENGTHS_AT for lam in ref.GRID_LAMBDA}):
        part = [st for st in settings if (st[0] == 0 and (P, G) in ref.LIST_LENGTHS_AT) == short]
        w = _check_case(hip, ref.planted_case(P, G, short=short), G, part, 'P={} G={}{}'.format(P, G, ' short lists' if short else ''))
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print('P={} G={}: worst err/tol out_value {:.3f} out_kl {:.3f}'.format(P, G, *worst))


@pytest.mark.parametrize('P,G', ref.DENSE_CASES)
def test_pool_rows_past_the_staging_budget(hip, P, G):
    """Dense category rows: a full pool holds more than AMAR_CALIBRATE_POOL_BUDGET ids, so the later positions read memory."""
    case = ref.planted_case(P, G, dense=True)
    assert np.diff(case[0][0])[case[2][-1]].sum() > ref.POOL_BUDGET
    worst = _check_case(hip, case, G, ref.dense_settings(P), 'dense P={} G={}'.format(P, G))
    print('dense P={} G={}: worst err/tol out_value {:.3f} out_kl {:.3f}'.format(P, G, *worst))


def test_exact_ties_go_to_the_smaller_position(hip):
    """Two genres and dyadic numbers: candidates of one genre with one score are the same arithmetic, so the position decides; with
    trade_off = 0 the score does not count at all."""
    cats, liked = ref.two_genre_case()
    pool = np.array([[12, 3, 20, 15, 1, 21, 0, 10], [0, 1, 2, 10, 11, 12, 20, 21], [21, 20, 12, 11, 10, 2, 1, 0]], dtype=np.int32)
    scores = np.array([[0.5, 0.75, 0.75, 0.5, 0.75, 0.25, 0.75, 0.5]] * 3, dtype=np.float32)
    users = np.zeros(3, dtype=np.int32)
    d = _device_case(((cats[0], cats[1], 1), liked, pool, scores, users))
    for lam in (0.0, 0.25, 1.0):
        for k in (1, 5, 8):
            items = _rerank(hip, d, 2, k, lam, 0.01)[0].cpu().numpy()
            for j in range(3):
                want, _, _, _, near = ref.greedy64(pool[j], scores[j], ref.liked_of(liked, 0), cats, 2, lam, 0.01, k, n_items=24)
                assert not near and np.array_equal(items[j], want), (lam, k, j, items[j], want)
    first = _rerank(hip, d, 2, 8, 0.0, 0.01)[0].cpu().numpy()
    # a drama first (0.7 is nearer to it), then a comedy: each the first of its genre in pool order
    assert first[1].tolist()[:2] == [0, 10] and first[2].tolist()[:2] == [2, 12]


def test_invariance_and_users(hip):
    """A second call, explicit users against users == NULL, a shuffled and duplicated subset of the lists, every list alone, a user
    id outside the table: the same bits per list."""
    import torch
    P, G = 17, 65
    case = ref.planted_case(P, G)
    d = _device_case(case)
    call = lambda users, pool=None, scores=None: [_bits(x) for x in _rerank(hip, d, G, 10, 0.5, 0.01, users=users, pool=pool, scores=scores,
                                                                             want_value=True, want_kl=True, want_target=True)]
    full = call('given')
    assert all(np.array_equal(a, b) for a, b in zip(full, call('given')))
    assert all(np.array_equal(a, b) for a, b in zip(full, call(None)))
    pick = np.concatenate([np.random.default_rng(1).permutation(len(case[2]))[:11], [5, 5, 3]])
    idx = torch.from_numpy(pick).cuda()
    sub = call(d['users'][idx].contiguous(), d['pool'][idx].contiguous(), d['scores'][idx].contiguous())
    assert all(np.array_equal(a[pick], b) for a, b in zip(full, sub))
    for j in (0, 1, 3, len(case[2]) - 1):
        one = call(d['users'][j:j + 1].contiguous(), d['pool'][j:j + 1].contiguous(), d['scores'][j:j + 1].contiguous())
        assert all(np.array_equal(a[j:j + 1], b) for a, b in zip(full, one))
    bad = d['users'].clone()
    bad[4], bad[9] = -1, ref.N_USERS
    out = _rerank(hip, d, G, 10, 0.5, 0.01, users=bad, want_value=True, want_kl=True, want_target=True)
    for j in (4, 9):
        assert torch.all(out[0][j] == -1) and all(torch.all(torch.isneginf(t[j])) for t in out[1:4]) and torch.all(out[4][j] == 0)
    assert np.array_equal(_bits(out[0])[10:], full[0][10:])


@pytest.mark.parametrize('K,G', [(1, 1), (5, 3), (17, 64), (64, 65), (33, 1024)])
def test_list_calibration_against_the_host_metric(hip, K, G):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    cats, liked, lists, _, users = ref.planted_case(K, G)
    d = _device_case((cats, liked, lists, np.zeros_like(lists, dtype=np.float32), users))
    ks = sorted({1, min(2, K), min(5, K), K})
    worst = 0.0
    for alpha in ref.GRID_ALPHA:
        kl, count, support = hip.list_calibration(d['pool'], d['liked_ptr'], d['liked_items'], d['cat_ptr'], d['cat_ids'], G, ks,
                                                  smoothing=alpha, users=d['users'])
        want, want_n, want_s = miscalibration(lists, users, liked, cats, ks, alpha)
        got = kl.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (len(lists), len(ks))
        assert np.array_equal(count.cpu().numpy(), want_n) and np.array_equal(support.cpu().numpy(), want_s)
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.all(np.abs(got - want) <= 1e-12), (alpha, float(np.abs(got - want).max()))
        assert np.all(got[want_s == 0] == 0.0)
        again = hip.list_calibration(d['pool'], d['liked_ptr'], d['liked_items'], d['cat_ptr'], d['cat_ids'], G, ks, smoothing=alpha, users=None)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, (kl, count, support)))
        # cutoffs in any order
        back = hip.list_calibration(d['pool'], d['liked_ptr'], d['liked_items'], d['cat_ptr'], d['cat_ids'], G, ks[::-1], smoothing=alpha)
        assert np.array_equal(_bits(back[0])[:, ::-1], _bits(kl))
    print('K={} G={}: max |kl - host| {:.3e}'.format(K, G, worst))


def test_refusals_make_no_device_call(hip):
    import ctypes
    import torch
    lib = hip.load()
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device='cuda')
    pool, sc = z(3, 65), z(3, 65, dtype=torch.float32)
    out_i, out_s, out_d = z(3, 65), z(3, 65, dtype=torch.float32), z(3, 8, dtype=torch.float64)
    lp, li, cp, ci, sup = z(4), z(4), z(11), z(4), z(3)
    torch.cuda.synchronize()
    before = lib.amar_last_hip_error()
    ks = (ctypes.c_int32 * 2)(1, 17)
    good = dict(P=16, G=8, k=4, lam=0.5, a=0.01, m=3, nu=3, users=None, lp=lp.data_ptr(), cp=cp.data_ptr(), row=2)
    cases = [(dict(P=65), -2), (dict(G=1025), -2), (dict(k=17), -2), (dict(row=9), -2), (dict(lam=1.5), -1), (dict(lam=-0.25), -1),
             (dict(lam=float('nan')), -1), (dict(a=0.0), -1), (dict(a=1.0), -1), (dict(a=float('nan')), -1), (dict(k=0), -1),
             (dict(G=0), -1), (dict(P=0), -1), (dict(nu=4), -1), (dict(lp=None), -1), (dict(cp=None), -1), (dict(row=-1), -1), (dict(nu=-1), -1)]
    for change, want in cases:
        a = dict(good, **change)
        got = lib.amar_rerank_calibrated_f32(pool.data_ptr(), sc.data_ptr(), a['m'], a['P'], a['users'], a['lp'], li.data_ptr(), a['nu'],
                                             a['cp'], ci.data_ptr(), 10, a['G'], a['row'], a['lam'], a['a'], a['k'], out_i.data_ptr(),
                                             out_s.data_ptr(), None, None, None, None)
        assert got == want, ('rerank', change, got)
        if set(change) & {'k', 'lam', 'row'}:
            continue
        got = lib.amar_list_calibration_f64(pool.data_ptr(), a['m'], a['P'], a['users'], a['lp'], li.data_ptr(), a['nu'], a['cp'],
                                            ci.data_ptr(), 10, a['G'], a['a'], ks, 1, out_d.data_ptr(), out_i.data_ptr(), sup.data_ptr(), None)
        assert got == want, ('metric', change, got)
    metric = lambda nk: lib.amar_list_calibration_f64(pool.data_ptr(), 3, 16, None, lp.data_ptr(), li.data_ptr(), 3, cp.data_ptr(), ci.data_ptr(),
                                                       10, 8, 0.01, ks, nk, out_d.data_ptr(), out_i.data_ptr(), sup.data_ptr(), None)
    assert metric(2) == -1 and metric(9) == -2 and metric(0) == -1
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert int(out_i.abs().sum()) == 0 and float(out_s.abs().sum()) == 0.0                 # nothing was launched
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    cats, liked = (cp, ci, 8, 0), (lp, li)
    with pytest.raises(ValueError):
        rec.rerank_calibrated(pool[:, :8], sc[:, :8], None, liked, cats, 9)
    with pytest.raises(ValueError):
        rec.rerank_calibrated(pool[:, :8], sc[:, :8], None, liked, cats, 4, trade_off=1.5)
    with pytest.raises(ValueError):
        rec.rerank_calibrated(pool[:, :8], sc[:, :8], None, liked, cats, 4, smoothing=0.0)


# ---- 2. models -----------------------------------------------------------------------------------------------------------
def _uip_model(name):
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    from tests import helpers
    from tests.test_explain_gpu import _Train
    from tests.test_similar_gpu import GRID1
    set_seed(11)
    g = helpers.tiny_graph(n_users=40, n_items=30, n_ratings=500, seed=5, n_props=25, n_links=160)
    if name == 'BasicGCN':
        model = basic.BasicGCN(g['adj'], **GRID1)
    else:
        model = hybrid.HybridBertGCN(g['adj'], **dict(GRID1, dense_units=[[24, 24], [32, 16], [16, 16]], clf_units=[16, 16],
                                                       feature_based=True, fusion_method='concatenate'))
        model.set_bert_table(np.random.default_rng(2).normal(0, 1, size=(g['n_users'] + g['n_items'], 48)).astype(np.float32))
        model.rs.build_head(model.gnn.output_dim(), 48)
    helpers.randomize_biases(model, seed=2)
    return model, _Train(g['ratings'], g['n_users'], g['n_items'], g['adj']), g


@pytest.mark.parametrize('name', ['BasicGCN', 'HybridBertGCN'])
def test_models_recommend_calibrated(hip, name):
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import miscalibration
    model, train, g = _uip_model(name)
    nu, ni = g['n_users'], g['n_items']
    cats = rec.item_category_csr(train)
    G = len(cats[2])
    liked = tuple(a.astype(np.int32) for a in rec.liked_csr(train.ratings, nu, ni))
    users, top_i, top_s = model.recommend(train, k=10)
    # trade_off = 1: recommend(k) itself
    u1, i1, s1 = model.recommend_calibrated(train, k=10, pool=25, trade_off=1.0)
    assert np.array_equal(u1, users) and i1.dtype == np.int64 and s1.dtype == np.float32
    assert np.array_equal(i1, top_i) and np.array_equal(s1.view(np.int32), top_s.view(np.int32))
    # pool == k: a permutation of recommend(k)
    _, i2, _ = model.recommend_calibrated(train, k=10, pool=10, trade_off=0.2)
    assert np.array_equal(np.sort(i2, axis=1), np.sort(top_i, axis=1))
    u3, i3, s3 = model.recommend_calibrated(train, k=10, pool=25, trade_off=0.3)
    seen = {(int(u), int(i)) for u, i in np.asarray(train.ratings)[:, :2]}
    assert i3.shape == (nu, 10) and not any((int(u), int(i)) in seen for u, row in zip(u3, i3) for i in row if i >= 0)
    assert all(len(set(row[row >= 0].tolist())) == (row >= 0).sum() for row in i3)
    pick = np.array([nu - 1, 0, 7, 3])
    u4, i4, s4 = model.recommend_calibrated(train, k=10, pool=25, trade_off=0.3, users=pick)
    assert np.array_equal(u4, pick) and np.array_equal(i4, i3[pick]) and np.array_equal(s4.view(np.int32), s3[pick].view(np.int32))
    with rec.device_lists():
        _, i5, s5 = model.recommend_calibrated(train, k=10, pool=25, trade_off=0.3)
        _, pool_i, pool_s = model.recommend(train, k=25)
    assert i5.is_cuda and i5.dtype == torch.int32
    rows = i5.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.where(rows >= 0, rows + nu, -1), i3) and np.array_equal(_bits(s5), s3.view(np.int32))
    # every step against float64 on the device pool
    d = _device_case(((cats[0].astype(np.int32), cats[1].astype(np.int32), cats[3]), liked, pool_i.cpu().numpy(), pool_s.cpu().numpy(),
                      np.arange(nu, dtype=np.int32)))
    out = _rerank(hip, d, G, 10, 0.3, 0.01, users=None, want_value=True, want_kl=True)
    assert np.array_equal(out[0].cpu().numpy(), i5.cpu().numpy())
    worst = ref.check_steps(pool_i.cpu().numpy(), pool_s.cpu().numpy(), np.arange(nu), liked, cats, G, out[0].cpu().numpy(), out[2].cpu().numpy(),
                            out[3].cpu().numpy(), 0.3, 0.01, 10, name, n_items=ni)
    print('{}: max err/tol out_value {:.3f} out_kl {:.3f}'.format(name, *worst))
    # the calibrated lists are no further from the users' tastes than the plain ones, on the host metric
    host = lambda items: miscalibration(np.where(items >= 0, items - nu, -1), users, liked, cats, (10,), 0.01)
    plain_kl, _, support = host(top_i)
    assert host(i3)[0][support > 0].mean() < plain_kl[support > 0].mean()
    # list_calibration: host node ids and device rows against the host metric
    kl, count, sup = model.list_calibration(train, i3, ks=(2, 10))
    want = miscalibration(np.where(i3 >= 0, i3 - nu, -1), users, liked, cats, (2, 10), 0.01)
    assert np.all(np.abs(kl - want[0]) <= 1e-12) and np.array_equal(count, want[1]) and np.array_equal(sup, want[2])
    with rec.device_lists():
        kl_d = model.list_calibration(train, i5, ks=(2, 10))[0]
    assert kl_d.is_cuda and np.array_equal(_bits(kl_d), kl.view(np.int64))
    kl4 = model.list_calibration(train, i4, users=pick, ks=(2, 10), categories=None)[0]
    assert np.array_equal(kl4.view(np.int64), kl[pick].view(np.int64))
    # a membership matrix in place of the graph's properties: the same categories, the same lists
    matrix = np.zeros((ni, G), dtype=np.int8)
    matrix[np.repeat(np.arange(ni), np.diff(cats[0])), cats[1]] = 1
    _, i6, _ = model.recommend_calibrated(train, k=10, pool=25, trade_off=0.3, categories=matrix)
    assert np.array_equal(i6, i3)
    _, i7, _ = model.recommend_calibrated(train, k=10, pool=25, trade_off=0.3, categories=5)
    assert i7.shape == i3.shape
    with pytest.raises(ValueError):
        model.list_calibration(train, np.zeros((nu, 3), dtype=np.int64))                   # user ids are not item node ids
    # evaluate_ranking(calibration=...)
    rng = np.random.default_rng(3)
    test = np.stack([rng.integers(0, nu, 200), rng.integers(nu, nu + ni, 200), rng.integers(0, 2, 200)], axis=1)
    plain = model.evaluate_ranking(train, test, [3, 10])
    both = model.evaluate_ranking(train, test, [3, 10], calibration={'smoothing': 0.01})
    assert set(both) - set(plain) == {'miscalibration_at_3', 'miscalibration_at_10'} and all(repr(both[key]) == repr(plain[key]) for key in plain)
    again = model.evaluate_ranking(train, test, [3, 10])
    assert list(again) == list(plain) and all(repr(again[key]) == repr(plain[key]) for key in plain)
    assert abs(both['miscalibration_at_10'] - plain_kl[support > 0].mean()) <= 1e-12
    some = model.evaluate_ranking(train, test, [10], calibration={'categories': 5, 'smoothing': 0.5}, users=np.array([4, 1, 9]))
    assert 0.0 <= some['miscalibration_at_10'] <= np.log(2.0) + 1e-6


# ---- 3. experiment ---------------------------------------------------------------------------------------------------------
def test_experiment_calibrate_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = ds.props[np.isin(ds.props[:, 0], ds.train[:, 1])]
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    captured = {}
    original = experiment.Experimenter.write_calibrated

    def spy(self, **kwargs):
        captured['exp'] = self
        captured['result'] = original(self, **kwargs)
        return captured['result']

    monkeypatch.setattr(experiment.Experimenter, 'write_calibrated', spy)
    monkeypatch.chdir(tmp_path)
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(paths)
    cfg['dataset']['type_adjacency'] = 'unary-uip'
    cfg['parameters']['epochs'] = 1
    cfg['parameters']['calibrate'] = {'k': 10, 'pool': 40, 'trade_off': 0.5, 'smoothing': 0.01, 'categories': 32}
    (tmp_path / 'cal.yaml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'cal_exps.yaml').write_text(
        "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
        "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
    run_log = setup_mlflow('cal', str(tmp_path / 'mlruns'))
    results = experiment.MultiExperimenter(str(tmp_path / 'cal.yaml'), str(tmp_path / 'cal_exps.yaml'), run_log).run()
    assert all(v is not None for v in results.values())
    runs = glob.glob(str(tmp_path / 'mlruns' / 'cal' / '*'))
    assert len(runs) == 1
    exp, (path, logged) = captured.pop('exp'), captured.pop('result')
    tsv = os.path.join(runs[0], 'artifacts', 'predictions', 'calibrated_top_10.tsv')
    assert os.path.exists(tsv) and os.path.samefile(tsv, path)
    frame = pd.read_csv(tsv, sep='\t', header=None)
    n_users = len(exp.trainset.users)
    assert len(frame) == n_users * 10 and frame.shape[1] == 3
    assert set(frame[0]) == set(np.asarray(exp.trainset.users).tolist()) and set(frame[1]) <= set(np.asarray(exp.trainset.items).tolist())
    users, items, scores = exp.model.recommend_calibrated(exp.trainset, k=10, pool=40, trade_off=0.5, smoothing=0.01, categories=32)
    assert np.array_equal(frame[1].to_numpy(), np.asarray(exp.trainset.items)[items - n_users].reshape(-1))
    assert set(logged) == {'plain_miscalibration_at_10', 'calibrated_miscalibration_at_10'}
    assert 0.0 <= logged['calibrated_miscalibration_at_10'] < logged['plain_miscalibration_at_10']
    on = {}
    for line in open(os.path.join(runs[0], 'run.jsonl')):
        record = json.loads(line)
        if record.get('event') == 'metrics' and 'step' not in record:
            on.update(record['metrics'])
    assert {name: on[name] for name in logged} == logged
