"""GPU: diversified re-ranking (amar_rerank_mmr_f32, amar_list_diversity_f64, recommend_diverse / list_diversity /
evaluate_ranking(diversity=...) and the experiment opt-in) against the float64 restatement of tests/diversify_ref.py (pytest -m gpu).

Tolerances (derived in tests/diversify_ref.py): tol_sim = (d + 8) 2^-24 ||a|| ||b||, tol_v = (1 - lam) tol_sim + 8 2^-24 (lam +
(1 - lam) |sim|).  Whole lists equal the float64 greedy except where a float64 step has a gap to the runner-up within 2 tol_v; at
most MAX_NEAR_TIE_LISTS of the 37 lists may differ that way (the seeds keep the reference itself within that cap:
tests/test_diversify_cpu.py)."""
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import diversify_ref as ref

pytestmark = pytest.mark.gpu


def _table(T, dev):
    """T as a column slice of a wider buffer (ldt > d), and the buffer."""
    import torch
    buf = torch.full((T.shape[0], T.shape[1] + 12), 7.0, dtype=torch.float32, device=dev)
    view = buf[:, 4:4 + T.shape[1]]
    view.copy_(torch.from_numpy(T))
    assert view.stride(0) > T.shape[1]
    return view, buf


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', ref.GRID_D)
@pytest.mark.parametrize('P', ref.GRID_P)
def test_mmr_kernel_against_float64(hip, P, d):
    import torch
    capi = hip
    dev = torch.device('cuda')
    for metric in ref.GRID_METRIC:
        T, pool, scores = ref.planted_case(P, d, metric)
        grid, tol = ref.sim(T, metric), ref.sim_tolerance(T, metric)
        t_d, t_buf = _table(T, dev)
        pool_d, scores_d = _dev(pool, scores)
        for lam in ref.GRID_LAMBDA:
            for k in ref.grid_ks(P):
                label = 'P={} d={} {} lam={} k={}'.format(P, d, metric, lam, k)
                items, sc, mmr, ild = capi.rerank_mmr(pool_d, scores_d, t_d, k, trade_off=lam, metric=metric, want_mmr=True, want_ild=True)
                got_i, got_s, got_v = items.cpu().numpy(), sc.cpu().numpy(), mmr.cpu().numpy()
                assert got_i.dtype == np.int32 and got_i.shape == (ref.M_LISTS, k) and got_s.dtype == np.float32 and not np.isnan(got_v).any()
                worst = ref.check_steps(pool, scores, got_i, got_v, grid, tol, lam, k, label)
                differing = 0
                for j in range(ref.M_LISTS):
                    # out_scores: the pool's own bits of the chosen items
                    for s in range(k):
                        if got_i[j, s] < 0:
                            assert np.isneginf(got_s[j, s])
                        else:
                            at = pool[j].tolist().index(got_i[j, s])
                            assert got_s[j, s].view(np.int32) == scores[j, at].view(np.int32), label
                    want_i, near = ref.greedy_with_near_tie(pool[j], scores[j], grid, tol, lam, k)
                    if not np.array_equal(got_i[j], want_i):
                        assert near, '{}: list {} differs from float64 without a near-tie'.format(label, j)
                        differing += 1
                print('{}: max |out_mmr - v| / tol_v {:.3f}, lists differing by near-ties {}'.format(label, worst, differing))
                assert differing <= ref.MAX_NEAR_TIE_LISTS, label
                # out_ild is amar_list_diversity_f64 of out_items, bit for bit
                ild2, _ = capi.list_diversity(items, t_d, [k], metric=metric)
                assert np.array_equal(_bits(ild), _bits(ild2[:, 0])), label
        assert torch.all(t_buf[:, :4] == 7.0) and torch.all(t_buf[:, 4 + d:] == 7.0)           # the buffer around the slice is untouched


def test_exact_ties_go_to_the_smaller_position(hip):
    """Small-integer vectors under 'dot', dyadic scores and trade-offs: every v is exact in float32, so the lists ARE the float64
    greedy, ties (there are many) resolved by position."""
    T, pool, scores = ref.exact_case()
    grid = ref.sim(T, 'dot')
    t_d, pool_d, scores_d = _dev(T, pool, scores)
    ties = 0
    for lam in (0.0, 0.25, 0.5, 1.0):
        for k in (1, 7, 24):
            items, sc, mmr = hip.rerank_mmr(pool_d, scores_d, t_d, k, trade_off=lam, metric='dot', want_mmr=True)
            got_i, got_v = items.cpu().numpy(), mmr.cpu().numpy()
            for j in range(len(pool)):
                _, want_i, _, want_v, gaps = ref.mmr64(pool[j], scores[j], grid, lam, k)
                assert np.array_equal(got_i[j], want_i), (lam, k, j)
                assert np.array_equal(got_v[j].astype(np.float64), want_v), (lam, k, j)
                ties += int((gaps == 0).sum())
    assert ties > 100


def test_trade_off_one_is_the_score_order(hip):
    T, pool, scores = ref.planted_case(33, 20, 'cosine')
    scores[5, 4] = scores[5, 9]                                          # an exact tie: the smaller position first
    t_d, pool_d, scores_d = _dev(T, pool, scores)
    for k in (1, 10, 33):
        items, sc = hip.rerank_mmr(pool_d, scores_d, t_d, k, trade_off=1.0, metric='cosine')
        got_i, got_s = items.cpu().numpy(), sc.cpu().numpy()
        for j in range(len(pool)):
            n = int((pool[j] >= 0).sum())
            order = np.lexsort((np.arange(n), -scores[j, :n].astype(np.float64)))[:k]
            assert np.array_equal(got_i[j, :len(order)], pool[j, order]) and np.all(got_i[j, len(order):] == -1)
            assert np.array_equal(got_s[j, :len(order)].view(np.int32), scores[j, order].view(np.int32))
            assert np.all(np.isneginf(got_s[j, len(order):]))


@pytest.mark.parametrize('metric', ref.GRID_METRIC)
def test_invariance(hip, metric):
    """A second call, a shuffled subset of the lists and every list alone: the same bits per list."""
    import torch
    T, pool, scores = ref.planted_case(33, 132, metric)
    t_d, pool_d, scores_d = _dev(T, pool, scores)
    call = lambda p, s: [_bits(x) for x in hip.rerank_mmr(p, s, t_d, 10, trade_off=0.3, metric=metric, want_mmr=True, want_ild=True)]
    full = call(pool_d, scores_d)
    assert all(np.array_equal(a, b) for a, b in zip(full, call(pool_d, scores_d)))
    pick = np.random.default_rng(1).permutation(len(pool))[:11]
    idx = torch.from_numpy(pick).cuda()
    assert all(np.array_equal(a[pick], b) for a, b in zip(full, call(pool_d[idx].contiguous(), scores_d[idx].contiguous())))
    for j in (0, 1, 3, len(pool) - 1):
        assert all(np.array_equal(a[j:j + 1], b) for a, b in zip(full, call(pool_d[j:j + 1].contiguous(), scores_d[j:j + 1].contiguous())))


@pytest.mark.parametrize('metric', ref.GRID_METRIC)
@pytest.mark.parametrize('K,d', [(5, 4), (17, 48), (64, 132), (33, 512)])
def test_list_diversity_against_float64(hip, K, d, metric):
    import torch
    T, lists, _ = ref.planted_case(K, d, metric)                          # lists 0 and 1 hold 0 and 1 valid items
    grid, tol = ref.sim(T, metric), ref.sim_tolerance(T, metric)
    t_d, t_buf = _table(T, torch.device('cuda'))
    lists_d, = _dev(lists)
    ks = sorted({1, min(2, K), min(5, K), K})
    ild, count = hip.list_diversity(lists_d, t_d, ks, metric=metric)
    got, cnt = ild.cpu().numpy(), count.cpu().numpy()
    assert got.dtype == np.float64 and cnt.dtype == np.int32 and got.shape == (len(lists), len(ks))
    worst = 0.0
    for j in range(len(lists)):
        for q, k in enumerate(ks):
            want, n = ref.ild64(lists[j, :k], grid)
            assert cnt[j, q] == n
            head = lists[j, :k][lists[j, :k] >= 0].astype(np.int64)
            bound = (tol[np.ix_(head, head)].max() if n >= 2 else 0.0) + 2.0 ** -50 * abs(want)
            assert abs(got[j, q] - want) <= bound, (j, k, got[j, q], want, bound)
            worst = max(worst, abs(got[j, q] - want) / bound if bound else 0.0)
            if n < 2:
                assert got[j, q] == 0.0
    print('K={} d={} {}: max |ild - float64| / bound {:.3f}'.format(K, d, metric, worst))
    again = hip.list_diversity(lists_d, t_d, ks, metric=metric)
    assert np.array_equal(_bits(again[0]), _bits(ild)) and np.array_equal(_bits(again[1]), _bits(count))
    assert torch.all(t_buf[:, :4] == 7.0) and torch.all(t_buf[:, 4 + d:] == 7.0)


def test_refusals_make_no_device_call(hip):
    import ctypes
    import torch
    lib = hip.load()
    T = torch.zeros((10, 520), dtype=torch.float32, device='cuda')
    lists = torch.zeros((3, 65), dtype=torch.int32, device='cuda')
    sc = torch.zeros((3, 65), dtype=torch.float32, device='cuda')
    out_i = torch.zeros((3, 65), dtype=torch.int32, device='cuda')
    out_s = torch.zeros((3, 65), dtype=torch.float32, device='cuda')
    out_d = torch.zeros((3, 8), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    before = lib.amar_last_hip_error()
    ks = (ctypes.c_int32 * 1)(1)
    good = dict(P=16, d=8, k=4, lam=0.5, ldt=520, T=T.data_ptr())
    cases = [(dict(P=65), -2), (dict(d=6), -2), (dict(d=516), -2), (dict(k=17), -2), (dict(lam=1.5), -1), (dict(lam=-0.25), -1),
             (dict(lam=float('nan')), -1), (dict(d=8, ldt=4), -1), (dict(T=None), -1), (dict(k=0), -1), (dict(ldt=522), -2)]
    for change, want in cases:
        a = dict(good, **change)
        got = lib.amar_rerank_mmr_f32(lists.data_ptr(), sc.data_ptr(), 3, a['P'], a['T'], a['ldt'], 10, a['d'], 1, a['lam'], a['k'],
                                      out_i.data_ptr(), out_s.data_ptr(), None, None, None)
        assert got == want, ('mmr', change, got)
        if 'k' in change or 'lam' in change:
            continue
        got = lib.amar_list_diversity_f64(lists.data_ptr(), 3, a['P'], a['T'], a['ldt'], 10, a['d'], 1, ks, 1, out_d.data_ptr(),
                                          out_i.data_ptr(), None)
        assert got == want, ('ild', change, got)
    two = (ctypes.c_int32 * 2)(1, 17)
    assert lib.amar_list_diversity_f64(lists.data_ptr(), 3, 16, T.data_ptr(), 520, 10, 8, 1, two, 2, out_d.data_ptr(), out_i.data_ptr(), None) == -1
    assert lib.amar_list_diversity_f64(lists.data_ptr(), 3, 16, T.data_ptr(), 520, 10, 8, 1, two, 9, out_d.data_ptr(), out_i.data_ptr(), None) == -2
    assert lib.amar_list_diversity_f64(lists.data_ptr(), 3, 16, T.data_ptr(), 520, 10, 8, 1, two, 0, out_d.data_ptr(), out_i.data_ptr(), None) == -1
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert int(out_i.abs().sum()) == 0 and float(out_s.abs().sum()) == 0.0                 # nothing was launched
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    with pytest.raises(NotImplementedError, match='6'):
        rec.rerank_mmr(lists[:, :8], sc[:, :8], torch.zeros((10, 6), device='cuda'), 4)
    with pytest.raises(ValueError):
        rec.rerank_mmr(lists[:, :8], sc[:, :8], T[:, :8], 9)
    with pytest.raises(ValueError):
        rec.rerank_mmr(lists[:, :8], sc[:, :8], T[:, :8], 4, trade_off=1.5)


# ---- 2. models -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['BasicGCN', 'HybridBertGCN', 'BasicRS'])
def test_models_recommend_diverse(hip, name):
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from tests.test_similar_gpu import _fixture, SPACES
    model, train, g = _fixture(name)
    nu, ni = g['n_users'], g['n_items']
    users, top_i, top_s = model.recommend(train, k=10)
    # trade_off = 1: recommend(k) itself
    u1, i1, s1 = model.recommend_diverse(train, k=10, pool=30, trade_off=1.0)
    assert np.array_equal(u1, users) and i1.dtype == np.int64 and s1.dtype == np.float32
    assert np.array_equal(i1, top_i) and np.array_equal(s1.view(np.int32), top_s.view(np.int32))
    # pool == k: a permutation of recommend(k)
    _, i2, _ = model.recommend_diverse(train, k=10, pool=10, trade_off=0.2)
    assert np.array_equal(np.sort(i2, axis=1), np.sort(top_i, axis=1))
    seen = {(int(u), int(i)) for u, i in np.asarray(train.ratings)[:, :2]}
    for space in SPACES[name]:
        for metric in ('cosine', 'dot'):
            label = '{} {} {}'.format(name, space, metric)
            u3, i3, s3 = model.recommend_diverse(train, k=10, pool=40, trade_off=0.5, metric=metric, space=space)
            assert i3.shape == (nu, 10) and not any((int(u), int(i)) in seen for u, row in zip(u3, i3) for i in row if i >= 0), label
            assert all(len(set(row[row >= 0].tolist())) == (row >= 0).sum() for row in i3)
            # a subset of the users in another order: bitwise the rows of the full call
            pick = np.array([nu - 1, 0, 7, 3])
            u4, i4, s4 = model.recommend_diverse(train, k=10, pool=40, trade_off=0.5, metric=metric, space=space, users=pick)
            assert np.array_equal(u4, pick) and np.array_equal(i4, i3[pick]) and np.array_equal(s4.view(np.int32), s3[pick].view(np.int32)), label
            # the device tensors inside device_lists(): the same lists as item rows
            with rec.device_lists():
                _, i5, s5 = model.recommend_diverse(train, k=10, pool=40, trade_off=0.5, metric=metric, space=space)
                _, pool_i, pool_s = model.recommend(train, k=40)
            assert i5.is_cuda and i5.dtype == torch.int32
            rows = i5.cpu().numpy().astype(np.int64)
            assert np.array_equal(np.where(rows >= 0, rows + nu, -1), i3) and np.array_equal(_bits(s5), s3.view(np.int32)), label
            # every step against float64 on the device pool and the model's own item vectors
            emb = model.item_embeddings(train, space=space)
            grid, tol = ref.sim(emb, metric), ref.sim_tolerance(emb, metric)
            out = hip.rerank_mmr(pool_i.contiguous(), pool_s.contiguous(), rec._as_device_matrix(model._item_embeddings(train, space), i5.device, 't'),
                                 10, trade_off=0.5, metric=metric, want_mmr=True)
            assert np.array_equal(out[0].cpu().numpy(), i5.cpu().numpy())
            worst = ref.check_steps(pool_i.cpu().numpy(), pool_s.cpu().numpy(), out[0].cpu().numpy(), out[2].cpu().numpy(), grid, tol, 0.5, 10, label)
            print('{}: max |out_mmr - v| / tol_v {:.3f}'.format(label, worst))
    # list_diversity: host node ids against the host metric
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import intra_list_diversity
    space = SPACES[name][0]
    emb = model.item_embeddings(train, space=space)
    ild, count = model.list_diversity(train, top_i, ks=(2, 10), space=space)
    want, want_n = intra_list_diversity(np.where(top_i >= 0, top_i - nu, -1), emb, (2, 10), 'cosine')
    assert np.array_equal(count, want_n) and np.all(np.abs(ild - want) <= (emb.shape[1] + 8) * ref.U24 + 2.0 ** -50)
    with pytest.raises(ValueError):
        model.list_diversity(train, np.zeros((2, 3), dtype=np.int64), space=space)        # user ids are not item node ids


def test_evaluate_ranking_diversity(hip):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import intra_list_diversity
    from tests.test_similar_gpu import _fixture
    model, train, g = _fixture('BasicGCN')
    nu, ni = g['n_users'], g['n_items']
    rng = np.random.default_rng(3)
    test = np.stack([rng.integers(0, nu, 200), rng.integers(nu, nu + ni, 200), rng.integers(0, 2, 200)], axis=1)
    ks = [3, 10]
    plain = model.evaluate_ranking(train, test, ks)
    both = model.evaluate_ranking(train, test, ks, diversity={'metric': 'cosine', 'space': 'graph'})
    assert set(both) - set(plain) == {'ild_at_3', 'item_coverage_at_3', 'ild_at_10', 'item_coverage_at_10'}
    assert all(repr(both[key]) == repr(plain[key]) for key in plain)
    again = model.evaluate_ranking(train, test, ks)
    assert list(again) == list(plain) and all(repr(again[key]) == repr(plain[key]) for key in plain)
    _, items, _ = model.recommend(train, k=10)
    emb = model.item_embeddings(train, space='graph')
    rows = np.where(items >= 0, items - nu, -1)
    ild, count = intra_list_diversity(rows, emb, ks, 'cosine')
    for q, k in enumerate(ks):
        has = count[:, q] >= 2
        assert abs(both['ild_at_{}'.format(k)] - ild[has, q].mean()) <= (emb.shape[1] + 8) * ref.U24 + 2.0 ** -50
        head = rows[:, :k]
        assert both['item_coverage_at_{}'.format(k)] == len(set(head[head >= 0].tolist())) / float(ni)
    dot = model.evaluate_ranking(train, test, ks, diversity={'metric': 'dot'}, users=np.array([4, 1, 9]))
    assert 'ild_at_10' in dot and 0 < dot['item_coverage_at_10'] <= 30.0 / ni


# ---- 3. experiment ---------------------------------------------------------------------------------------------------------
def test_experiment_diversify_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    captured = {}
    original = experiment.Experimenter.write_diverse

    def spy(self, **kwargs):
        captured['exp'] = self
        captured['result'] = original(self, **kwargs)
        return captured['result']

    monkeypatch.setattr(experiment.Experimenter, 'write_diverse', spy)
    monkeypatch.chdir(tmp_path)

    def run(name, diversify):
        cfg = json.loads(json.dumps(BASE_CONFIG))
        cfg['dataset'].update(paths)
        cfg['parameters']['epochs'] = 1
        if diversify:
            cfg['parameters']['diversify'] = diversify
        (tmp_path / (name + '.yaml')).write_text(yaml.safe_dump(cfg))
        (tmp_path / (name + '_exps.yaml')).write_text(
            "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
            "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
        run_log = setup_mlflow(name, str(tmp_path / 'mlruns'))
        results = experiment.MultiExperimenter(str(tmp_path / (name + '.yaml')), str(tmp_path / (name + '_exps.yaml')), run_log).run()
        assert all(v is not None for v in results.values())
        runs = glob.glob(str(tmp_path / 'mlruns' / name / '*'))
        assert len(runs) == 1
        return runs[0]

    run_on = run('with_key', {'k': 10, 'pool': 40, 'trade_off': 0.5, 'metric': 'cosine', 'space': 'graph'})
    exp, (path, logged) = captured.pop('exp'), captured.pop('result')
    tsv = os.path.join(run_on, 'artifacts', 'predictions', 'diverse_top_10.tsv')
    assert os.path.exists(tsv) and os.path.samefile(tsv, path)
    frame = pd.read_csv(tsv, sep='\t', header=None)
    n_users = len(exp.trainset.users)
    assert len(frame) == n_users * 10 and frame.shape[1] == 3
    assert set(frame[0]) == set(np.asarray(exp.trainset.users).tolist()) and set(frame[1]) <= set(np.asarray(exp.trainset.items).tolist())
    users, items, scores = exp.model.recommend_diverse(exp.trainset, k=10, pool=40, trade_off=0.5, metric='cosine', space='graph')
    assert np.array_equal(frame[1].to_numpy(), np.asarray(exp.trainset.items)[items - n_users].reshape(-1))
    assert set(logged) == {p + n for p in ('plain_', 'diverse_') for n in ('ild_at_10', 'item_coverage_at_10')}
    assert all(0.0 <= logged[p + 'item_coverage_at_10'] <= 1.0 for p in ('plain_', 'diverse_'))
    # the run's own log holds both metric pairs, with the values write_diverse returned
    def logged_metrics(root):
        out = {}
        for line in open(os.path.join(root, 'run.jsonl')):
            record = json.loads(line)
            if record.get('event') == 'metrics' and 'step' not in record:
                out.update(record['metrics'])
        return out

    on = logged_metrics(run_on)
    assert {name: on[name] for name in logged} == logged
    run_off = run('without_key', None)
    assert 'exp' not in captured
    rel = lambda root: sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, '**', '*'), recursive=True) if os.path.isfile(p))
    assert rel(run_off) == [p for p in rel(run_on) if 'diverse' not in p]
    # without the key: the same seeded run, so the same metric values (wall-clock times aside) and the same prediction files
    off = logged_metrics(run_off)
    assert set(off) == set(on) - set(logged)
    assert all(off[name] == on[name] for name in off if 'time' not in name), {n: (off[n], on[n]) for n in off if off[n] != on[n]}
    for path_off in glob.glob(os.path.join(run_off, 'artifacts', 'predictions', '**', '*'), recursive=True):
        if os.path.isfile(path_off):
            path_on = os.path.join(run_on, os.path.relpath(path_off, run_off))
            assert open(path_off, 'rb').read() == open(path_on, 'rb').read(), path_off
