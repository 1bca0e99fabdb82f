"""GPU: exact full-catalogue positions (`rank_items()`, amar_rank_of_f32) and the cut-off-free metrics from them
(`evaluate_ranking(rank_metrics=...)`, amar_rank_of_metrics_f64) against the numpy reference of tests/rank_of_ref.py — the kernel
on every template form, slicing, independence, `recommend` itself, the metrics kernel, the models' two routes, fit() and the
experiment surface (pytest -m gpu).

The counts and the scores' bits are compared exactly.  The scores S come bitwise from code that this feature does not touch:
capi.recommend over windows of at most 64 items (k = 64, no exclusion)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import helpers
from tests import rank_of_ref as ref
from tests.test_group_recommend_gpu import _Train, _bits, _csr, _dev, _model_case, _score_matrix

pytestmark = pytest.mark.gpu

HEADS = [(16, [16]), (32, [32, 40, 32]), (64, [64, 24]), (128, [128])]                    # MAXT 1, 2, 4, 8


def _head(capi, rng, c1, hidden, n_users, n_items):
    import torch
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
        ti[n_items // 2] = ti[1]                          # duplicated rows: exact ties below and above a target
        ti[n_items - 1] = ti[1]
    tu[2] *= 1.0e6                                        # this user's scores saturate
    blob, _ = capi.chain_pack([w for w, _ in layers], [b for _, b in layers])
    return torch.from_numpy(blob).cuda(), torch.from_numpy(tu).cuda(), torch.from_numpy(ti).cuda(), dims, acts


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    return (np.array_equal(_bits(got[0]), _bits(want[0])) and all(np.array_equal(np.asarray(g, dtype=np.int64), w) for g, w in zip(got[1:], want[1:]))
            and all(g.dtype == np.int32 for g in got[1:]) and got[0].dtype == np.float32)


def _largest_slices(capi, m, n_items, dims):
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    lib = capi.load()
    return max(s for s in range(1, 65) if lib.amar_rank_of_slices(m, n_items, dims_c, len(dims) - 1, s) == s)


# ---- 1. the kernel against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items', [1, 17, 1100])
@pytest.mark.parametrize('c1,hidden', HEADS)
def test_kernel_against_reference(hip, c1, hidden, n_items):
    capi = hip
    rng = np.random.default_rng(9000 * c1 + n_items + helpers.seed_offset())
    n_users, T = 37, capi.RANK_OF_MAX_TARGETS
    blob, tu_d, ti_d, dims, acts = _head(capi, rng, c1, hidden, n_users, n_items)
    S = _score_matrix(capi, tu_d, ti_d, blob, dims, acts)
    if n_items >= 17:
        assert len(np.unique(S[2])) < n_items // 2                                      # saturated: many exactly equal scores
    perm = rng.permutation(n_users)
    perm = np.concatenate([perm[perm != 2][:35], [2]])                                  # the saturated user is listed
    users = np.concatenate([perm, perm[3:4]])                                           # a shuffled subset with a repeat: 37 entries, 16 + 16 + 5
    pick = lambda n: sorted(rng.choice(n_items, size=min(n_items, n), replace=False).tolist())
    targets = [pick(int(rng.integers(0, 13))) for _ in users]
    targets[0], targets[1] = [], pick(1)
    targets[2], targets[3] = pick(T), pick(T + 1)                                       # a full entry; one more: the binding splits it
    targets[7] = sorted(set(pick(5)) | {1 % n_items, n_items // 2})                     # the tied rows themselves
    targets[35] = pick(20)                                                              # the saturated user
    excl = [set(rng.choice(n_items, size=min(n_items, int(rng.integers(0, 40))), replace=False).tolist()) for _ in range(n_users)]
    excl[users[4]] |= set(targets[4][:1]) if targets[4] else {0}                        # a target inside the exclusion row
    targets[4] = sorted(set(targets[4]) | {min(excl[users[4]])})
    excl[users[5]] = set(range(n_items))                                                # everything excluded
    targets[5] = pick(3)
    targets[6] = pick(4)
    excl[users[6]] = set(range(n_items)) - set(targets[6])                              # everything but the targets
    excl[users[8]] = set()
    t_ptr, t_items = _csr(targets)
    e_ptr, e_items = _csr(excl)
    ep_d, ei_d = _dev(e_ptr), _dev(e_items)
    args = (tu_d, ti_d, blob, dims, acts, 'relu')

    got = _host(capi.rank_of(*args, users, t_ptr, t_items, excl_ptr=ep_d, excl_items=ei_d))
    want = ref.rank_of(S, users, excl, targets)
    assert _same(got, want)
    lo5, hi5 = t_ptr[5], t_ptr[6]
    assert (got[1][lo5:hi5] == 0).all() and (got[2][lo5:hi5] == 0).all() and (got[3][lo5:hi5] == 0).all()
    # the same bits on a second run
    assert _same(_host(capi.rank_of(*args, users, t_ptr, t_items, excl_ptr=ep_d, excl_items=ei_d)), want)
    # exclusion off: every item is a candidate
    free = _host(capi.rank_of(*args, users, t_ptr, t_items))
    assert _same(free, ref.rank_of(S, users, None, targets))
    assert np.array_equal(free[1] + free[2] + free[3] + 1 <= n_items, np.ones(len(t_items), dtype=bool))
    # any item slicing gives the same arrays (the entries the library sees: after the binding's split)
    m_split = len(capi.rank_of_entries(users, t_ptr)[0])
    for slices in sorted({1, _largest_slices(capi, m_split, n_items, dims)}):
        sliced = _host(capi.rank_of(*args, users, t_ptr, t_items, excl_ptr=ep_d, excl_items=ei_d, n_slices=slices))
        assert _same(sliced, got), slices
    # an entry alone: bitwise its part of the full call
    for j in (1, 2, 3, 4, 7, 35, 36):
        one_ptr, one_items = _csr([targets[j]])
        alone = _host(capi.rank_of(*args, users[j:j + 1], one_ptr, one_items, excl_ptr=ep_d, excl_items=ei_d))
        assert _same(alone, tuple(g[t_ptr[j]:t_ptr[j + 1]] for g in got)), j
    # more than RANK_OF_MAX_TARGETS in one entry is the library's refusal
    if n_items > T:
        with pytest.raises(capi.AmarError):
            capi.rank_of(*args, users[3:4], *_csr([targets[3]]), split=False)
    # nothing listed, nothing asked: nothing launched
    for nothing in (capi.rank_of(*args, [], [0], []), capi.rank_of(*args, [4, 5], [0, 0, 0], [])):
        assert all(tuple(t.shape) == (0,) for t in nothing)


def test_refusals(hip):
    import torch
    capi = hip
    blob, _ = capi.chain_pack([np.eye(16, dtype=np.float32), np.ones((16, 1), dtype=np.float32)],
                              [np.zeros(16, dtype=np.float32), np.zeros(1, dtype=np.float32)])
    blob = torch.from_numpy(blob).cuda()
    tu, ti = torch.zeros((4, 16), device='cuda'), torch.zeros((9, 16), device='cuda')
    args = (tu, ti, blob, [16, 16, 1], ['relu', 'sigmoid'], 'relu')
    with pytest.raises(ValueError):
        capi.rank_of(*args, [0], [0, 1], [2], excl_ptr=_dev([0, 0, 0]), excl_items=_dev([]))       # not n_users + 1 pointers
    with pytest.raises(ValueError):
        capi.rank_of(*args, [0], [0, 1], [2], excl_ptr=_dev([0, 0, 0, 0, 0]))
    with pytest.raises(ValueError):
        capi.rank_of(*args, [0], [0, 1], [2], n_slices=7)                                           # not a count the library launches
    lib = capi.load()
    f, i = ctypes.c_void_p(tu.data_ptr()), ctypes.c_void_p(_dev([0, 1]).data_ptr())
    dims, acts = (ctypes.c_int32 * 3)(16, 16, 1), (ctypes.c_int32 * 2)(1, 2)
    call = lambda **kw: lib.amar_rank_of_f32(*[kw.get(name, default) for name, default in (
        ('Tu', f), ('ldu', 16), ('n_users', 4), ('Ti', ctypes.c_void_p(ti.data_ptr())), ('ldi', 16), ('n_items', 9), ('c1', 16),
        ('wpack', ctypes.c_void_p(blob.data_ptr())), ('dims', dims), ('acts', acts), ('n_layers', 2), ('in_act', 1), ('users', i), ('m', 1),
        ('excl_ptr', None), ('excl_items', None), ('tgt_ptr', i), ('tgt_items', i), ('n_targets', 1), ('max_targets', 1), ('n_slices', 0),
        ('out_scores', f), ('out_greater', i), ('out_before', i), ('out_after', i), ('stream', None))])
    assert call(Tu=None) == -1 and call(tgt_ptr=None) == -1 and call(tgt_items=None) == -1 and call(out_greater=None) == -1
    assert call(m=-1) == -1 and call(n_targets=-1) == -1 and call(excl_ptr=i) == -1 and call(users=None) == -1
    assert call(max_targets=capi.RANK_OF_MAX_TARGETS + 1) == -2
    assert call(m=0, users=None, n_users=0) == 0 and call(n_targets=0, tgt_items=None) == 0


# ---- 2. against recommend() itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c1,hidden', HEADS)
def test_positions_are_recommends(hip, c1, hidden):
    capi = hip
    rng = np.random.default_rng(31 * c1 + helpers.seed_offset())
    n_users, n_items = 21, 60
    blob, tu_d, ti_d, dims, acts = _head(capi, rng, c1, hidden, n_users, n_items)
    excl = [set(rng.choice(n_items, size=int(rng.integers(0, 30)), replace=False).tolist()) for _ in range(n_users)]
    e_ptr, e_items = _csr(excl)
    ep_d, ei_d = _dev(e_ptr), _dev(e_items)
    lists, list_scores = capi.recommend(tu_d, ti_d, blob, dims, acts, 'relu', 64, excl_ptr=ep_d, excl_items=ei_d)
    lists, list_scores = lists.cpu().numpy(), list_scores.cpu().numpy()
    t_ptr = np.arange(n_users + 1) * n_items
    t_items = np.tile(np.arange(n_items), n_users)
    scores, greater, before, _ = _host(capi.rank_of(tu_d, ti_d, blob, dims, acts, 'relu', np.arange(n_users), t_ptr, t_items,
                                                     excl_ptr=ep_d, excl_items=ei_d))
    rank = (1 + greater + before).reshape(n_users, n_items)
    scores = scores.reshape(n_users, n_items)
    for u in range(n_users):
        listed = lists[u][lists[u] >= 0]
        assert sorted(listed.tolist()) == sorted(set(range(n_items)) - excl[u])
        assert np.array_equal(rank[u][listed], np.arange(1, len(listed) + 1)), u
        assert np.array_equal(_bits(scores[u][listed]), _bits(list_scores[u][:len(listed)])), u


# ---- 3. the metrics kernel ---------------------------------------------------------------------------------------------------------
def test_metrics_kernel_against_reference(hip):
    capi = hip
    rng = np.random.default_rng(77 + helpers.seed_offset())
    n_users, n_items = 37, 300
    blob, tu_d, ti_d, dims, acts = _head(capi, rng, 16, [16], n_users, n_items)
    S = _score_matrix(capi, tu_d, ti_d, blob, dims, acts)
    excl = [set(rng.choice(n_items, size=int(rng.integers(0, 120)), replace=False).tolist()) for _ in range(n_users)]
    relevant = [set(rng.choice(n_items, size=int(rng.integers(1, 90)), replace=False).tolist()) for _ in range(n_users)]
    relevant[5] = set()                                                                 # nothing held out
    excl[6] = set(range(n_items))                                                       # no candidate
    excl[7] = set(range(n_items)) - {3, 8, 200}
    relevant[7] = {3, 8, 200}                                                           # no candidate that is not a target
    relevant[8] = set(rng.choice(n_items, size=150, replace=False).tolist())            # more than two entries' worth
    users = rng.permutation(n_users)
    targets = [sorted(relevant[u] - excl[u]) for u in users]
    t_ptr, t_items = _csr(targets)
    e_ptr, e_items = _csr(excl)
    flat = capi.rank_of(tu_d, ti_d, blob, dims, acts, 'relu', users, t_ptr, t_items, excl_ptr=_dev(e_ptr), excl_items=_dev(e_items))
    assert _same(_host(flat), ref.rank_of(S, users, excl, targets))
    n_cand = np.array([n_items - len(excl[u]) for u in users])
    out, valid = capi.rank_of_metrics(*flat, _dev(t_ptr), _dev(n_cand))
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    want = [ref.metrics(S[u], excl[u], relevant[u]) for u in users]
    assert out.dtype == np.float64 and valid.dtype == np.int32
    assert valid.tolist() == [int(w[3]) for w in want] and not valid[np.isin(users, [5, 6, 7])].any() and valid.sum() > 20
    assert np.abs(out - np.array([w[:3] for w in want])).max() <= 1e-12
    assert (out[valid == 0] == 0).all()
    again, again_valid = capi.rank_of_metrics(*flat, _dev(t_ptr), _dev(n_cand))
    assert np.array_equal(again.cpu().numpy().view(np.int64), out.view(np.int64)) and np.array_equal(again_valid.cpu().numpy(), valid)
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_rank_metrics
    host, host_valid = full_ranking_rank_metrics(S[users], [relevant[u] for u in users], [excl[u] for u in users], per_user=True)
    assert host_valid.tolist() == (valid > 0).tolist() and np.abs(out - host).max() <= 1e-12
    nobody, nobody_valid = capi.rank_of_metrics(*(t[:0] for t in flat), _dev([0]), _dev([]))
    assert tuple(nobody.shape) == (0, 3) and tuple(nobody_valid.shape) == (0,)


# ---- 4. the models -------------------------------------------------------------------------------------------------------------------
def _held_out(g, rng, n=300):
    nu, ni = g['n_users'], g['n_items']
    keys = rng.choice(nu * ni, size=n, replace=False)
    return np.stack([keys // ni, keys % ni + nu, rng.integers(0, 2, size=n)], axis=1).astype(np.int64)


@pytest.mark.parametrize('name', ['BasicGCN', 'HybridCBRS'])
def test_models(hip, name, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics_device, full_ranking_rank_metrics
    capi = hip
    model, train, g, route = _model_case(name)
    nu, ni = g['n_users'], g['n_items']
    calls = {'fused': 0}
    fused = capi.rank_of
    monkeypatch.setattr(capi, 'rank_of', lambda *a, **kw: (calls.__setitem__('fused', calls['fused'] + 1), fused(*a, **kw))[1])
    _, all_items, all_scores = model.recommend(train, k=ni, exclude_seen=False)
    S = np.zeros((nu, ni), dtype=np.float32)
    S[np.arange(nu)[:, None], all_items - nu] = all_scores
    seen = [set() for _ in range(nu)]
    for u, i, _ in g['ratings'].tolist():
        seen[u].add(i - nu)
    k = 10
    _, items, scores = model.recommend(train, k=k)
    pairs_u, pairs_i = np.repeat(np.arange(nu), ni), np.tile(np.arange(ni) + nu, nu)
    order = np.random.default_rng(1).permutation(nu * ni)                               # the caller's order, with a pair asked twice
    order = np.concatenate([order, order[:5]])
    out = model.rank_items(train, pairs_u[order], pairs_i[order])
    assert calls['fused'] == (1 if route == 'fused' else 0)                              # a head that fell back would show up here
    assert sorted(out) == sorted(rec.RANK_ITEMS_KEYS) and all(len(v) == len(order) for v in out.values())
    assert np.array_equal(out['rank'][-5:], out['rank'][:5])
    back = np.empty(nu * ni, dtype=np.int64)
    back[order[:nu * ni]] = np.arange(nu * ni)
    rank, score, ties, cand, pct = (out[key][:nu * ni][back].reshape(nu, ni) for key in rec.RANK_ITEMS_KEYS)
    assert np.array_equal(_bits(score), _bits(S))                                       # filled for seen items too
    for u in range(nu):
        listed = items[u][items[u] >= 0] - nu
        assert np.array_equal(rank[u][listed], np.arange(1, len(listed) + 1)), u
        assert np.array_equal(_bits(score[u][listed]), _bits(scores[u][:len(listed)]))
        unseen = np.array(sorted(set(range(ni)) - seen[u]), dtype=np.int64)
        assert (rank[u][np.array(sorted(seen[u]), dtype=np.int64)] == 0).all() and (rank[u][unseen] >= 1).all()
        assert (rank[u][np.setdiff1d(unseen, listed)] > k).all()
        assert sorted(rank[u][unseen].tolist()) == list(range(1, len(unseen) + 1))
        assert (cand[u] == len(unseen)).all()
        want = ref.counts(S[u], seen[u], list(range(ni)))
        assert np.array_equal(ties[u], want[2] + want[3])
        assert np.array_equal(pct[u][unseen], 1.0 - (rank[u][unseen] - 1) / float(len(unseen))) and np.isnan(pct[u][sorted(seen[u])]).all()
    everything = model.rank_items(train, pairs_u, pairs_i, exclude_seen=False)
    assert (everything['rank'] >= 1).all() and (everything['candidates'] == ni).all()
    # evaluate_ranking(rank_metrics=...) against the host restatement on the model's own dense scores
    test = _held_out(g, np.random.default_rng(2))
    relevant = [set() for _ in range(nu)]
    for u, i, y in test.tolist():
        if y == 1:
            relevant[u].add(i - nu)
    plain = model.evaluate_ranking(train, test, [5, 10])
    with rec.device_lists():                                                            # the call path of the parent commit
        u_old, lists_old, _ = model.recommend(train, k=10, users=None, exclude_seen=True)
    assert plain == full_ranking_metrics_device(None, lists_old.contiguous(), test, [5, 10], nu, ni)
    assert not any(key in plain for key in ('auc', 'mrr', 'map', 'rank_metrics_users'))
    both = model.evaluate_ranking(train, test, [5, 10], rank_metrics=('auc', 'mrr', 'map'))
    assert {key: both[key] for key in plain} == plain
    want = full_ranking_rank_metrics(S, relevant, seen)
    for key in ('auc', 'mrr', 'map'):
        assert abs(both[key] - want[key]) <= 1e-12, key
    assert both['rank_metrics_users'] == want['rank_metrics_users']
    only = model.evaluate_ranking(train, test, [], rank_metrics=['map'])
    assert sorted(only) == ['map', 'rank_metrics_users'] and only['map'] == both['map']
    sub = np.array([7, 3, 3, 30])
    part = model.evaluate_ranking(train, test, [], users=sub, exclude_seen=False, rank_metrics=['auc', 'mrr'])
    want = full_ranking_rank_metrics(S[sub], [relevant[u] for u in sub], None)
    assert abs(part['auc'] - want['auc']) <= 1e-12 and abs(part['mrr'] - want['mrr']) <= 1e-12
    assert part['rank_metrics_users'] == want['rank_metrics_users']
    with pytest.raises(ValueError):
        model.evaluate_ranking(train, test, [5], rank_metrics=['ndcg'])
    # no side effects: recommend() returns the bits it returned before
    _, items2, scores2 = model.recommend(train, k=k)
    assert np.array_equal(items, items2) and np.array_equal(_bits(scores), _bits(scores2))


def test_fit_reports_val_auc_and_leaves_training_bit_for_bit(hip):
    import torch
    from deep_cbrs_amar_renaissance_amd.utilities.keras import EarlyStopping
    from tests.test_validation_gpu import _bce_model, _bce_sequence, _validation_args
    models, hists = [], []
    for validated in (False, True):
        g, seq = _bce_sequence(shuffle=True)
        model = _bce_model(g, 'BasicGCN')
        kwargs = {}
        if validated:
            _, ranking, test = _validation_args(g)
            ranking = dict(ranking, ks=[], rank_metrics=['auc'])
            kwargs = dict(validation_ranking=ranking, callbacks=[EarlyStopping(monitor='val_auc', mode='max', patience=5)])
        hists.append(model.fit(seq, epochs=1, verbose=False, **kwargs))
        models.append(model)
    assert hists[0]['loss'] == hists[1]['loss']
    assert len(hists[1]['val_auc']) == 1 and 0.0 <= hists[1]['val_auc'][0] <= 1.0
    assert not any(key.startswith('val_') for key in hists[0]) and 'val_rank_metrics_users' not in hists[1]
    assert hists[1]['val_auc'][0] == models[1].evaluate_ranking(ranking['trainset'], test, [], rank_metrics=['auc'])['auc']
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pa, pb), name
    with pytest.raises(ValueError):
        models[0].fit(seq, epochs=1, verbose=False, validation_ranking=dict(ranking, rank_metrics=['recall']))


# ---- 5. the experiment surface -----------------------------------------------------------------------------------------------------
def test_experiment_logs_rank_metrics(hip, tmp_path, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    logged = {}
    monkeypatch.chdir(tmp_path)

    def run(name, names):
        cfg = json.loads(json.dumps(BASE_CONFIG))
        cfg['dataset'].update(paths)
        cfg['parameters']['epochs'] = 1
        cfg['parameters']['full_ranking_rank_metrics'] = names
        (tmp_path / (name + '.yaml')).write_text(yaml.safe_dump(cfg))
        (tmp_path / (name + '_exps.yaml')).write_text(
            "linear:\n  gcn:\n    model:\n      name: basic.BasicGCN\n      embedding_dim: 8\n      n_hiddens: [8, 8]\n"
            "      dense_units: [24, 24]\n      clf_units: [48, 48]\n    dataset:\n      load_function_name: load_user_item_graph\n")
        run_log = setup_mlflow(name, str(tmp_path / 'mlruns'))
        original = run_log.log_metrics
        monkeypatch.setattr(run_log, 'log_metrics', lambda metrics, *a, **kw: (logged.update(metrics), original(metrics, *a, **kw))[1])
        multi = experiment.MultiExperimenter(str(tmp_path / (name + '.yaml')), str(tmp_path / (name + '_exps.yaml')), run_log)
        return multi.run()

    assert all(v is not None for v in run('with_key', ['auc', 'map']).values())
    assert 0.0 <= logged['full_auc'] <= 1.0 and 0.0 < logged['full_map'] <= 1.0 and 'full_mrr' not in logged
    assert logged['full_rank_metrics_users_evaluated'] > 0 and 'full_rank_metrics_users_skipped' in logged
    assert glob.glob(str(tmp_path / 'mlruns' / 'with_key' / '*'))
    logged.clear()
    assert all(v is None for v in run('bad_key', ['auc', 'ndcg']).values())               # the ValueError fails the experiment
    assert 'full_auc' not in logged
