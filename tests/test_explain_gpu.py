"""GPU: explanations (amar_explain_f32, capi.explain, model.explain) against the float64 restatement of tests/explain_ref.py
(pytest -m gpu).

Tolerances (derived in tests/explain_ref.py): tol_sim = (d + 8) 2^-24 ||a|| ||b||, tol_p = w_p sum_j tol_sim + (n_j + 2) 2^-24
|score|.  Whole rankings equal the float64 ones except at entries the reference marks as near-ties (a gap to a neighbour, at or
across the cut, within 2 tol); at most 2 % of a case's written entries may be such (the seeds keep the reference itself within that
cap: tests/test_explain_cpu.py).  Supports are exact."""
import numpy as np
import pytest

from tests import explain_ref as ref

pytestmark = pytest.mark.gpu


def _table(T, dev='cuda'):
    """T as a column slice of a wider buffer (ldt > d), and the buffer."""
    import torch
    buf = torch.full((T.shape[0], T.shape[1] + 12), 7.0, dtype=torch.float32, device=dev)
    view = buf[:, 4:4 + T.shape[1]]
    view.copy_(torch.from_numpy(T))
    assert view.stride(0) > T.shape[1]
    return view, buf


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _device_case(case):
    lp, li = ref.csr(case['liked'])
    pp, pi = ref.csr(case['prop_rows'])
    view, buf = _table(case['T'])
    return {'lists': _dev(case['lists'], np.int32), 'users': _dev(case['users'], np.int32), 'liked_ptr': _dev(lp, np.int32),
            'liked_items': _dev(li, np.int32), 'T': view, 'buf': buf, 'prop_ptr': _dev(pp, np.int32), 'prop_ids': _dev(pi, np.int32),
            'weight': _dev(case['weight'], np.float32), 'max_prop_row': case['max_prop_row']}


def _run(hip, dc, E, Q, metric, lists=None, users='given'):
    props = dict(prop_ptr=dc['prop_ptr'], prop_ids=dc['prop_ids'], prop_weight=dc['weight'], max_prop_row=dc['max_prop_row']) if Q else {}
    out = hip.explain(dc['lists'] if lists is None else lists, dc['liked_ptr'], dc['liked_items'], dc['T'], E, Q, metric=metric,
                      users=dc['users'] if isinstance(users, str) else users, **props)
    return [t.cpu().numpy() for t in out]


def _check(case, got, refs, metric, E, Q, label, exact=False):
    """The rules of the module docstring over every (list, target); returns (entries that differ from float64, written entries)."""
    ev, es, pr, ps, pc = got
    grid, tol = ref.sim_grid(case['T'], metric), ref.sim_tolerance(case['T'], metric)
    differ = entries = 0
    worst_s = worst_p = 0.0
    for j, per_list in enumerate(refs):
        liked = set(case['liked'][case['users'][j]].tolist())
        for t, r in enumerate(per_list):
            where = '{} list {} target {}'.format(label, j, t)
            want = ref.padded(r, E, Q)
            n = int((want[0] >= 0).sum())
            assert np.all(ev[j, t, n:] == -1) and np.all(np.isneginf(es[j, t, n:])), where
            assert np.all(ev[j, t, :n] >= 0), where
            nq = int((want[2] >= 0).sum())
            if Q:
                assert np.all(pr[j, t, nq:] == -1) and np.all(np.isneginf(ps[j, t, nq:])) and np.all(pc[j, t, nq:] == 0), where
                assert np.all(pr[j, t, :nq] >= 0), where
            if r is None:
                continue
            i = int(case['lists'][j, t])
            items = ev[j, t, :n].tolist()
            assert len(set(items)) == n and i not in items and set(items) <= liked, where
            for q in range(n):
                err = abs(float(es[j, t, q]) - grid[i, items[q]])
                assert err <= tol[i, items[q]], (where, q, err, tol[i, items[q]])
                worst_s = max(worst_s, err / tol[i, items[q]]) if tol[i, items[q]] > 0 else worst_s
                if q:
                    assert es[j, t, q - 1] > es[j, t, q] or (es[j, t, q - 1] == es[j, t, q] and items[q - 1] < items[q]), where
                if items[q] != want[0][q]:
                    assert not exact and r['ev_flag'][q], (where, q, items, want[0])
                    differ += 1
            entries += n
            if exact:
                assert np.array_equal(es[j, t, :n].astype(np.float64), want[1][:n]), where
            if not Q:
                continue
            props = pr[j, t, :nq].tolist()
            assert len(set(props)) == nq and set(props) <= set(r['prop_ids'].tolist()), where
            for q in range(nq):
                p = props[q]
                assert pc[j, t, q] == r['support_of'][p] > 0, (where, q)
                err = abs(float(ps[j, t, q]) - r['score_of'][p])
                assert err <= r['tol_of'][p], (where, q, err, r['tol_of'][p])
                worst_p = max(worst_p, err / r['tol_of'][p]) if r['tol_of'][p] > 0 else worst_p
                if q:
                    assert ps[j, t, q - 1] > ps[j, t, q] or (ps[j, t, q - 1] == ps[j, t, q] and props[q - 1] < p), where
                if p != want[2][q]:
                    assert not exact and r['prop_flag'][q], (where, q, props, want[2])
                    differ += 1
            entries += nq
            if exact:
                assert np.array_equal(ps[j, t, :nq].astype(np.float64), want[3][:nq]), where
    print('{}: {} of {} entries differ from float64, max err / tol: sim {:.3f}, score {:.3f}'.format(label, differ, entries, worst_s, worst_p))
    assert differ <= ref.NEAR_TIE_CAP * max(entries, 1), (label, differ, entries)
    return differ, entries


# ---- 1. the kernel grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ref.GRID_METRIC)
@pytest.mark.parametrize('K', ref.GRID_K)
@pytest.mark.parametrize('d', ref.GRID_D)
def test_kernel_against_float64(hip, d, K, metric):
    case = ref.kernel_case(d, K, metric)
    dc = _device_case(case)
    refs = ref.case_reference(case, metric, 16, 16)                    # a smaller cut reads a prefix of the same rankings and flags
    for E, Q in ref.GRID_EQ:
        got = _run(hip, dc, E, Q, metric)
        assert got[0].shape == (ref.M_LISTS, K, E) and got[2].shape == (ref.M_LISTS, K, Q)
        _check(case, got, refs, metric, E, Q, 'd={} K={} {} E={} Q={}'.format(d, K, metric, E, Q))
    buf = dc['buf'].cpu().numpy()
    assert np.all(buf[:, :4] == 7.0) and np.all(buf[:, 4 + d:] == 7.0) and np.array_equal(buf[:, 4:4 + d], case['T'])


# ---- 2. the exact case ---------------------------------------------------------------------------------------------------
def test_exact_case_is_bitwise_and_ties_go_by_index(hip):
    case = ref.exact_case()
    dc = _device_case(case)
    E = Q = 16
    refs = ref.case_reference(case, 'dot', E, Q)
    got = _run(hip, dc, E, Q, 'dot')
    differ, entries = _check(case, got, refs, 'dot', E, Q, 'exact', exact=True)
    assert differ == 0
    ties = sum(int((np.diff(r['ev_sims'][:E]) == 0).sum()) + int((np.diff(r['prop_scores'][:Q]) == 0).sum())
               for per_list in refs for r in per_list if r is not None)
    assert ties > 100, ties


# ---- 3. independence and repeatability -----------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ref.GRID_METRIC)
def test_independence_and_repeatability(hip, metric):
    import torch
    case = ref.kernel_case(20, 17, metric)
    dc = _device_case(case)
    bits = lambda outs: [a.view(np.int32) if a.dtype == np.float32 else a for a in outs]
    full = bits(_run(hip, dc, 3, 3, metric))
    again = bits(_run(hip, dc, 3, 3, metric))
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    pick = np.array([30, 2, 17, 9, 36, 0])
    sub = bits(_run(hip, dc, 3, 3, metric, lists=dc['lists'][torch.from_numpy(pick).cuda()].contiguous(),
                    users=dc['users'][torch.from_numpy(pick).cuda()].contiguous()))
    assert all(np.array_equal(a[pick], b) for a, b in zip(full, sub))
    # users == NULL with one list per user equals the explicit identity
    ident = torch.arange(ref.N_USERS, dtype=torch.int32, device='cuda')
    lists = dc['lists'][:ref.N_USERS].contiguous()
    a = bits(_run(hip, dc, 3, 3, metric, lists=lists, users=ident))
    b = bits(_run(hip, dc, 3, 3, metric, lists=lists, users=None))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a user id outside 0..n_users-1 writes padding for the whole list
    bad = dc['users'].clone()
    bad[5] = ref.N_USERS
    c = _run(hip, dc, 3, 3, metric, users=bad)
    assert np.all(c[0][5] == -1) and np.all(np.isneginf(c[1][5])) and np.all(c[2][5] == -1) and np.all(np.isneginf(c[3][5])) and np.all(c[4][5] == 0)
    assert np.array_equal(c[0][6], full[0][6])


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_make_no_device_call(hip):
    import torch
    lib = hip.load()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')
    T, lists = z((10, 520), torch.float32), z((3, 65), torch.int32)
    ptr, items = z((4,), torch.int32), z((4,), torch.int32)
    pptr, pids, w = z((11,), torch.int32), z((4,), torch.int32), z((4,), torch.float32)
    o_i, o_f = z((3, 65, 17), torch.int32), z((3, 65, 17), torch.float32)
    torch.cuda.synchronize()
    before = lib.amar_last_hip_error()
    good = dict(K=16, d=8, E=3, Q=3, T=T.data_ptr(), ldt=520, pptr=pptr.data_ptr(), pids=pids.data_ptr(), w=w.data_ptr(), mpr=4, m=3)
    cases = [(dict(d=6), -2), (dict(K=65), -2), (dict(E=17), -2), (dict(Q=17), -2), (dict(mpr=hip.EXPLAIN_MAX_PROP_ROW + 1), -2),
             (dict(T=None), -1), (dict(pids=None), -1), (dict(w=None), -1), (dict(E=0), -1), (dict(Q=-1), -1), (dict(K=0), -1),
             (dict(d=516), -2), (dict(ldt=4), -1), (dict(ldt=522), -2), (dict(m=2, users=None), -1)]
    for change, want in cases:
        a = dict(good, users=ptr.data_ptr())
        a.update(change)
        got = lib.amar_explain_f32(lists.data_ptr(), a['m'], a['K'], a['users'], ptr.data_ptr(), items.data_ptr(), 3, a['T'], a['ldt'], 10,
                                   a['d'], 1, a['pptr'], a['pids'], a['w'], 4, a['mpr'], a['E'], a['Q'], o_i.data_ptr(), o_f.data_ptr(),
                                   o_i.data_ptr(), o_f.data_ptr(), o_i.data_ptr(), None)
        assert got == want, (change, got)
    assert hip.EXPLAIN_MAX_PROP_ROW >= 256
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert int(o_i.abs().sum()) == 0 and float(o_f.abs().sum()) == 0.0                      # nothing was launched


# ---- 5. models -----------------------------------------------------------------------------------------------------------
class _Train:
    def __init__(self, ratings, n_users, n_items, adj):
        self.ratings, self.users, self.items, self.adj_matrix = ratings, np.arange(n_users), np.arange(n_items), adj


def _model_case(kind):
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    from tests.test_similar_gpu import GRID1
    set_seed(11)
    g = helpers.tiny_graph(n_users=40, n_items=30, n_ratings=500, seed=5, n_props=25 if kind == 'unary-uip' else 0, n_links=160)
    model = basic.BasicGCN(g['adj'], **GRID1)
    helpers.randomize_biases(model, seed=2)
    return model, _Train(g['ratings'], g['n_users'], g['n_items'], g['adj']), g


def _model_reference(model, train, g, lists, users, E, Q, metric, weight_kind):
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    nu, ni = g['n_users'], g['n_items']
    emb = model.item_embeddings(train)
    lp, li = rec.liked_csr(train.ratings, nu, ni)
    liked = [li[lp[u]:lp[u + 1]] for u in range(nu)]
    csr = rec.item_property_csr(train)
    prop_rows = weight = None
    if csr is not None:
        prop_rows = [csr[1][csr[0][i]:csr[0][i + 1]] for i in range(ni)]
        weight = rec.property_weights(csr[2], ni, weight_kind)
    case = {'T': emb, 'liked': liked, 'prop_rows': prop_rows, 'weight': weight, 'users': users,
            'lists': np.where(lists >= 0, lists - nu, -1)}
    return case, ref.case_reference(case, metric, E, Q)


def _check_model(model, train, g, o, lists, us, E, Q, metric, kind, label):
    nu = g['n_users']
    case, refs = _model_reference(model, train, g, lists, us, E, Q, metric, kind)
    got = [np.where(o['evidence'] >= 0, o['evidence'] - nu, -1), o['evidence_sim'], o['properties'], o['property_score'], o['property_support']]
    _check(case, got, refs, metric, E, Q, label)


def test_basic_gcn_explain_on_a_unary_uip_graph(hip):
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    model, train, g = _model_case('unary-uip')
    nu = g['n_users']
    users, top, _ = model.recommend(train, k=5)
    out = model.explain(train, k=5)
    assert list(out) == list(rec.EXPLAIN_KEYS) and np.array_equal(out['users'], users) and np.array_equal(out['items'], top)
    assert out['evidence'].shape == (nu, 5, 3) and out['properties'].shape == (nu, 5, 3) and out['evidence'].dtype == np.int64

    check = lambda *a: _check_model(model, train, g, *a)
    check(out, top, users, 3, 3, 'cosine', 'idf', 'BasicGCN explain(k=5)')
    # explicit items, another metric and weight, exclude_seen=False: the target is never its own evidence
    pick = np.array([7, 0, 31])
    seen = model.explain(train, users=pick, k=5, n_evidence=4, n_properties=2, metric='dot', property_weight='none', exclude_seen=False)
    _, top_seen, _ = model.recommend(train, k=5, users=pick, exclude_seen=False)
    assert np.array_equal(seen['items'], top_seen)
    assert not np.any(seen['evidence'] == seen['items'][:, :, None])
    check(seen, top_seen, pick, 4, 2, 'dot', 'none', 'exclude_seen=False')
    liked_targets = np.asarray(train.ratings)[np.asarray(train.ratings)[:, 2] == 1]
    mine = np.full((3, 4), -1, dtype=np.int64)
    for a, u in enumerate(pick):
        own = liked_targets[liked_targets[:, 0] == u, 1][:3]
        mine[a, :len(own)] = own
    given = model.explain(train, users=pick, items=mine, n_evidence=2, n_properties=3)
    assert np.array_equal(given['items'], mine) and not np.any((given['evidence'] == mine[:, :, None]) & (mine[:, :, None] >= 0))
    check(given, mine, pick, 2, 3, 'cosine', 'idf', 'items=')
    with rec.device_lists():
        dev = model.explain(train, k=5)
    assert dev['evidence'].is_cuda and dev['items'].dtype == torch.int32
    rows = dev['evidence'].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.where(rows >= 0, rows + nu, -1), out['evidence'])
    assert np.array_equal(dev['property_score'].cpu().numpy().view(np.int32), out['property_score'].view(np.int32))


def test_two_step_model_explain_on_a_unary_kg_pair(hip):
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    from tests import helpers
    from tests.test_recommend_gpu import GRID1
    set_seed(11)
    g = helpers.kg_graph(seed=3)
    adjs = (g['adj_ui'], g['adj_ip'])
    model = basic.BasicTSGCN(g['n_users'], g['n_items'], adjs, **GRID1)
    helpers.randomize_biases(model, seed=2)
    train = _Train(g['ratings'], g['n_users'], g['n_items'], adjs)
    csr = rec.item_property_csr(train)
    assert csr is not None and len(csr[2]) == g['n_props'] and csr[3] > 0
    users, top, _ = model.recommend(train, k=5)
    out = model.explain(train, k=5)
    assert np.array_equal(out['users'], users) and np.array_equal(out['items'], top) and out['properties'].shape == (g['n_users'], 5, 3)
    assert (out['property_support'] > 0).any()
    _check_model(model, train, g, out, top, users, 3, 3, 'cosine', 'idf', 'BasicTSGCN explain(k=5)')
    again = model.explain(train, k=5)                                  # the cached device CSRs (keyed on the tuple of graphs)
    assert all(np.array_equal(np.asarray(out[key]).view(np.int32) if np.asarray(out[key]).dtype == np.float32 else out[key],
                              np.asarray(again[key]).view(np.int32) if np.asarray(again[key]).dtype == np.float32 else again[key])
               for key in out)
    pick = np.array([9, 2])
    dot = model.explain(train, users=pick, k=4, n_evidence=2, n_properties=4, metric='dot', property_weight='none', exclude_seen=False)
    _, top_dot, _ = model.recommend(train, k=4, users=pick, exclude_seen=False)
    assert np.array_equal(dot['items'], top_dot) and not np.any(dot['evidence'] == dot['items'][:, :, None])
    _check_model(model, train, g, dot, top_dot, pick, 2, 4, 'dot', 'none', 'BasicTSGCN dot')


def test_a_unary_trainset_has_no_property_part(hip):
    model, train, g = _model_case('unary')
    out = model.explain(train, k=5, n_properties=3)
    nu = g['n_users']
    assert out['properties'].shape == (nu, 5, 0) and out['property_score'].shape == (nu, 5, 0) and out['property_support'].shape == (nu, 5, 0)
    assert out['evidence'].shape == (nu, 5, 3)
    users, top, _ = model.recommend(train, k=5)
    case, refs = _model_reference(model, train, g, top, users, 3, 0, 'cosine', 'idf')
    _check(case, [np.where(out['evidence'] >= 0, out['evidence'] - nu, -1), out['evidence_sim'], out['properties'], out['property_score'],
                  out['property_support']], refs, 'cosine', 3, 0, 'unary')


# ---- 6. experiment opt-in ------------------------------------------------------------------------------------------------
def test_experiment_explain_opt_in(hip, tmp_path, monkeypatch):
    import glob
    import json
    import os
    import pandas as pd
    import yaml
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
    original = experiment.Experimenter.write_explanations

    def spy(self, **kwargs):
        captured['exp'], captured['path'] = self, original(self, **kwargs)
        return captured['path']

    monkeypatch.setattr(experiment.Experimenter, 'write_explanations', spy)
    monkeypatch.chdir(tmp_path)

    def run(name, with_props):
        cfg = json.loads(json.dumps(BASE_CONFIG))
        cfg['dataset'].update({k: v for k, v in paths.items() if with_props or k != 'props_triples_filepath'})
        if with_props:
            cfg['dataset']['type_adjacency'] = 'unary-uip'
        cfg['parameters']['epochs'] = 1
        cfg['parameters']['explain'] = {'k': 5, 'n_evidence': 2, 'n_properties': 3, 'metric': 'cosine', 'space': 'graph'}
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

    words = lambda cell: [] if pd.isna(cell) else str(cell).split(' ')
    for name, with_props in (('uip', True), ('unary', False)):
        root = run(name, with_props)
        exp, path = captured.pop('exp'), captured.pop('path')
        tsv = os.path.join(root, 'artifacts', 'predictions', 'explanations_5.tsv')
        assert os.path.exists(tsv) and os.path.samefile(tsv, path)
        frame = pd.read_csv(tsv, sep='\t', header=None, dtype=str, keep_default_na=False)
        out = exp.model.explain(exp.trainset, k=5, n_evidence=2, n_properties=3, metric='cosine', space='graph')
        nu = len(exp.trainset.users)
        user_ids, item_ids = np.asarray(exp.trainset.users), np.asarray(exp.trainset.items)
        valid = out['items'] >= 0
        assert len(frame) == int(valid.sum()) and frame.shape[1] == 8
        rows = [(j, t) for j in range(out['items'].shape[0]) for t in range(5) if valid[j, t]]
        assert frame[0].tolist() == [str(user_ids[out['users'][j]]) for j, t in rows]
        assert frame[1].tolist() == [str(item_ids[out['items'][j, t] - nu]) for j, t in rows]
        assert frame[2].tolist() == [str(t + 1) for j, t in rows]
        if with_props:
            prop_ids = np.unique(ds.props[:, 1])
            assert np.array_equal(exp.property_ids, prop_ids) and out['properties'].shape[2] == 3 and (out['properties'] >= 0).any()
        else:
            assert exp.property_ids is None and out['properties'].shape[2] == 0
        for row, (j, t) in zip(frame.itertuples(index=False), rows):
            ev = out['evidence'][j, t]
            assert words(row[3] or None) == [str(item_ids[e - nu]) for e in ev[ev >= 0]]
            assert [np.float32(x) for x in words(row[4] or None)] == out['evidence_sim'][j, t][ev >= 0].tolist()
            pr = out['properties'][j, t]
            assert words(row[5] or None) == [str(prop_ids[p]) for p in pr[pr >= 0]] if with_props else row[5] == ''
            assert [np.float32(x) for x in words(row[6] or None)] == out['property_score'][j, t][pr >= 0].tolist()
            assert [int(x) for x in words(row[7] or None)] == out['property_support'][j, t][pr >= 0].tolist()
