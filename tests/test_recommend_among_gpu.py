"""GPU: recommendation among candidates (csrc/amar_rank_among.hip, recommend.py:recommend_among) — pytest -m gpu.

The yardstick of the kernel is the kernel it was made from, and the comparison is exact: for candidates C,
capi.recommend_among(cand=C, excl=E) must return the item rows and the score bits of capi.recommend(excl = E u complement(C)) —
one score routine, so the same bits per pair; a strict total order, so the same lists.  One value check per kernel form against
the float64 restatement of tests/rank_forms_ref.py shows the gather reads inside its window.  The models are held to their own
complete rankings, struck down to the candidates on the host."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import among_ref
from tests import chain_ref
from tests import helpers
from tests import rank_forms_ref as rf

pytestmark = pytest.mark.gpu

KS = (1, 10, 64)
N_USERS = 24
EINVAL, EUNSUPPORTED = -1, -2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _csr(segments):
    ptr = np.cumsum([0] + [len(s) for s in segments])
    return ptr.astype(np.int32), np.array([i for s in segments for i in sorted(s)], dtype=np.int32)


def _form_of(maxt):
    """The narrowest head of the grid that reaches the kernel form MAXT = maxt."""
    forms = [f for f in rf.FORMS if rf.route('recommend', rf.dims_of(f))[1]['maxt'] == maxt]
    return min(forms, key=lambda f: (max(rf.dims_of(f)), sum(rf.dims_of(f))))


class Head:
    """A built case on the device: the packed stack and Tu / Ti as column windows of wider NaN-filled tensors (ld = 2 c1)."""

    def __init__(self, capi, case):
        import torch
        self.case, self.dims, self.acts, self.in_act = case, case['dims'], case['acts'], case['in_act']
        ks, bs = [w for w, _ in case['layers']], [b for _, b in case['layers']]
        blob = capi.chain_pack(ks, bs)[0] if len(ks) <= capi.CHAIN_MAX_LAYERS else chain_ref.pack(ks, bs)
        self.blob = torch.from_numpy(np.ascontiguousarray(blob, dtype=np.float32)).cuda()
        c1 = self.dims[0]
        self.tables = []
        for table in (case['tu'], case['ti']):
            wide, off = rf.windowed(table, 'x2')
            view = torch.from_numpy(wide).cuda()[:, off:off + c1]
            assert view.data_ptr() % 16 == 0 and not view.is_contiguous()
            self.tables.append(view)
        self.tu, self.ti = self.tables

    def args(self):
        return (self.tu, self.ti, self.blob, self.dims, self.acts, self.in_act)


_CASES = {}


def _case(capi, maxt):
    """Head and route of a kernel form, built once and shared (nothing writes to it): 24 users, 2 tiles + 37 items."""
    if maxt not in _CASES:
        form = _form_of(maxt)
        route = capi.rank_route('among', rf.dims_of(form))
        assert route['fits'] and route['maxt'] == maxt
        n_items = 2 * route['tile_items'] + 37
        _CASES[maxt] = (form, route, n_items, Head(capi, rf.build(form, n_items, n_users=N_USERS)))
    return _CASES[maxt]


def _candidate_sets(k, tile, n):
    rng = np.random.default_rng(100 + k)
    pick = lambda c: np.sort(rng.choice(n, size=c, replace=False))
    return {'empty': np.zeros(0, dtype=np.int64), 'first': np.array([0]), 'last': np.array([n - 1]), 'all': np.arange(n),
            'every_other': np.arange(0, n, 2), 'k_minus_1': pick(k - 1), 'tile_minus_1': pick(tile - 1), 'tile': pick(tile),
            'tile_plus_1': pick(tile + 1), 'last_tile': np.arange(2 * tile, n), 'random_3_percent': pick(max(1, round(0.03 * n)))}


def _allowed_slices(capi, m, n_cand, dims):
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    ok = [s for s in range(1, 65) if capi.load().amar_recommend_slices(m, n_cand, dims_c, len(dims) - 1, s) == s]
    return sorted({s for s in (1, 2, max(ok)) if s in ok})


# ---- 1. the kernel against the kernel it was made from ---------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('maxt', [1, 2, 4, 8])
def test_among_equals_recommend_with_the_complement_excluded(hip, maxt, k):
    capi = hip
    form, route, n, head = _case(capi, maxt)
    tile = route['tile_items']
    base = helpers.select_case_exclusions(k, tile_rows=tile, n=n, m=N_USERS)
    user_lists = (None, np.array([23, 22, 17, 17, 5, 4, 1, 0], dtype=np.int32))      # everyone; a subset, descending, one user twice
    everything = set(range(n))
    listed, sliced = 0, set()
    for name, cand in _candidate_sets(k, tile, n).items():
        c = set(cand.tolist())
        excl = [set(base[u]) for u in range(N_USERS)]
        excl[22] = set(c)                                                 # every candidate is seen
        excl[23] = set(sorted(c)[1:])                                     # ... all but one
        e_ptr, e_items = _csr(excl)
        w_ptr, w_items = _csr([e | (everything - c) for e in excl])       # the only way amar_recommend_f32 can say "among C"
        for users in user_lists:
            u_dev = None if users is None else _dev(users)
            m = N_USERS if users is None else len(users)
            want_i, want_s = capi.recommend(*head.args(), k, users=u_dev, excl_ptr=_dev(w_ptr), excl_items=_dev(w_items))
            want_i, want_s = want_i.cpu().numpy(), want_s.cpu().numpy()
            order = np.arange(N_USERS) if users is None else users
            assert (want_i[order == 22] == -1).all() and ((want_i[order == 23] >= 0).sum(1) == min(1, len(c))).all()
            for n_slices in _allowed_slices(capi, m, len(cand), head.dims):
                got_i, got_s = capi.recommend_among(*head.args(), k, cand, users=u_dev, excl_ptr=_dev(e_ptr), excl_items=_dev(e_items),
                                                    n_slices=n_slices)
                got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
                assert got_i.dtype == np.int32 and got_i.shape == (m, k) == got_s.shape
                assert np.array_equal(got_i, want_i), (form.name, name, k, n_slices)
                assert np.array_equal(_bits(got_s), _bits(want_s)), (form.name, name, k, n_slices)
                sliced.add(n_slices)
            listed += int((want_i >= 0).sum())
            assert set(want_i[want_i >= 0].tolist()) <= c
    assert listed > 0 and {1, 2, 3} <= sliced                            # three tiles of candidates were cut one per slice


# ---- 2. values: the gather reads inside its window ---------------------------------------------------------------------------------
@pytest.mark.parametrize('maxt', [1, 2, 4, 8])
def test_values_against_float64(hip, maxt):
    """k = 64 over a 64-candidate set without exclusions returns every candidate's score; against the float64 restatement within
    max(1e-6, 8 x the float32 restatement's own error).  Tu and Ti are windows of tensors whose padding is NaN: a gathered read
    outside a row's window would land in the scores."""
    capi = hip
    form, route, n, head = _case(capi, maxt)
    case = head.case
    cand = np.sort(np.random.default_rng(7).choice(n, size=64, replace=False))
    cand[[0, -1]] = 0, n - 1
    got_i, got_s = (t.cpu().numpy() for t in capi.recommend_among(*head.args(), 64, cand))
    assert (np.sort(got_i, axis=1) == cand[None, :]).all()               # every candidate, nothing else, nothing padded
    S = np.full((N_USERS, n), np.nan, dtype=np.float32)
    S[np.arange(N_USERS)[:, None], got_i] = got_s
    args = (case['tu'], case['ti'][cand], case['layers'], case['acts'], case['in_act'])
    s32, s64 = rf.scores(*args, np.float32), rf.scores(*args, np.float64)
    assert not np.isnan(S[:, cand]).any()
    tol = rf.bound(s32, s64)
    err = float(np.abs(S[:, cand].astype(np.float64) - s64).max())
    print('among form {:<12s} max |kernel - float64| {:.3e}  bound {:.3e}'.format(form.name, err, tol))
    assert err <= tol, (form.name, err, tol)
    want_i, want_s = among_ref.topk_among(S, range(N_USERS), None, cand, 64)          # the order, on the kernel's own bits
    assert np.array_equal(got_i.astype(np.int64), want_i) and np.array_equal(_bits(got_s), _bits(want_s))


# ---- 3. refusals: nothing is launched ------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import torch
    capi = hip
    lib = capi.load()
    form, route, n, head = _case(capi, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def raw(h, n_users, n_items, k, cand, n_cand, outs):
        dims_c = (ctypes.c_int32 * len(h.dims))(*h.dims)
        acts_c = (ctypes.c_int32 * len(h.acts))(*[capi.ACT_CODES[a] for a in h.acts])
        return lib.amar_recommend_among_f32(p(h.tu), int(h.tu.stride(0)), n_users, p(h.ti), int(h.ti.stride(0)), n_items, h.dims[0], p(h.blob),
                                            dims_c, acts_c, len(h.acts), capi.ACT_CODES[h.in_act], None, n_users, None, None,
                                            None if cand is None else p(cand), n_cand, k, 1, None, None, p(outs[0]), p(outs[1]), None)

    o_i = torch.full((N_USERS * 65,), 7, dtype=torch.int32, device='cuda')
    o_s = torch.full((N_USERS * 65,), 7.0, dtype=torch.float32, device='cuda')
    cand = _dev([0, 1, 2])
    torch.cuda.synchronize()
    before = lib.amar_last_hip_error()
    assert raw(head, N_USERS, n, 65, cand, 3, (o_i, o_s)) == EUNSUPPORTED                      # k = 65
    assert raw(head, N_USERS, n, 4, None, 3, (o_i, o_s)) == EINVAL                             # NULL cand_items with n_cand > 0
    assert raw(head, N_USERS, n, 4, cand, -1, (o_i, o_s)) == EINVAL and raw(head, N_USERS, n, 4, cand, n + 1, (o_i, o_s)) == EINVAL
    largest, past = rf.capacity_heads(lambda d: capi.rank_fits('among', d))
    past_head = Head(capi, rf.build(rf._f('past_among', 128, past[1:-1], "the first head past among's capacity"), 8, n_users=4))
    assert raw(past_head, 4, 8, 4, cand, 3, (o_i, o_s)) == EUNSUPPORTED                        # a head past the capacity
    with pytest.raises(capi.AmarError):
        capi.recommend_among(*past_head.args(), 4, [0, 1, 2])
    with pytest.raises(capi.AmarError):
        capi.recommend_among(*head.args(), 65, [0, 1, 2])
    for bad in ([2, 1, 0], [0, 1, 1], [0, n], [-1, 0]):                                        # checked before anything is uploaded
        with pytest.raises(ValueError, match='cand'):
            capi.recommend_among(*head.args(), 4, bad)
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert (o_i == 7).all() and (o_s == 7.0).all()                                            # nothing was launched
    at_head = Head(capi, rf.build(rf._f('at_among', 128, largest[1:-1], 'the same call at the limit'), 8, n_users=4))
    assert raw(at_head, 4, 8, 4, cand, 3, (o_i, o_s)) == 0                                     # ... and the largest head is served
    assert raw(head, N_USERS, n, 4, None, 0, (o_i, o_s)) == 0                                  # n_cand == 0: NULL is fine, all padding
    torch.cuda.synchronize()
    assert (o_i[:N_USERS * 4] == -1).all() and torch.isneginf(o_s[:N_USERS * 4]).all()


# ---- 4. the models -----------------------------------------------------------------------------------------------------------------
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
    set_seed(23)
    g = helpers.tiny_graph(n_users=40, n_items=60, n_ratings=500, seed=15, n_props=7, n_links=150)       # unary-uip, 60 items <= 64
    nu, ni = g['n_users'], g['n_items']
    rng = np.random.default_rng(9)
    if name == 'BasicGCN':
        model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48])
        train, route = _Train(g['ratings'], nu, ni, adj_matrix=g['adj']), 'fused'
    elif name == 'BasicRS':
        model = basic.BasicRS(dense_units=[32, 16], clf_units=[128, 128, 128])                           # past every ranker's capacity
        model.build_head(32, 32)
        train = UserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 32)).astype(np.float32))
        train.adj_matrix = g['adj']
        route = 'pairs'
    else:
        model = hybrid.HybridCBRS(feature_based=False, dense_units=[[32, 16], [64, 16], [32, 8]], clf_units=[16])
        model.build_head(16, 40)
        train = HybridUserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 16)).astype(np.float32),
                                         rng.normal(0, 1, size=(nu + ni, 40)).astype(np.float32))
        train.adj_matrix = g['adj']
        route = 'pairs'
    helpers.randomize_biases(model, seed=2)
    with torch.no_grad():
        (model.rs if hasattr(model, 'rs') else model).clf.layers[-1].kernel.mul_(10.0)
    return model, train, g, route


def _same(got, want_i, want_s):
    return np.array_equal(got[1], want_i) and np.array_equal(_bits(got[2]), _bits(want_s))


@pytest.mark.parametrize('name', ['BasicGCN', 'BasicRS', 'HybridCBRS'])
def test_models_against_their_own_full_ranking(hip, name, monkeypatch):
    """With <= 64 items recommend(k=64) is every user's complete ranking; recommend_among must return it struck down to the
    candidates and cut to k: items exactly, scores bit for bit.  Per-user candidates take the pair route in every model, so they
    are held to the pair route's complete ranking (`_recommend_pairs`; for BasicGCN tests/test_recommend_gpu.py holds that one within
    2e-6 of the fused one, which is not 'bit for bit')."""
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    capi = hip
    model, train, g, route = _model_case(name)
    nu, ni = g['n_users'], g['n_items']
    assert ni <= 64 and model._group_route(train, kind='among')[0] == route
    full = model.recommend(train, k=64)
    full_pairs = model._recommend_pairs(train, k=64)
    open_full = model.recommend(train, k=64, exclude_seen=False)
    assert ((open_full[1] >= 0).sum(1) == ni).all() and ((full[1] >= 0).sum(1) < ni).any()
    calls = {'fused': 0, 'pairs': 0}
    fused, topk = capi.recommend_among, capi.topk_segmented
    monkeypatch.setattr(capi, 'recommend_among', lambda *a, **kw: (calls.__setitem__('fused', calls['fused'] + 1), fused(*a, **kw))[1])
    monkeypatch.setattr(capi, 'topk_segmented', lambda *a, **kw: (calls.__setitem__('pairs', calls['pairs'] + 1), topk(*a, **kw))[1])
    rng = np.random.default_rng(3)
    sets = [nu + np.sort(rng.choice(ni, size=c, replace=False)) for c in (1, 7, 30)] + [np.zeros(0, dtype=np.int64)]
    n_calls = 0
    for cand in sets:
        for k in (1, 10, 64):
            got = model.recommend_among(train, cand[::-1], k=k)
            n_calls += 1
            assert np.array_equal(got[0], np.arange(nu)) and got[1].dtype == np.int64 and got[2].dtype == np.float32 and got[1].shape == (nu, k)
            assert _same(got, *among_ref.filter_lists(full[1], full[2], set(cand.tolist()), k)), (name, len(cand), k)
    assert calls == ({'fused': n_calls, 'pairs': 0} if route == 'fused' else {'fused': 0, 'pairs': n_calls}), calls
    # every item is a candidate: recommend() itself
    for k in (5, 64):
        assert _same(model.recommend_among(train, np.arange(nu, nu + ni), k=k), full[1][:, :k], full[2][:, :k])
    # a subset of the users, in the caller's order, one of them twice
    users = [7, 3, 3, 39]
    got = model.recommend_among(train, sets[2], k=10, users=users)
    assert np.array_equal(got[0], users) and _same(got, *among_ref.filter_lists(full[1][users], full[2][users], set(sets[2].tolist()), 10))
    # the mask form is the id form
    mask = np.zeros(ni, dtype=bool)
    mask[sets[2] - nu] = True
    assert _same(model.recommend_among(train, mask, k=10), *model.recommend_among(train, sets[2], k=10)[1:])
    # exclude_seen=False
    got = model.recommend_among(train, sets[2], k=64, exclude_seen=False)
    assert _same(got, *among_ref.filter_lists(open_full[1], open_full[2], set(sets[2].tolist()), 64)) and ((got[1] >= 0).sum(1) == 30).all()
    # per-user candidates: the pair route, against the pair route's complete ranking
    before = dict(calls)
    per = [nu + np.sort(rng.choice(ni, size=int(rng.integers(0, 40)), replace=False)) for _ in range(nu)]
    got = model.recommend_among(train, per, k=10)
    assert calls['fused'] == before['fused'] and calls['pairs'] == before['pairs'] + 1
    assert _same(got, *among_ref.filter_lists(full_pairs[1], full_pairs[2], [set(p.tolist()) for p in per], 10))
    got = model.recommend_among(train, [per[u] for u in users], k=10, users=users)
    assert _same(got, *among_ref.filter_lists(full_pairs[1][users], full_pairs[2][users], [set(per[u].tolist()) for u in users], 10))
    assert np.array_equal(got[1][1], got[1][2])
    # candidates from the graph's properties: only items that pass the loop restatement come back
    ptr, props, _, _ = rec.item_property_csr(train)
    has = [set(props[ptr[i]:ptr[i + 1]].tolist()) for i in range(ni)]
    kw = dict(any_of=[0, 1, 2], none_of=[6])
    passing = among_ref.items_with_properties(has, **kw)
    assert 0 < len(passing) < ni
    got = model.recommend_among(train, rec.items_with_properties(train, **kw), k=64)
    assert set(got[1][got[1] >= 0].tolist()) <= {nu + r for r in passing}
    assert _same(got, *among_ref.filter_lists(full[1], full[2], {nu + r for r in passing}, 64))
    # device lists
    with rec.device_lists():
        u, rows, sc = model.recommend_among(train, sets[1], k=10)
    want = model.recommend_among(train, sets[1], k=10)
    assert rows.is_cuda and rows.dtype.is_floating_point is False and np.array_equal(np.where(rows.cpu().numpy() >= 0, rows.cpu().numpy() + nu, -1), want[1])
    for bad in (dict(candidates=[nu - 1]), dict(candidates=[nu], k=65), dict(candidates=[nu], users=[nu]), dict(candidates=np.ones(ni + 1, dtype=bool)),
                dict(candidates=[[nu]] * (nu - 1))):
        with pytest.raises(ValueError):
            model.recommend_among(train, **bad)
    # no side effects: recommend() returns the bits it returned before
    after = model.recommend(train, k=64)
    assert np.array_equal(full[1], after[1]) and np.array_equal(_bits(full[2]), _bits(after[2]))


# ---- 5. the experiment surface -------------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, among_key, paths):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(paths)
    cfg['parameters']['epochs'] = 1
    if among_key:
        cfg['parameters']['recommend_among'] = among_key
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


def test_experiment_recommend_among_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    capture = {}
    original = experiment.Experimenter.write_recommend_among

    def spy(self, **kw):
        capture['exp'] = self
        return original(self, **kw)

    monkeypatch.setattr(experiment.Experimenter, 'write_recommend_among', spy)
    monkeypatch.chdir(tmp_path)
    listed = np.unique(ds.train[:, 1])[::9][:40].tolist()                 # original item ids, and one nobody has rated
    unknown = int(ds.train[:, 1].max()) + 1000
    run_on = _run_experiment(tmp_path, 'with_key', {'k': 5, 'candidates': listed + [unknown]}, paths)
    exp = capture.pop('exp')
    top = pd.read_csv(os.path.join(run_on, 'artifacts', 'predictions', 'among_top_5.tsv'), sep='\t', header=None)
    nu, item_ids = len(exp.trainset.users), np.asarray(exp.trainset.items)
    index = {i: r for r, i in enumerate(item_ids.tolist())}
    cand = np.array([index[i] for i in listed]) + nu
    users, items, scores = exp.model.recommend_among(exp.trainset, cand, k=5)
    u, r = np.nonzero(items >= 0)
    assert len(top) == len(u) > 0 and top.shape[1] == 4 and set(top[2].tolist()) <= set(listed)
    assert np.array_equal(top[0].to_numpy(), np.asarray(exp.trainset.users)[users[u]]) and top[1].tolist() == (r + 1).tolist()
    assert np.array_equal(top[2].to_numpy(), item_ids[items[u, r] - nu])
    assert np.array_equal(_bits(top[3].to_numpy().astype(np.float32)), _bits(scores[u, r]))
    run_off = _run_experiment(tmp_path, 'without_key', None, paths)
    assert 'exp' not in capture
    assert not glob.glob(os.path.join(run_off, '**', 'among_top_*'), recursive=True)
