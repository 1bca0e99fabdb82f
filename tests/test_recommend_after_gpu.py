"""GPU: cursor paging (csrc/amar_rank_after.hip, amar_topk_segmented_after_f32, recommend.py:recommend_after / recommend_deep) —
pytest -m gpu.

The yardstick of the kernel is the kernel it was made from, and the comparison is exact: a page from a cursor must be the item rows
and the score bits amar_recommend_f32 returns with the earlier pages merged into every user's exclusion row — one score routine, so
the same bits per pair; a strict total order, so the same lists.  Cursors that are no list entries, and the pair route's ranker, are
held to tests/after_ref.py on the kernels' own score bits.  The models are held to recommend() and to their own chained pages."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import after_ref
from tests import helpers
from tests import rank_forms_ref as rf
from tests.test_recommend_among_gpu import Head, _Train, _bits, _csr, _dev, _form_of
from tests.test_recommend_among_gpu import _model_case as _small_model_case

pytestmark = pytest.mark.gpu

N_USERS = 24                                   # one full block of 16 selectors and a partial one
FORM_NAMES = ['maxt_1', 'maxt_2', 'maxt_4', 'maxt_8', 'dot_relu_zeros']      # the four kernel forms and a bulk tie (40 % of the pairs at 0)
INF = float('inf')


def _form(name):
    return _form_of(int(name[5:])) if name.startswith('maxt_') else rf.FORMS[rf.FORM_NAMES.index(name)]


def _exclusions(n, tile):
    """One set per user: 0 nothing, 1 a whole tile, 17 all but 100 rows (the catalogue runs out on the second page), 18 all but 30
    (less than one page), 19 everything, 20 / 21 all but exactly 64 / 65, the others eleven scattered rows."""
    rng = np.random.default_rng(5)
    excl = [set(rng.choice(n, size=11, replace=False).tolist()) for _ in range(N_USERS)]
    excl[0], excl[1], excl[19] = set(), set(range(tile)), set(range(n))
    for u, left in ((17, 100), (18, 30), (20, 64), (21, 65)):
        excl[u] = set(range(n)) - set(rng.choice(n, size=left, replace=False).tolist())
    return excl


_CASES = {}


def _case(capi, name):
    """Head, route and exclusions of a form, built once and shared (nothing writes to it): 24 users, 2 tiles + 5 items."""
    if name not in _CASES:
        form = _form(name)
        route = capi.rank_route('recommend', rf.dims_of(form))
        assert route['fits']
        n = 2 * route['tile_items'] + 5
        excl = _exclusions(n, route['tile_items'])
        _CASES[name] = (form, route, n, Head(capi, rf.build(form, n, n_users=N_USERS)), excl)
    return _CASES[name]


def _allowed_slices(capi, m, n_items, dims):
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    ok = [s for s in range(1, 65) if capi.load().amar_recommend_slices(m, n_items, dims_c, len(dims) - 1, s) == s]
    return sorted({s for s in (1, 2, max(ok)) if s in ok})


def _excl_dev(excl):
    ptr, items = _csr(excl)
    return dict(excl_ptr=_dev(ptr), excl_items=_dev(items))


def _host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _cursor(items, scores):
    return _dev(items, np.int32), _dev(scores, np.float32)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


# ---- 1. the start cursor is amar_recommend_f32 --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FORM_NAMES)
def test_start_cursor_is_recommend(hip, name):
    capi = hip
    form, route, n, head, excl = _case(capi, name)
    kw = _excl_dev(excl)
    start = _cursor(np.full(N_USERS, -1), np.full(N_USERS, INF))
    for k in (1, 10, 64):
        want = _host(capi.recommend(*head.args(), k, **kw))
        got = _host(capi.recommend_after(*head.args(), k, *start, **kw))
        assert got[0].dtype == np.int32 and got[0].shape == (N_USERS, k) == got[1].shape
        assert _same(got, want), (form.name, k)
        assert (want[0][19] == -1).all() and (want[0][0] >= 0).all()


# ---- 2. the next page is the exclusion list grown by the pages before ----------------------------------------------------------------
@pytest.mark.parametrize('k', (64, 10))
@pytest.mark.parametrize('name', FORM_NAMES)
def test_next_page_equals_exclusion_by_growth(hip, name, k):
    capi = hip
    form, route, n, head, excl = _case(capi, name)
    slices = _allowed_slices(capi, N_USERS, n, head.dims)
    assert len(slices) == 3 and slices[-1] > 2
    shown = [set(e) for e in excl]
    page = _host(capi.recommend(*head.args(), k, **_excl_dev(excl)))
    inside_a_tie = 0
    for number in (2, 3):
        for u in range(N_USERS):
            shown[u] |= set(page[0][u][page[0][u] >= 0].tolist())
        want = _host(capi.recommend(*head.args(), k, **_excl_dev(shown)))                     # the old way: everything shown is excluded
        cursor = _cursor(page[0][:, -1], page[1][:, -1])
        full = page[0][:, -1] >= 0
        inside_a_tie += int((want[1][full, 0] == page[1][full, -1]).sum())                    # the boundary fell between equal scores
        for n_slices in slices:
            got = _host(capi.recommend_after(*head.args(), k, *cursor, n_slices=n_slices, **_excl_dev(excl)))
            assert _same(got, want), (form.name, k, number, n_slices)
        page = want
        valid = (page[0] >= 0).sum(1)
        left = [max(0, min(k, n - len(excl[u]) - (number - 1) * k)) for u in range(N_USERS)]
        assert valid.tolist() == left
    assert (page[0][[17, 18, 19]] == -1).all() or k == 10                                     # the catalogue ran out before 3 x 64
    if name.startswith('dot_relu') and k == 64:
        assert inside_a_tie > 0                                                               # the users with 65 and 100 unseen items


# ---- 3. a cursor that is no list entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FORM_NAMES)
def test_cursor_that_is_not_a_list_entry(hip, name):
    """Over 60 items amar_recommend_f32 at k = 64 without exclusions returns every pair's score bits, so tests/after_ref.py can say
    exactly what follows any position: an excluded row, a row past the catalogue, a score between two items' scores, a score no
    item has with item -1, a tied score with a row in the middle of the tie."""
    capi = hip
    form = _form(name)
    n = 60
    head = Head(capi, rf.build(form, n, n_users=N_USERS))
    all_i, all_s = _host(capi.recommend(*head.args(), 64))
    assert ((all_i >= 0).sum(1) == n).all()
    S = np.zeros((N_USERS, n), dtype=np.float32)
    for u in range(N_USERS):
        S[u, all_i[u, :n]] = all_s[u, :n]
    rng = np.random.default_rng(17)
    excl = [set(rng.choice(n, size=int(c), replace=False).tolist()) for c in rng.integers(0, 30, size=N_USERS)]
    excl[0], excl[1] = set(), set(range(n))
    items, scores = np.zeros(N_USERS, dtype=np.int64), np.zeros(N_USERS, dtype=np.float32)
    for u in range(N_USERS):
        ranked = np.unique(S[u])                                             # ascending, distinct
        kind = u % 6
        if kind == 0 and excl[u]:
            items[u] = sorted(excl[u])[len(excl[u]) // 2]                    # an excluded row at its own score
            scores[u] = S[u, items[u]]
        elif kind == 1:
            items[u], scores[u] = n + 5, S[u, all_i[u, 9]]                   # a row past the catalogue: the whole tie of that score is skipped
        elif kind == 2 and len(ranked) > 1:
            lo, hi = ranked[len(ranked) // 2 - 1], ranked[len(ranked) // 2]
            items[u], scores[u] = 3, np.float32(lo + (hi - lo) / 2)          # between two scores (or one of them, where they are neighbours)
        elif kind == 3:
            items[u], scores[u] = -1, S[u, all_i[u, 20]]                     # a score with item -1: every row of that score follows
        elif kind == 4:
            items[u], scores[u] = 2 ** 30, ranked[0]                         # the lowest score, past every row: nothing follows
        else:
            items[u], scores[u] = all_i[u, 30], all_s[u, 30]                 # a list entry, for contrast
    for k in (10, 64):
        want = after_ref.pages(S, k, (items, scores), excluded=excl)
        got = _host(capi.recommend_after(*head.args(), k, *_cursor(items, scores), **_excl_dev(excl)))
        assert _same((got[0].astype(np.int64), got[1]), want), (form.name, k)
    assert (got[0][[u for u in range(N_USERS) if u % 6 == 4]] == -1).all() and (got[0] >= 0).any()


# ---- 4. exhaustion -----------------------------------------------------------------------------------------------------------------------
def test_exhausted_lists_stay_exhausted(hip):
    capi = hip
    form, route, n, head, excl = _case(capi, 'maxt_1')
    kw = _excl_dev(excl)
    first = _host(capi.recommend(*head.args(), 64, **kw))
    assert (first[0][18] >= 0).sum() == 30 and (first[0][19] == -1).all() and (first[0][20] >= 0).all()
    second = _host(capi.recommend_after(*head.args(), 64, *_cursor(first[0][:, -1], first[1][:, -1]), **kw))
    for u in (18, 19, 20):                                                   # 30, 0 and exactly 64 unseen items: nothing is left
        assert (second[0][u] == -1).all() and np.isneginf(second[1][u]).all()
    assert (second[0][21] >= 0).sum() == 1 and (second[0][17] >= 0).sum() == 36
    third = _host(capi.recommend_after(*head.args(), 64, *_cursor(second[0][:, -1], second[1][:, -1]), **kw))
    for u in (17, 18, 19, 20, 21):                                           # a page chained onto an exhausted list is all padding
        assert (third[0][u] == -1).all() and np.isneginf(third[1][u]).all()
    assert (third[0][0] >= 0).all()


# ---- 5. the same user with two cursors ---------------------------------------------------------------------------------------------------
def test_same_user_two_cursors(hip):
    capi = hip
    form, route, n, head, excl = _case(capi, 'maxt_2')
    kw = _excl_dev(excl)
    first = _host(capi.recommend(*head.args(), 10, users=_dev([3]), **kw))
    items, scores = np.array([-1, first[0][0, -1]]), np.array([INF, first[1][0, -1]], dtype=np.float32)
    both = _host(capi.recommend_after(*head.args(), 10, *_cursor(items, scores), users=_dev([3, 3]), **kw))
    assert not np.array_equal(both[0][0], both[0][1]) and not set(both[0][0].tolist()) & set(both[0][1].tolist())
    for row in (0, 1):
        alone = _host(capi.recommend_after(*head.args(), 10, *_cursor(items[row:row + 1], scores[row:row + 1]), users=_dev([3]), **kw))
        assert _same((both[0][row:row + 1], both[1][row:row + 1]), alone)
    assert _same((both[0][:1], both[1][:1]), first)


# ---- 6. the pair route's ranker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 64))
def test_topk_segmented_after(hip, k):
    capi = hip
    rng = np.random.default_rng(3)
    lengths = (0, 1, 63, 64, 65, 200, 0, 200)
    seg = np.cumsum((0,) + lengths)
    ids = np.concatenate([rng.permutation(400)[:c] for c in lengths])
    scores = rng.choice(np.array([0.0, 0.0, 0.125, 0.5, 0.875], dtype=np.float32), size=len(ids))        # heavy ties
    loose = rng.random(len(ids)) < 0.4
    scores[loose] = rng.random(int(loose.sum())).astype(np.float32)
    dev = (_dev(seg), _dev(ids), _dev(scores, np.float32))
    m = len(lengths)

    def ref(cursor_items, cursor_scores):
        out = [after_ref.next_page(scores[seg[u]:seg[u + 1]], k, (cursor_scores[u], cursor_items[u]), items=ids[seg[u]:seg[u + 1]]) for u in range(m)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    plain = _host(capi.topk_segmented(*dev, k))
    start = (np.full(m, -1), np.full(m, INF, dtype=np.float32))
    got = _host(capi.topk_segmented_after(*dev, k, *_cursor(*start)))
    assert _same(got, plain) and _same((got[0].astype(np.int64), got[1]), ref(*start))       # the start cursor: its sibling's output
    page, seen = plain, [set() for _ in range(m)]
    for _ in range(4 if k == 64 else 3):                                                     # chained pages: 200 items run out on the fourth
        for u in range(m):
            row = page[0][u][page[0][u] >= 0].tolist()
            assert not seen[u] & set(row)
            seen[u] |= set(row)
        cursor = (page[0][:, -1].astype(np.int64), page[1][:, -1])
        page = _host(capi.topk_segmented_after(*dev, k, *_cursor(*cursor)))
        assert _same((page[0].astype(np.int64), page[1]), ref(*cursor))
    if k == 64:
        assert (page[0] == -1).all() and all(len(seen[u]) == lengths[u] for u in range(m))
    # positions that are no entries: a tied score past / before every id, a score between, the end, a score below everything
    cursor = (np.array([5, 7, 10 ** 9, -1, 401, 3, -1, -1]), np.array([0.5, 0.0, 0.0, 0.0, 0.125, 0.3, -INF, -1.0], dtype=np.float32))
    got = _host(capi.topk_segmented_after(*dev, k, *_cursor(*cursor)))
    assert _same((got[0].astype(np.int64), got[1]), ref(*cursor))
    assert (got[0][[0, 6, 7]] == -1).all() and (got[0][3] >= 0).any()


# ---- 7. the models ---------------------------------------------------------------------------------------------------------------------------
def _model_case(name, n_items):
    """(model, train, g, route): 60 items = the graph tests/test_recommend_among_gpu.py builds (a complete ranking fits one page);
    200 items = the same models over a catalogue of more than three pages."""
    if n_items == 60:
        return _small_model_case(name)
    import torch
    from deep_cbrs_amar_renaissance_amd.data.datasets import HybridUserItemEmbeddings, UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    set_seed(29)
    g = helpers.tiny_graph(n_users=40, n_items=n_items, n_ratings=1600, seed=21)
    nu, ni = g['n_users'], g['n_items']
    rng = np.random.default_rng(13)
    if name == 'BasicGCN':
        model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=[48, 48])
        train, route = _Train(g['ratings'], nu, ni, adj_matrix=g['adj']), 'fused'
    elif name == 'BasicRS':
        model = basic.BasicRS(dense_units=[32, 16], clf_units=[128, 128, 128])                           # past every ranker's capacity
        model.build_head(32, 32)
        train, route = UserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 32)).astype(np.float32)), 'pairs'
    else:
        model = hybrid.HybridCBRS(feature_based=False, dense_units=[[32, 16], [64, 16], [32, 8]], clf_units=[16])
        model.build_head(16, 40)
        train = HybridUserItemEmbeddings(g['ratings'], g['users'], g['items'], rng.normal(0, 1, size=(nu + ni, 16)).astype(np.float32),
                                         rng.normal(0, 1, size=(nu + ni, 40)).astype(np.float32))
        route = 'pairs'
    helpers.randomize_biases(model, seed=2)
    with torch.no_grad():
        (model.rs if hasattr(model, 'rs') else model).clf.layers[-1].kernel.mul_(10.0)
    return model, train, g, route


@pytest.mark.parametrize('n_items', [60, 200])
@pytest.mark.parametrize('name', ['BasicGCN', 'BasicRS', 'HybridCBRS'])
def test_models(hip, name, n_items, monkeypatch):
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    capi = hip
    model, train, g, route = _model_case(name, n_items)
    nu, ni = g['n_users'], g['n_items']
    assert ni == n_items and model._group_route(train, 'recommend')[0] == route
    calls = {'recommend': 0, 'recommend_after': 0, 'topk_segmented': 0, 'topk_segmented_after': 0}
    for fn in list(calls):
        monkeypatch.setattr(capi, fn, (lambda f, real: lambda *a, **kw: (calls.__setitem__(f, calls[f] + 1), real(*a, **kw))[1])(fn, getattr(capi, fn)))
    first = model.recommend(train, k=64)
    calls.update({f: 0 for f in calls})
    deep = model.recommend_deep(train, 150)
    assert calls == ({'recommend': 1, 'recommend_after': 2, 'topk_segmented': 0, 'topk_segmented_after': 0} if route == 'fused' else
                     {'recommend': 0, 'recommend_after': 0, 'topk_segmented': 1, 'topk_segmented_after': 2}), calls       # scored once
    assert np.array_equal(deep[0], np.arange(nu)) and deep[1].dtype == np.int64 and deep[2].dtype == np.float32
    assert deep[1].shape == (nu, 150) == deep[2].shape
    assert np.array_equal(deep[1][:, :64], first[1]) and np.array_equal(_bits(deep[2][:, :64]), _bits(first[2]))
    seen = [set() for _ in range(nu)]
    for u, i, _ in np.asarray(train.ratings).tolist():
        seen[u].add(i)
    for u in range(nu):
        row, sc = deep[1][u], deep[2][u]
        valid = int((row >= 0).sum())
        assert valid == min(150, ni - len(seen[u])) and (row[valid:] == -1).all() and np.isneginf(sc[valid:]).all()
        assert len(set(row[:valid].tolist())) == valid and not set(row[:valid].tolist()) & seen[u]
        assert row[:valid].min(initial=nu) >= nu and row[:valid].max(initial=nu) < nu + ni
        head_s, head_i = sc[:max(valid - 1, 0)], row[:max(valid - 1, 0)]
        assert ((head_s > sc[1:valid]) | ((head_s == sc[1:valid]) & (head_i < row[1:valid]))).all(), (name, u)                                      # strictly ordered by (score descending, node id ascending)
    if n_items == 200:
        assert ((deep[1] >= 0).sum(1) > 128).all()                          # three pages with something on each
    # recommend_after chained by hand is recommend_deep
    page, chain_i, chain_s = first, [first[1]], [first[2]]
    for page_k in (64, 22):
        page = model.recommend_after(train, (page[1][:, -1], page[2][:, -1]), k=page_k)
        chain_i.append(page[1])
        chain_s.append(page[2])
    assert np.array_equal(np.concatenate(chain_i, 1), deep[1]) and np.array_equal(_bits(np.concatenate(chain_s, 1)), _bits(deep[2]))
    # a subset of the users in the caller's order, one of them twice; shorter lists are prefixes; exclude_seen=False
    users = [7, 3, 3, 39]
    sub = model.recommend_deep(train, 100, users=users)
    assert np.array_equal(sub[0], users) and np.array_equal(sub[1], deep[1][users][:, :100]) and np.array_equal(_bits(sub[2]), _bits(deep[2][users][:, :100]))
    page = model.recommend_after(train, (deep[1][users, 9], deep[2][users, 9]), k=10, users=users)
    assert np.array_equal(page[1], deep[1][users][:, 10:20]) and np.array_equal(_bits(page[2]), _bits(deep[2][users][:, 10:20]))
    open_deep = model.recommend_deep(train, 70, exclude_seen=False)
    assert ((open_deep[1] >= 0).sum(1) == min(70, ni)).all()
    with rec.device_lists():
        _, rows, sc = model.recommend_deep(train, 70)
    assert rows.is_cuda and tuple(rows.shape) == (nu, 70)
    assert np.array_equal(np.where(rows.cpu().numpy() >= 0, rows.cpu().numpy() + nu, -1), deep[1][:, :70])
    # the fused route against pair-route paging over the model's own pair scores (the 2e-6 of tests/test_recommend_gpu.py and
    # tests/test_recommend_among_gpu.py between the two routes' scores): the same items wherever no two neighbouring scores of the
    # float64 list are that close
    if route == 'fused':
        head = model._scoring_head()
        towers = head.towers(*model._recommend_tables(train))
        paired = rec.deep_pairs(lambda u, i: head.score_towers(towers, u, i), train, 150, None, True, device=towers[0].device)
        fin = np.isfinite(deep[2])
        assert np.array_equal(fin, np.isfinite(paired[2])) and np.abs(deep[2][fin] - paired[2][fin]).max() <= 2e-6
        exact = 0
        for u in range(nu):
            valid = int(fin[u].sum())
            gaps = -np.diff(paired[2][u, :valid].astype(np.float64))
            if not np.any(gaps <= 2e-6):
                assert np.array_equal(deep[1][u], paired[1][u]), u
                exact += 1
        assert exact >= nu // 2
    # the limits of the old calls stand, and nothing above left a trace
    for call in (lambda: model.recommend(train, k=65), lambda: model.recommend_among(train, [nu], k=65), lambda: model.recommend_deep(train, 1025),
                 lambda: model.recommend_after(train, (first[1][:, -1], first[2][:, -1]), k=65)):
        with pytest.raises(ValueError):
            call()
    again = model.recommend(train, k=64)
    assert np.array_equal(first[1], again[1]) and np.array_equal(_bits(first[2]), _bits(again[2]))


# ---- 8. the experiment surface -----------------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, deep_key, paths):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(paths)
    cfg['parameters']['epochs'] = 1
    if deep_key:
        cfg['parameters']['recommend_deep'] = deep_key
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


def _files(run):
    return sorted(os.path.relpath(p, run) for p in glob.glob(os.path.join(run, 'artifacts', 'predictions', '**'), recursive=True) if os.path.isfile(p))


def test_experiment_recommend_deep_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = {k: v for k, v in synthetic.write_dataset(ds, str(tmp_path / 'datasets')).items() if k != 'props_triples_filepath'}
    capture = {}
    original = experiment.Experimenter.write_recommend_deep

    def spy(self, **kw):
        capture['exp'] = self
        return original(self, **kw)

    monkeypatch.setattr(experiment.Experimenter, 'write_recommend_deep', spy)
    monkeypatch.chdir(tmp_path)
    run_on = _run_experiment(tmp_path, 'with_key', {'k': 100}, paths)
    exp = capture.pop('exp')
    top = pd.read_csv(os.path.join(run_on, 'artifacts', 'predictions', 'deep_top_100.tsv'), sep='\t', header=None)
    nu, item_ids = len(exp.trainset.users), np.asarray(exp.trainset.items)
    users, items, scores = exp.model.recommend_deep(exp.trainset, 100)
    u, r = np.nonzero(items >= 0)
    assert len(top) == len(u) > 64 * nu and top.shape[1] == 3
    assert np.array_equal(top[0].to_numpy(), np.asarray(exp.trainset.users)[users[u]])
    assert np.array_equal(top[1].to_numpy(), item_ids[items[u, r] - nu])
    assert np.allclose(top[2].to_numpy(), scores[u, r].astype(np.float64), rtol=0, atol=1e-12)
    run_off = _run_experiment(tmp_path, 'without_key', None, paths)
    assert 'exp' not in capture
    assert not glob.glob(os.path.join(run_off, '**', 'deep_top_*'), recursive=True)
    assert _files(run_off) and _files(run_off) == [f for f in _files(run_on) if 'deep_top_' not in f]      # the files it wrote before
