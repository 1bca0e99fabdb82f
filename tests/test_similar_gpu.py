"""GPU: similarity search (amar_nearest_f32 and the models' similar_items / similar_users / recommend_like) against the float64
restatement of tests/similar_ref.py, invariance, and the opt-in experiment surface (pytest -m gpu).

Score tolerance (derived, similar_ref.score_tolerance): (d + 8) 2^-24 ||q|| ||t||, the norms being 1 for cosine.  Lists equal the
float64 ranking except where float64 gaps inside the first k + 1 ranks are within twice the observed score error; at most
MAX_NEAR_TIE_QUERIES of the 37 queries may differ that way (the cap of tests/test_recommend_gpu.py)."""
import glob
import json
import os

import numpy as np
import pytest
import yaml

from tests import helpers, similar_ref as ref

pytestmark = pytest.mark.gpu

MAX_NEAR_TIE_QUERIES = 3
M_QUERIES = 37                  # not a multiple of the 16-query block


def case_seed(n_rows, d, metric):
    return 100000 * d + 10 * n_rows + (1 if metric == 'cosine' else 0) + helpers.seed_offset()


def _csr(excl, order, dev):
    """Exclusion CSR over the listed queries `order` (segment j = the set of query order[j])."""
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    ptr, rows = rec.lists_csr([sorted(excl[j]) for j in order], 1 << 30)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev)


def _bits(rows, scores):
    return rows.cpu().numpy(), scores.cpu().numpy().view(np.int32)


# ---- 1. the kernel against float64, and its invariance ---------------------------------------------------------------
@pytest.mark.parametrize('metric', ['dot', 'cosine'])
@pytest.mark.parametrize('d', [4, 36, 64, 200, 512])
@pytest.mark.parametrize('n_rows', [1, 17, 3191])
def test_kernel_against_float64(hip, n_rows, d, metric):
    import torch
    capi = hip
    m = M_QUERIES
    Q, T, excl = ref.planted_case(n_rows, d, metric, case_seed(n_rows, d, metric), m=m)
    want64 = ref.nearest64(Q, T, metric)
    tol = ref.score_tolerance(Q, T, metric)
    dev = torch.device('cuda')
    # queries: rows of a separate matrix with ldq > d; the table: a column slice of a wider buffer (ldt > d)
    q_buf = torch.zeros((m, d + 4), dtype=torch.float32, device=dev)
    t_buf = torch.full((n_rows, d + 12), 7.0, dtype=torch.float32, device=dev)
    q_d, t_d = q_buf[:, :d], t_buf[:, 4:4 + d]
    q_d.copy_(torch.from_numpy(Q))
    t_d.copy_(torch.from_numpy(T))
    assert q_d.stride(0) > d and t_d.stride(0) > d
    ptr_d, ex_d = _csr(excl, range(m), dev)
    subset = np.random.default_rng(case_seed(n_rows, d, metric) + 7).permutation(m)[:11]
    sub_ptr, sub_ex = _csr(excl, subset.tolist(), dev)
    for k in (1, 10, 64):
        label = 'n={} d={} {} k={}'.format(n_rows, d, metric, k)
        got = capi.nearest(q_d, t_d, k, metric=metric, excl_ptr=ptr_d, excl_rows=ex_d)
        got_r, got_s = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert got_r.dtype == np.int32 and got_s.dtype == np.float32 and got_r.shape == (m, k) and got_s.shape == (m, k)
        differing, err = ref.check_lists(np.arange(m), got_r, got_s, want64, excl, k, label, tol)
        print('{}: max score error {:.3e}, lists differing by near-ties {}'.format(label, err, differing))
        assert differing <= MAX_NEAR_TIE_QUERIES, label
        # the all-zero query scores 0 against everything under cosine: never NaN
        assert not np.isnan(got_s).any()
        if metric == 'cosine':
            z = got_s[m - 1]
            assert np.all(z[np.isfinite(z)] == 0)
        # two calls: the same bits
        again = capi.nearest(q_d, t_d, k, metric=metric, excl_ptr=ptr_d, excl_rows=ex_d)
        assert all(np.array_equal(x, y) for x, y in zip(_bits(*again), _bits(*got))), label
        # a shuffled subset of the queries: bitwise the rows of the full call
        sub = capi.nearest(q_d, t_d, k, metric=metric, query_rows=torch.from_numpy(subset.astype(np.int32)).to(dev),
                           excl_ptr=sub_ptr, excl_rows=sub_ex)
        assert np.array_equal(sub[0].cpu().numpy(), got_r[subset]), label
        assert np.array_equal(sub[1].cpu().numpy().view(np.int32), got_s[subset].view(np.int32)), label
        # any table slicing: the same bits
        for slices in (1, 2, 5):
            if capi.load().amar_nearest_slices(m, n_rows, d, slices) != slices:
                continue
            sl = capi.nearest(q_d, t_d, k, metric=metric, excl_ptr=ptr_d, excl_rows=ex_d, n_slices=slices)
            assert all(np.array_equal(x, y) for x, y in zip(_bits(*sl), _bits(*got))), (label, slices)
        # exclusion off: every row ranks
        all_r, _ = capi.nearest(q_d, t_d, k, metric=metric)
        assert (all_r.cpu().numpy() >= 0).sum(axis=1).tolist() == [min(k, n_rows)] * m
    if n_rows > 4:
        big_r, _ = capi.nearest(q_d, t_d, 64, metric=metric)
        row = big_r.cpu().numpy()[5].tolist()
        dup = [i for i in (1, n_rows // 2, n_rows - 1) if i in row]
        assert [i for i in row if i in dup] == sorted(dup)                            # exact ties in row order
    assert torch.all(t_buf[:, :4] == 7.0) and torch.all(t_buf[:, 4 + d:] == 7.0)         # the buffer around the slice is untouched


@pytest.mark.parametrize('k', [1, 63, 64])
def test_selector_adversarial_orders(hip, k):
    """The shared selector where it merges most and least: 197 rows, 19 queries, scores strictly ascending in the row id (every row
    beats the threshold: a merge per full buffer) and the table reversed (nothing after the first k passes), exclusions on group
    and tile edges, one query with nothing left and one with k - 1 rows left.  dot with Q = e0 and T[i] = i e0: the scores are the
    integers, exact in float32, so the lists are known exactly."""
    import torch
    capi, n, m, d = hip, helpers.SELECT_ROWS, helpers.SELECT_QUERIES, 4
    dev = torch.device('cuda')
    excl = helpers.select_case_exclusions(k, tile_rows=256)                              # d = 4 stages 256-row tiles
    ptr_d, ex_d = _csr(excl, range(m), dev)
    Q = np.zeros((m, d), dtype=np.float32)
    Q[:, 0] = 1.0
    for reverse in (False, True):
        value = np.arange(n)[::-1] if reverse else np.arange(n)                          # score of row i
        T = np.zeros((n, d), dtype=np.float32)
        T[:, 0] = value
        want_r = helpers.select_case_expected(excl, k, np.argsort(-value, kind='stable').tolist())
        want_s = np.where(want_r >= 0, value[np.maximum(want_r, 0)], -np.inf).astype(np.float32)
        q_d, t_d = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev)
        for slices in (1, 2, 3):
            if capi.load().amar_nearest_slices(m, n, d, slices) != slices:
                continue
            got_r, got_s = capi.nearest(q_d, t_d, k, metric='dot', excl_ptr=ptr_d, excl_rows=ex_d, n_slices=slices)
            assert np.array_equal(got_r.cpu().numpy(), want_r), (k, reverse, slices)
            assert np.array_equal(got_s.cpu().numpy(), want_s), (k, reverse, slices)


def test_slicing_is_exercised(hip):
    """The grid above really reaches the sliced form (two launches) at its large table."""
    s = hip.load().amar_nearest_slices
    assert all(s(M_QUERIES, 3191, d, 2) == 2 and s(M_QUERIES, 3191, d, 5) == 5 for d in (4, 36, 64, 200, 512))
    assert s(M_QUERIES, 3191, 64, 0) > 1


def test_nearest_host_and_device_arrays(hip):
    """recommend.nearest: host or device arrays, per-query exclusion lists, host results; device results inside device_lists()."""
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    Q, T, excl = ref.planted_case(50, 12, 'cosine', 5, m=9)
    lists = [sorted(excl[j]) for j in range(9)]
    rows, scores = rec.nearest(Q, T, k=7, exclude=lists)
    assert rows.dtype == np.int64 and scores.dtype == np.float32 and rows.shape == (9, 7)
    want = ref.nearest64(Q, T, 'cosine')
    assert ref.check_lists(np.arange(9), rows, scores, want, excl, 7, 'nearest host', ref.score_tolerance(Q, T, 'cosine'))[0] == 0
    r2, s2 = rec.nearest(torch.from_numpy(Q).cuda(), torch.from_numpy(T).cuda(), k=7, exclude=lists)
    assert np.array_equal(r2, rows) and np.array_equal(s2.view(np.int32), scores.view(np.int32))
    with rec.device_lists():
        r3, s3 = rec.nearest(Q, T, k=7, exclude=lists)
    assert r3.is_cuda and r3.dtype == torch.int32 and np.array_equal(r3.cpu().numpy(), rows)
    with pytest.raises(NotImplementedError, match='6'):
        rec.nearest(np.zeros((2, 6), dtype=np.float32), np.zeros((3, 6), dtype=np.float32))
    with pytest.raises(ValueError):
        rec.nearest(Q, T, exclude=lists[:3])


# ---- 2. models -------------------------------------------------------------------------------------------------------
GRID1 = dict(embedding_dim=8, n_hiddens=[8, 8], n_layers=2, dense_units=[24, 24], clf_units=[48, 48],
             l2_regularizer=1e-4, final_node='concatenation', aggregate='mean', dropout_rate=0.0, activation='relu')


class _Train:
    """The parts of a training Sequence the embedding accessors read."""

    def __init__(self, ratings, n_users, n_items, **tables):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)
        self.__dict__.update(tables)


def _fixture(name):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemEmbeddings
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    set_seed(11)
    if name == 'BasicGCN':
        g = helpers.tiny_graph(seed=5)
        model = basic.BasicGCN(g['adj'], **GRID1)
        train = _Train(g['ratings'], g['n_users'], g['n_items'])
    elif name == 'HybridBertGCN':
        g = helpers.tiny_graph(seed=6)
        model = hybrid.HybridBertGCN(g['adj'], **dict(GRID1, dense_units=[[24, 24], [32, 16], [16, 16]], clf_units=[16, 16],
                                                       feature_based=True, fusion_method='concatenate'))
        bert = np.random.default_rng(2).normal(0, 1, size=(g['n_users'] + g['n_items'], 48)).astype(np.float32)
        model.set_bert_table(bert)
        model.rs.build_head(model.gnn.output_dim(), 48)
        train = _Train(g['ratings'], g['n_users'], g['n_items'])
    else:
        g = helpers.tiny_graph(n_users=45, n_items=70, n_ratings=900, seed=9)
        table = np.random.default_rng(4).normal(0, 1, size=(g['n_users'] + g['n_items'], 32)).astype(np.float32)
        model = basic.BasicRS(dense_units=[64, 32], clf_units=[64, 64])
        model.build_head(32, 32)
        train = UserItemEmbeddings(g['ratings'], g['users'], g['items'], table)
    helpers.randomize_biases(model, seed=2)
    return model, train, g


SPACES = {'BasicGCN': ('graph', 'tower'), 'HybridBertGCN': ('graph', 'tower'), 'BasicRS': ('tower',)}


@pytest.mark.parametrize('name', ['BasicGCN', 'HybridBertGCN', 'BasicRS'])
def test_models_against_float64_of_their_embeddings(hip, name):
    model, train, g = _fixture(name)
    nu, ni = g['n_users'], g['n_items']
    assert tuple(model._embedding_spaces()) == SPACES[name]
    for space in SPACES[name] + (None,):
        for side, n, base, emb_fn, search in (('items', ni, nu, model.item_embeddings, model.similar_items),
                                              ('users', nu, 0, model.user_embeddings, model.similar_users)):
            emb = emb_fn(train, space=space)
            assert emb.dtype == np.float32 and emb.shape[0] == n and emb.shape[1] % 4 == 0
            if space is None:
                assert np.array_equal(emb, emb_fn(train, space=SPACES[name][0]))
                continue
            for metric in ('cosine', 'dot'):
                want64 = ref.nearest64(emb, emb, metric)
                tol = ref.score_tolerance(emb, emb, metric)
                label = '{} {} {} {}'.format(name, space, side, metric)
                ids, nb, sc = search(train, k=10, metric=metric, space=space)
                assert ids.dtype == np.int64 and nb.dtype == np.int64 and sc.dtype == np.float32
                assert np.array_equal(ids, np.arange(n) + base) and nb.shape == (n, 10) and sc.shape == (n, 10)
                differing, err = ref.check_lists(np.arange(n), nb, sc, want64, {j: {j} for j in range(n)}, 10, label, tol, base=base)
                print('{}: max score error {:.3e}, differing {}'.format(label, err, differing))
                assert differing <= MAX_NEAR_TIE_QUERIES, label
                assert not np.any(nb == ids[:, None])                                     # the query itself is absent
                # a subset in the caller's order, the query itself allowed
                pick = np.array([n - 1, 0, 7, 3]) + base
                ids2, nb2, sc2 = search(train, pick, k=5, metric=metric, space=space, exclude_self=False)
                assert np.array_equal(ids2, pick)
                differing, err = ref.check_lists(pick - base, nb2, sc2, want64, {}, 5, label + ' with self', tol, base=base)
                assert differing <= MAX_NEAR_TIE_QUERIES
                if metric == 'cosine':
                    # a query of non-zero norm ranks first: whatever stands before it is a float64 near-tie at cosine 1
                    for r, q in enumerate((pick - base).tolist()):
                        if np.any(emb[q] != 0):
                            pos = nb2[r].tolist().index(q + base)
                            assert np.all(want64[q, nb2[r, :pos] - base] >= 1 - 2 * tol[0, 0]), label


@pytest.mark.parametrize('name', ['BasicGCN', 'HybridBertGCN', 'BasicRS'])
def test_recommend_like_and_state(hip, name):
    from deep_cbrs_amar_renaissance_amd.data.datasets import UserItemGraph
    model, train, g = _fixture(name)
    nu, ni = g['n_users'], g['n_items']
    rec0 = model.recommend(train, k=10)
    if name == 'BasicGCN':
        seq = UserItemGraph(g['ratings'], g['users'], g['items'], g['adj'], batch_size=256)
        score = lambda: model.predict(seq)
    elif name == 'BasicRS':
        score = lambda: model.predict(train)
    else:                                                    # ids against the resident BERT table
        score = lambda: model((g['u_ids'], g['i_ids'], None, None)).cpu().numpy()
    pred0 = score()
    state0 = (model.gnn.hoist, model.gnn._hoisted, model._towers) if name != 'BasicRS' else None
    for space in SPACES[name]:
        items = np.array([nu + 4, nu, nu + ni - 1])
        ids, nb, sc = model.similar_items(train, items, k=8, space=space)
        # one-item profiles are those items' own searches, bit for bit
        lnb, lsc = model.recommend_like(train, [[int(i)] for i in items], k=8, space=space)
        assert np.array_equal(lnb, nb) and np.array_equal(lsc.view(np.int32), sc.view(np.int32))
        # a profile of several items: the mean of their rows, its own items excluded; duplicates count once in the exclusion
        profile = [nu + 1, nu + 5, nu + 2, nu + 5]
        emb = model.item_embeddings(train, space=space)
        q = emb[[1, 5, 2, 5]].astype(np.float64).mean(axis=0, keepdims=True)
        want64 = ref.nearest64(q, emb, 'cosine')
        pnb, psc = model.recommend_like(train, [profile], k=8, space=space)
        # the mean itself is formed in f32 on the device: L - 1 additions (each within u of a partial sum, itself within the sum of
        # the rows' norms) and a division move the query by at most u ((L - 1) / L sum ||e_i|| + ||q||), and a cosine moves by at
        # most twice the query's relative change
        norms = np.sqrt((emb[[1, 5, 2, 5]].astype(np.float64) ** 2).sum(axis=1))
        qn = float(np.sqrt((q ** 2).sum()))
        tol = ref.score_tolerance(q, emb, 'cosine') + (2 * ref.U24 * (0.75 * norms.sum() + qn) / qn if qn > 0 else 0.0)
        assert ref.check_lists(np.zeros(1, dtype=np.int64), pnb, psc, want64, {0: {1, 5, 2}}, 8, name + ' profile', tol, base=nu)[0] <= 1
        keep, _ = model.recommend_like(train, [profile], k=ni, space=space, exclude_liked=False) if ni <= 64 else (None, None)
        if keep is not None:
            assert set(profile) <= set(keep[0].tolist())
    if state0 is not None:
        assert (model.gnn.hoist, model.gnn._hoisted, model._towers) == state0
    assert np.array_equal(score().view(np.int32), pred0.view(np.int32))
    rec1 = model.recommend(train, k=10)
    assert np.array_equal(rec0[1], rec1[1]) and np.array_equal(rec0[2].view(np.int32), rec1[2].view(np.int32))


def test_hybrid_tower_space_needs_the_bert_table(hip):
    from deep_cbrs_amar_renaissance_amd.models import hybrid
    g = helpers.tiny_graph(seed=6)
    model = hybrid.HybridBertGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [32, 16], [16, 16]], clf_units=[16, 16])
    train = _Train(g['ratings'], g['n_users'], g['n_items'])
    with pytest.raises(ValueError, match='set_bert_table') as like_recommend:
        model.recommend(train, k=5)
    with pytest.raises(ValueError) as raised:
        model.similar_items(train, space='tower')
    assert str(raised.value) == str(like_recommend.value)
    assert model.item_embeddings(train, space='graph').shape[0] == g['n_items']          # the graph space does not read it


def test_unsupported_width_is_stated(hip):
    from deep_cbrs_amar_renaissance_amd.models import basic
    g = helpers.tiny_graph(seed=5)
    model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 18], clf_units=[16, 16])
    train = _Train(g['ratings'], g['n_users'], g['n_items'])
    assert model.item_embeddings(train, space='tower').shape == (g['n_items'], 18)
    with pytest.raises(NotImplementedError, match='18'):
        model.similar_items(train, space='tower')
    assert model.similar_items(train, k=3, space='graph')[1].shape == (g['n_items'], 3)


# ---- 3. experiment -----------------------------------------------------------------------------------------------------
def _run_experiment(tmp_path, name, similar, capture):
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.utilities.utils import setup_mlflow
    from tests.test_experiment_gpu import BASE_CONFIG
    cfg = json.loads(json.dumps(BASE_CONFIG))
    cfg['dataset'].update(capture['paths'])
    cfg['parameters']['epochs'] = 1
    if similar:
        cfg['parameters']['similar_items'] = similar
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
    return runs[0]


def test_experiment_similar_items_opt_in(hip, tmp_path, monkeypatch):
    import pandas as pd
    from deep_cbrs_amar_renaissance_amd import experiment
    from deep_cbrs_amar_renaissance_amd.data import synthetic
    ds = synthetic.ml1m(1)
    ds.train = ds.train[:40000]
    ds.test = ds.test[np.isin(ds.test[:, 0], ds.train[:, 0]) & np.isin(ds.test[:, 1], ds.train[:, 1])][:4000]
    ds.props = None
    paths = synthetic.write_dataset(ds, str(tmp_path / 'datasets'))
    capture = {'paths': {k: v for k, v in paths.items() if k != 'props_triples_filepath'}}
    original = experiment.Experimenter.write_similar_items

    def spy(self, **kwargs):
        capture['exp'] = self
        return original(self, **kwargs)

    monkeypatch.setattr(experiment.Experimenter, 'write_similar_items', spy)
    monkeypatch.chdir(tmp_path)
    run_on = _run_experiment(tmp_path, 'with_key', {'k': 10, 'metric': 'cosine', 'space': 'graph'}, capture)
    exp = capture.pop('exp')
    tsv = os.path.join(run_on, 'artifacts', 'predictions', 'similar_items_10.tsv')
    assert os.path.exists(tsv)
    frame = pd.read_csv(tsv, sep='\t', header=None)
    n_items = len(exp.trainset.items)
    assert len(frame) == n_items * 10 and frame.shape[1] == 3
    originals = set(np.asarray(exp.trainset.items).tolist())
    assert set(frame[0]) == originals and set(frame[1]) <= originals and not np.any(frame[0] == frame[1])
    assert frame.groupby(0, sort=False)[2].apply(lambda s: np.all(np.diff(s.to_numpy()) <= 0)).all()      # best first
    ids, nb, sc = exp.model.similar_items(exp.trainset, k=10, metric='cosine', space='graph')
    item_ids, nu = np.asarray(exp.trainset.items), len(exp.trainset.users)
    assert np.array_equal(frame[0].to_numpy(), np.repeat(item_ids[ids - nu], 10))
    assert np.array_equal(frame[1].to_numpy(), item_ids[nb - nu].reshape(-1))
    run_off = _run_experiment(tmp_path, 'without_key', None, capture)
    assert 'exp' not in capture
    rel = lambda root: sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, '**', '*'), recursive=True) if os.path.isfile(p))
    assert rel(run_off) == [p for p in rel(run_on) if 'similar_items' not in p]
