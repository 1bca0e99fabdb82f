"""Host: similarity search (`similar_items` / `similar_users` / `recommend_like`, amar_nearest_f32) — the float64 reference's own
rules, the entry point's argument checks (they run before any device call) and the model surface.  No device."""

import numpy as np
import pytest

from tests import helpers, similar_ref as ref

EINVAL, EUNSUPPORTED = -1, -2


# ---- 1. the reference's own rules ------------------------------------------------------------------------------------
def test_reference_zero_row_scores_zero():
    Q = np.array([[0, 0, 0, 0], [1, 2, 0, 0]], dtype=np.float32)
    T = np.array([[3, 0, 0, 0], [0, 0, 0, 0], [2, 4, 0, 0]], dtype=np.float32)
    cos = ref.nearest64(Q, T, 'cosine')
    assert np.all(np.isfinite(cos)) and np.all(cos[0] == 0) and np.all(cos[:, 1] == 0)
    assert cos[1, 2] == pytest.approx(1.0, abs=1e-15) and cos[1, 0] == pytest.approx(1 / np.sqrt(5), abs=1e-15)
    dot = ref.nearest64(Q, T, 'dot')
    assert np.array_equal(dot, np.array([[0, 0, 0], [3, 0, 10]], dtype=np.float64))
    with pytest.raises(ValueError):
        ref.nearest64(Q, T, 'l2')


def test_reference_ties_exclusion_padding():
    grid = np.array([0.5, 0.9, 0.5, 0.9, 0.1])
    rows, scores = ref.topk64(grid, set(), 3)
    assert rows.tolist() == [1, 3, 0] and scores.tolist() == [0.9, 0.9, 0.5]          # ties by row id
    rows, scores = ref.topk64(grid, {1, 0}, 4)
    assert rows.tolist() == [3, 2, 4, -1] and scores[:3].tolist() == [0.9, 0.5, 0.1] and np.isneginf(scores[3])
    rows, scores = ref.topk64(grid, set(range(5)), 2)
    assert rows.tolist() == [-1, -1] and np.all(np.isneginf(scores))


def test_reference_checker_accepts_truth_and_rejects_a_swap():
    Q, T, excl = ref.planted_case(90, 8, 'cosine', seed=1, m=5)
    want = ref.nearest64(Q, T, 'cosine')
    lists = [ref.topk64(want[j], excl[j], 4) for j in range(5)]
    rows = np.stack([r for r, _ in lists])
    scores = np.stack([s for _, s in lists]).astype(np.float32)
    tol = ref.score_tolerance(Q, T, 'cosine')
    assert ref.check_lists(np.arange(5), rows, scores, want, excl, 4, 'truth', tol)[0] == 0
    bad = rows.copy()
    bad[2, [0, 1]] = bad[2, [1, 0]]
    with pytest.raises(AssertionError):
        ref.check_lists(np.arange(5), bad, scores, want, excl, 4, 'swap', tol)


@pytest.mark.parametrize('metric', ['dot', 'cosine'])
def test_f32_evaluation_stays_within_the_near_tie_cap(metric):
    """The seeds of the GPU kernel test (tests/test_similar_gpu.py:case_seed), with the shift of helpers.seed_offset(): an f32 numpy
    evaluation of the same data meets the derived score bound and differs from the float64 ranking in at most 3 of 37 lists."""
    from tests.test_similar_gpu import MAX_NEAR_TIE_QUERIES, case_seed
    for n_rows, d in ((17, 36), (3191, 4), (3191, 512)):
        Q, T, excl = ref.planted_case(n_rows, d, metric, case_seed(n_rows, d, metric))
        want = ref.nearest64(Q, T, metric)
        rows, scores = ref.nearest32(Q, T, metric, 10, excl)
        differing, _ = ref.check_lists(np.arange(len(Q)), rows, scores, want, excl, 10, 'f32 numpy', ref.score_tolerance(Q, T, metric))
        assert differing <= MAX_NEAR_TIE_QUERIES


# ---- 2. entry-point argument checks ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from deep_cbrs_amar_renaissance_amd import capi
    return capi.load()


def _call(lib, **over):
    """amar_nearest_f32 with fake (aligned, never dereferenced) pointers: every case below returns before any device call."""
    a = dict(Q=0x1000, ldq=8, n_queries=5, T=0x2000, ldt=8, n_rows=7, d=8, metric=1, query_rows=None, m=5, excl_ptr=None, excl_rows=None,
             k=3, n_slices=0, ws_rows=None, ws_scores=0x3000, out_rows=0x4000, out_scores=0x5000)
    a.update(over)
    return lib.amar_nearest_f32(a['Q'], a['ldq'], a['n_queries'], a['T'], a['ldt'], a['n_rows'], a['d'], a['metric'], a['query_rows'], a['m'],
                                a['excl_ptr'], a['excl_rows'], a['k'], a['n_slices'], a['ws_rows'], a['ws_scores'], a['out_rows'],
                                a['out_scores'], None)


@pytest.mark.parametrize('over', [dict(Q=None), dict(T=None), dict(m=-1, query_rows=0x6000), dict(n_queries=-1), dict(n_rows=-1), dict(d=-4),
                                  dict(k=0), dict(k=-3), dict(metric=7), dict(metric=-1), dict(m=4), dict(excl_ptr=0x6000),
                                  dict(ldq=4), dict(ldt=4), dict(ws_scores=None), dict(n_slices=3)])
def test_entry_point_invalid_arguments(lib, over):
    assert _call(lib, **over) == EINVAL, over


@pytest.mark.parametrize('over', [dict(d=6), dict(d=516, ldq=516, ldt=516), dict(d=0), dict(k=65), dict(ldq=10), dict(ldt=9),
                                  dict(Q=0x1004), dict(T=0x2008)])
def test_entry_point_unsupported_shapes(lib, over):
    assert _call(lib, **over) == EUNSUPPORTED, over


def test_entry_point_empty_call_is_ok(lib):
    assert _call(lib, m=0, n_queries=0) == 0
    assert _call(lib, m=0, n_queries=0, d=512, ldq=512, ldt=640, k=64, metric=0, ws_scores=None) == 0


def test_nearest_slices(lib):
    s = lib.amar_nearest_slices
    assert s(37, 3191, 64, 1) == 1
    assert s(37, 0, 64, 0) == 1 and s(0, 100, 64, 0) == 1
    # d = 64 stages 128 rows per tile: 3191 rows are 25 tiles; slices cover whole tiles, so 2 -> 13 + 12 and 5 -> 5 x 5
    assert s(37, 3191, 64, 2) == 2 and s(37, 3191, 64, 5) == 5
    assert s(37, 3191, 64, 64) == 25                     # no more slices than tiles
    assert s(37, 3191, 64, 7) == 7 and s(37, 3191, 64, 9) == 9 and s(37, 3191, 64, 10) == 9      # ceil(25 / 10) = 3 tiles: 9 slices
    # d = 512 stages 32 rows per tile, d = 4 stages 256
    assert s(37, 3191, 512, 64) == 50 and s(37, 3191, 4, 64) == 13                  # 100 tiles: 2 per slice; 13 tiles
    # automatic: few query blocks -> slices of at least four tiles, at most 16; many blocks -> 1
    assert s(37, 3191, 64, 0) == 5                       # cap 25 // 4 = 6 wanted -> ceil(25 / 6) = 5 tiles each -> 5 slices
    assert s(37, 100000, 64, 0) == 16
    assert s(100000, 3191, 64, 0) == 1
    assert s(37, 17, 64, 0) == 1 and s(37, 17, 64, 5) == 1
    assert s(-1, 10, 64, 0) == EINVAL and s(1, -10, 64, 0) == EINVAL
    assert s(1, 10, 6, 0) == EUNSUPPORTED and s(1, 10, 516, 0) == EUNSUPPORTED


def test_workspace_floats(lib):
    w = lib.amar_nearest_workspace_floats
    assert w(37, 3191, 10, 0, 1) == 0
    assert w(37, 3191, 10, 1, 1) == 3192 + 40            # inverse norms, both parts rounded up to 4
    assert w(37, 3191, 10, 0, 5) == 37 * 5 * 10
    assert w(37, 3191, 10, 1, 5) == 3192 + 40 + 37 * 5 * 10
    assert w(37, 3191, 0, 1, 1) == EINVAL and w(37, 3191, 10, 7, 1) == EINVAL


def test_nearest_supported():
    from deep_cbrs_amar_renaissance_amd import capi
    assert capi.nearest_supported(4, 1) and capi.nearest_supported(512, 64) and capi.nearest_supported(36, 10)
    assert not capi.nearest_supported(6, 10) and not capi.nearest_supported(516, 10) and not capi.nearest_supported(0, 10)
    assert not capi.nearest_supported(64, 65) and not capi.nearest_supported(64, 0)


# ---- 3. the model surface ------------------------------------------------------------------------------------------
class _Train:
    def __init__(self, n_users, n_items):
        self.users, self.items, self.ratings = np.arange(n_users), np.arange(n_items), np.zeros((0, 3), dtype=np.int64)


def _models():
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    g = helpers.tiny_graph(seed=1)
    return {'BasicRS': basic.BasicRS(dense_units=[32, 16], clf_units=[16, 16]),
            'BasicGCN': basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8]),
            'HybridCBRS': hybrid.HybridCBRS(feature_based=False, dense_units=[[32, 16], [64, 16], [32, 8]], clf_units=[16]),
            'HybridBertGCN': hybrid.HybridBertGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[[24, 24], [32, 16], [16, 16]], clf_units=[16, 16])}, g


def test_space_resolution_per_model_class():
    models, _ = _models()
    want = {'BasicRS': ('tower',), 'BasicGCN': ('graph', 'tower'), 'HybridCBRS': ('tower',), 'HybridBertGCN': ('graph', 'tower')}
    for name, model in models.items():
        assert tuple(model._embedding_spaces()) == want[name], name
        assert model._resolve_space(None) == want[name][0], name                      # 'graph' where the model has a gnn
        assert model._resolve_space('tower') == 'tower'
        with pytest.raises(ValueError):
            model._resolve_space('bert')
    for name in ('BasicRS', 'HybridCBRS'):
        with pytest.raises(ValueError, match='tower'):                                    # the error names the spaces the model has
            models[name].similar_items(_Train(40, 30), space='graph')
        with pytest.raises(ValueError, match='tower'):
            models[name].item_embeddings(_Train(40, 30), space='graph')


def test_argument_checks_come_before_any_device_work():
    models, g = _models()
    model, train = models['BasicGCN'], _Train(g['n_users'], g['n_items'])
    nu, ni = g['n_users'], g['n_items']
    with pytest.raises(ValueError):
        model.similar_items(train, items=[nu - 1])                                        # a user id is no item node id
    with pytest.raises(ValueError):
        model.similar_items(train, items=[nu + ni])
    with pytest.raises(ValueError):
        model.similar_users(train, users=[nu])
    with pytest.raises(ValueError):
        model.similar_users(train, users=[-1])
    with pytest.raises(ValueError):
        model.similar_items(train, items=[0.5])
    for bad_metric in ('l2', None, 7):
        with pytest.raises(ValueError):
            model.similar_items(train, metric=bad_metric)
        with pytest.raises(ValueError):
            model.similar_users(train, metric=bad_metric)
        with pytest.raises(ValueError):
            model.recommend_like(train, [[nu]], metric=bad_metric)
    for bad_k in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            model.similar_items(train, k=bad_k)
        with pytest.raises(ValueError):
            model.recommend_like(train, [[nu]], k=bad_k)
    with pytest.raises(ValueError, match='empty'):
        model.recommend_like(train, [[nu], []])
    with pytest.raises(ValueError):
        model.recommend_like(train, [[nu - 1]])                                           # profiles hold item node ids


def test_nearest_argument_checks():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    q, t = np.zeros((3, 8), dtype=np.float32), np.zeros((5, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        rec.nearest(q, t, k=0)
    with pytest.raises(ValueError):
        rec.nearest(q, t, metric='manhattan')
    ptr, rows = rec.lists_csr([[4, 1, 1], [], [0]], 5)
    assert ptr.tolist() == [0, 2, 2, 3] and rows.tolist() == [1, 4, 0] and ptr.dtype == np.int32 and rows.dtype == np.int32
    with pytest.raises(ValueError):
        rec.lists_csr([[5]], 5)
    with pytest.raises(NotImplementedError, match='6'):
        rec.check_width(6)
    with pytest.raises(NotImplementedError, match='516'):
        rec.check_width(516)
    assert rec.check_width(512) == 512


def test_every_generated_model_class_has_the_methods():
    from deep_cbrs_amar_renaissance_amd.models import basic, hybrid
    classes = [basic.BasicRS, hybrid.HybridCBRS]
    for module, table in ((basic, basic.BASIC_GNNS), (hybrid, hybrid.HYBRID_GNNS)):
        for parent, gnns, name_getter in table:
            prefix = 'Basic' if module is basic else 'HybridBert'
            for gnn in gnns:
                name = name_getter(gnn.__name__) if name_getter is not None else prefix + gnn.__name__
                classes.append(getattr(module, name))
    assert len(classes) == 32
    for cls in classes:
        for method in ('similar_items', 'similar_users', 'recommend_like', 'user_embeddings', 'item_embeddings'):
            assert callable(getattr(cls, method, None)), (cls.__name__, method)
