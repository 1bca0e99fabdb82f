"""CPU: the float64 restatement of the explanations (tests/explain_ref.py) on a hand-computed case, the host CSR builders, the
argument refusals of `explain`, the declarations, and the near-tie cap that the GPU grid's seeds must keep."""
import os
import re

import numpy as np
import pytest

from tests import explain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_a_hand_computed_case():
    # 5 items in the plane, 4 properties, 3 users.  dot products of the rows:
    #        i0 (1,0)  i1 (0,1)  i2 (1,1)  i3 (-1,0)  i4 (2,0)
    T = np.array([[1, 0], [0, 1], [1, 1], [-1, 0], [2, 0]], dtype=np.float32)
    grid = ref.sim_grid(T, 'dot')
    assert grid.tolist() == [[1, 0, 1, -1, 2], [0, 1, 1, 0, 0], [1, 1, 2, -1, 2], [-1, 0, -1, 1, -2], [2, 0, 2, -2, 4]]
    tol = ref.sim_tolerance(T, 'dot')
    assert np.isclose(tol[2, 4], 10 * 2.0 ** -24 * np.sqrt(2.0) * 2.0)
    props = [np.array([0, 1]), np.array([1]), np.array([0, 1, 2]), np.array([0, 3]), np.array([], dtype=np.int64)]
    weight = np.array([1.0, 0.5, 2.0, 4.0], dtype=np.float32)
    liked = [np.array([0, 1, 3, 4]), np.array([2]), np.array([], dtype=np.int64)]
    # user 0, target i2: sims to liked 0, 1, 3, 4 are 1, 1, -1, 2 -> evidence 4 (2), then 0 before 1 on the tie (1, 1), then 3 (-1)
    r = ref.explain_target(2, liked[0], grid, tol, props, weight, 3, 3)
    assert r['ev_items'].tolist() == [4, 0, 1, 3] and r['ev_sims'].tolist() == [2, 1, 1, -1]
    assert r['ev_flag'].tolist() == [False, True, True]               # ranks 1 and 2 are an exact tie of non-zero values
    # p0: liked 0 (1) and 3 (max(-1, 0) = 0): score 1 * 1 = 1, support 2;  p1: liked 0 (1) and 1 (1): 0.5 * 2 = 1, support 2;  p2: nobody
    assert r['prop_ids'].tolist() == [0, 1] and r['prop_scores'].tolist() == [1.0, 1.0] and r['prop_support'].tolist() == [2, 2]
    assert r['support_of'] == {0: 2, 1: 2, 2: 0}
    # user 0, target i0 is liked itself: it is neither evidence nor a supporter.  sims to 1, 3, 4: 0, -1, 2
    r = ref.explain_target(0, liked[0], grid, tol, props, weight, 2, 2)
    assert r['ev_items'].tolist() == [4, 1, 3] and r['ev_sims'].tolist() == [2, 0, -1]
    # p0: liked 3 only (sim -1 -> 0): score 0, support 1;  p1: liked 1 (sim 0): score 0, support 1: the tie goes to p0
    assert r['prop_ids'].tolist() == [0, 1] and r['prop_scores'].tolist() == [0.0, 0.0] and r['prop_support'].tolist() == [1, 1]
    assert r['prop_flag'].tolist() == [False, False]                  # sim -1 is sign-certain and sim 0 exact: float32 gives 0 and 0 too
    # user 1, target i3: liked {2}: sim -1; p0 shared with i2: support 1, score 0;  p3 nobody
    r = ref.explain_target(3, liked[1], grid, tol, props, weight, 2, 2)
    assert r['ev_items'].tolist() == [2] and r['prop_ids'].tolist() == [0] and r['prop_support'].tolist() == [1]
    ev, es, pr, ps, pc = ref.padded(r, 2, 2)
    assert ev.tolist() == [2, -1] and es[0] == -1 and np.isneginf(es[1]) and pr.tolist() == [0, -1] and np.isneginf(ps[1]) and pc.tolist() == [1, 0]
    # user 2 likes nothing; a -1 target is None
    lst = ref.explain_list([4, -1], liked[2], grid, tol, props, weight, 2, 2)
    assert lst[1] is None and len(lst[0]['ev_items']) == 0 and len(lst[0]['prop_ids']) == 0
    assert ref.padded(None, 1, 1)[0].tolist() == [-1]
    # cosine: a zero row scores 0
    Tz = np.array([[3, 4], [0, 0], [4, 3]], dtype=np.float32)
    gz = ref.sim_grid(Tz, 'cosine')
    assert np.all(gz[1] == 0) and np.isclose(gz[0, 2], 24.0 / 25.0)


def _graphs():
    from tests import helpers
    g = helpers.tiny_graph(n_users=12, n_items=9, n_ratings=60, seed=3, n_props=7, n_links=30)
    return g


class _Train:
    def __init__(self, ratings, n_users, n_items, adj):
        self.ratings, self.users, self.items, self.adj_matrix = ratings, np.arange(n_users), np.arange(n_items), adj


def test_liked_and_property_csr():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    from deep_cbrs_amar_renaissance_amd.data.preprocess import build_adjacency_matrix
    g = _graphs()
    nu, ni = g['n_users'], g['n_items']
    ratings = np.concatenate([g['ratings'], g['ratings'][:5]])          # duplicate pairs collapse
    ptr, items = rec.liked_csr(ratings, nu, ni)
    for u in range(nu):
        want = sorted({int(i) - nu for uu, i, l in g['ratings'] if uu == u and l == 1})
        assert items[ptr[u]:ptr[u + 1]].tolist() == want
    with pytest.raises(ValueError):
        rec.liked_csr(np.array([[0, nu + ni, 1]]), nu, ni)
    assert rec.liked_csr(np.zeros((0, 3), dtype=np.int64), nu, ni)[0].tolist() == [0] * (nu + 1)
    want_rows = [sorted({int(p) - ni for it, p, _ in g['triples'] if it == i}) for i in range(ni)]
    assert len(g['triples']) > len({(int(a), int(b)) for a, b, _ in g['triples']})          # the graph holds duplicate links
    kg = build_adjacency_matrix(g['ratings'], g['users'], g['items'], g['triples'], g['props'], type_adjacency='unary-kg')
    for adj in (g['adj'], kg):
        pptr, pids, df, longest = rec.item_property_csr(_Train(g['ratings'], nu, ni, adj))
        assert [pids[pptr[i]:pptr[i + 1]].tolist() for i in range(ni)] == want_rows
        assert df.tolist() == [sum(p in row for row in want_rows) for p in range(7)] and longest == max(len(r) for r in want_rows)
    unary = build_adjacency_matrix(g['ratings'], g['users'], g['items'])
    assert rec.item_property_csr(_Train(g['ratings'], nu, ni, unary)) is None
    assert rec.item_property_csr(_Train(g['ratings'], nu, ni, None)) is None


def test_idf_values():
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    w = rec.property_weights(np.array([1, 2, 8, 0]), 8, 'idf')
    assert w.dtype == np.float32 and np.array_equal(w, np.array([np.log(8.0), np.log(4.0), 0.0, 0.0]).astype(np.float32))
    assert np.array_equal(rec.property_weights(np.array([1, 2]), 8, 'none'), np.ones(2, dtype=np.float32))
    assert np.array_equal(ref.idf(np.array([1, 2, 8, 0]), 8), w)
    with pytest.raises(ValueError):
        rec.property_weights(np.array([1]), 8, 'tf')


def test_explain_refuses_bad_arguments_before_any_work():
    from deep_cbrs_amar_renaissance_amd import recommend as rec

    class Model(rec.SimilarSearch):
        def _embedding_spaces(self):
            raise AssertionError("the arguments are checked first")

    for bad in (dict(n_evidence=0), dict(n_evidence=17), dict(n_evidence=True), dict(n_properties=-1), dict(n_properties=17),
                dict(n_properties=2.0), dict(property_weight='tf'), dict(metric='euclid')):
        with pytest.raises(ValueError):
            Model().explain(None, **bad)
    with pytest.raises(NotImplementedError, match='6'):
        rec.check_width(6, 'item vectors')


def test_entry_point_is_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    decl = re.search(r'\bint\s+amar_explain_f32\s*\(([^;]*)\)\s*;', header)
    assert decl and 'amar_explain_f32' in capi.SIGNATURES
    assert len(decl.group(1).split(',')) == len(capi.SIGNATURES['amar_explain_f32'][1]) == 25
    assert callable(capi.explain)
    for name, value in (('K', 64), ('E', 16), ('PROP_ROW', capi.EXPLAIN_MAX_PROP_ROW)):
        assert re.search(r'#define\s+AMAR_EXPLAIN_MAX_{}\s+{}\b'.format(name, value), header)
    assert capi.EXPLAIN_MAX_PROP_ROW >= 256 and (capi.EXPLAIN_MAX_K, capi.EXPLAIN_MAX_E) == (64, 16)
    assert 'amar_explain.hip' in open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert 'amar_explain_f32' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_explanations_frame():
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import explanations_frame
    user_ids, item_ids, prop_ids = np.array([10, 20]), np.array([7, 8, 9]), np.array([100, 200])
    out = {'users': np.array([1, 0]), 'items': np.array([[2, 4], [3, -1]]),
           'evidence': np.array([[[3, 4], [2, -1]], [[4, -1], [-1, -1]]]),
           'evidence_sim': np.array([[[0.5, 0.25], [1.0, -np.inf]], [[0.75, -np.inf], [-np.inf, -np.inf]]], dtype=np.float32),
           'properties': np.array([[[1], [-1]], [[0], [-1]]]), 'property_score': np.array([[[2.0], [-np.inf]], [[1.5], [-np.inf]]], dtype=np.float32),
           'property_support': np.array([[[3], [0]], [[1], [0]]], dtype=np.int32)}
    frame = explanations_frame(out, user_ids, item_ids, prop_ids)
    assert frame['users'].tolist() == [20, 20, 10] and frame['items'].tolist() == [7, 9, 8] and frame['rank'].tolist() == [1, 2, 1]
    assert frame['evidence'].tolist() == ['8 9', '7', '9'] and frame['evidence_sim'].tolist() == ['0.5 0.25', '1.0', '0.75']
    assert frame['properties'].tolist() == ['200', '', '100'] and frame['property_support'].tolist() == ['3', '', '1']
    assert explanations_frame(out, user_ids, item_ids)['properties'].tolist() == ['1', '', '0']
    empty = dict(out, properties=np.zeros((2, 2, 0), dtype=np.int64), property_score=np.zeros((2, 2, 0), dtype=np.float32),
                 property_support=np.zeros((2, 2, 0), dtype=np.int32))
    assert explanations_frame(empty, user_ids, item_ids)['properties'].tolist() == ['', '', '']


def test_kernel_case_holds_what_the_gpu_grid_needs():
    case = ref.kernel_case(20, 17, 'cosine')
    assert case['lists'].shape == (37, 17) and len(set(case['users'].tolist())) == 23
    assert sorted({len(l) for l in case['liked']}) == sorted(ref.LIKED_LADDER)
    assert np.all(case['T'][ref.ZERO_ROW] == 0) and any(ref.ZERO_ROW in l for l in case['liked']) and ref.ZERO_ROW in case['lists']
    lens = {len(case['prop_rows'][i]) for i in case['lists'].reshape(-1) if i >= 0}
    assert set(ref.TARGET_ROWS) <= lens and case['max_prop_row'] == 300
    inside = sum(int(i in case['liked'][case['users'][j]]) for j in range(37) for i in case['lists'][j] if i >= 0)
    assert inside >= 10
    assert any(row[-1] == -1 for row in case['lists']) and any(-1 in row[:-1] and row[-1] >= 0 for row in case['lists'])
    assert all(np.all(np.diff(l) > 0) for l in case['liked']) and all(np.all(np.diff(r) > 0) for r in case['prop_rows'])
    exact = ref.exact_case()
    assert np.all(exact['T'] == np.round(exact['T'])) and np.all(np.log2(exact['weight']) == np.round(np.log2(exact['weight'])))


@pytest.mark.parametrize('metric', ref.GRID_METRIC)
@pytest.mark.parametrize('d', ref.GRID_D)
def test_gpu_grid_seeds_stay_within_the_near_tie_cap(d, metric):
    """The float64 reference itself marks at most 2 % of a case's written entries as near-ties, for every case of the GPU grid."""
    for K in ref.GRID_K:
        case = ref.kernel_case(d, K, metric)
        refs = ref.case_reference(case, metric, 16, 16)                # a smaller cut reads a prefix of the same rankings and flags
        for E, Q in ref.GRID_EQ:
            flagged, entries = ref.near_tie_rate(refs, E, Q)
            assert flagged <= ref.NEAR_TIE_CAP * entries, (d, K, metric, E, Q, flagged, entries)
