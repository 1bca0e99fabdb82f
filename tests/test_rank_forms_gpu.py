"""GPU: the score stage of the three fused rankers (csrc/amar_rank_score.inc) on every head form of tests/rank_forms_ref.py —
ragged c1 and hidden widths, every activation at the input, in the stack and at the dot, the widest layer a hidden one, the deepest
stack, strided tables — and the heads at and past the kernels' LDS capacity (pytest -m gpu).

Two layers of checks per form.  (a) values: the kernel's score matrix S against the float64 restatement, within
max(1e-6, 8 x the float32 restatement's own error); NaN anywhere fails (the strided tables carry NaN outside their window).
(b) order and counts, exactly, on S's own bits: recommend's lists, rank_of's counts, recommend_group's lists."""
import ctypes

import numpy as np
import pytest

from tests import chain_ref
from tests import group_recommend_ref as group_ref
from tests import helpers
from tests import rank_forms_ref as rf
from tests import rank_of_ref

pytestmark = pytest.mark.gpu

KS = (1, 10, 64)
STRATEGIES = ('mean', 'min', 'max')
EUNSUPPORTED = -2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _csr(segments):
    ptr = np.cumsum([0] + [len(s) for s in segments])
    return ptr.astype(np.int32), np.array([i for s in segments for i in sorted(s)], dtype=np.int32)


class Head:
    """A built case on the device: the packed stack, Tu / Ti as the form's (possibly strided) views, and the call arguments."""

    def __init__(self, capi, form, case):
        import torch
        self.case, self.dims, self.acts, self.in_act = case, case['dims'], case['acts'], case['in_act']
        ks, bs = [w for w, _ in case['layers']], [b for _, b in case['layers']]
        # the rankers take RANK_MAX_LAYERS MFMA layers plus the dot, one layer more than amar_chain_pack_f32 packs: that head's blob is
        # laid out by the restated packer (tests/chain_ref.py; test_chain_route_cpu.py holds it equal to the library's)
        blob = capi.chain_pack(ks, bs)[0] if len(ks) <= capi.CHAIN_MAX_LAYERS else chain_ref.pack(ks, bs)
        assert len(blob) == capi.rank_route('recommend', self.dims)['wpack_floats']
        self.blob = torch.from_numpy(np.ascontiguousarray(blob, dtype=np.float32)).cuda()
        c1 = self.dims[0]
        self.tables = []
        for table in (case['tu'], case['ti']):
            wide, off = rf.windowed(table, form.ld)
            wide_d = torch.from_numpy(wide).cuda()
            view = wide_d[:, off:off + c1]
            assert view.data_ptr() % 16 == 0 and (len(table) == 1 or (form.ld == 'c1') == view.is_contiguous())
            self.tables.append(view)
        self.tu, self.ti = self.tables

    def args(self, ti=None):
        return (self.tu, self.ti if ti is None else ti, self.blob, self.dims, self.acts, self.in_act)


def _score_matrix(capi, head):
    """S [n_users, n_items]: every pair's score as amar_recommend_f32 returns it, gathered over windows of 64 items (k = 64, no
    exclusion): -inf-padded lists hold every item of a window, so nothing is selected away."""
    n_users, n_items = int(head.tu.shape[0]), int(head.ti.shape[0])
    S = np.full((n_users, n_items), np.nan, dtype=np.float32)
    seen = np.zeros((n_users, n_items), dtype=bool)
    for w in range(0, n_items, 64):
        it, sc = capi.recommend(*head.args(head.ti[w:w + 64]), k=64)
        it, sc = it.cpu().numpy(), sc.cpu().numpy()
        r, c = np.nonzero(it >= 0)
        S[r, w + it[r, c]] = sc[r, c]
        seen[r, w + it[r, c]] = True
    assert seen.all()                                                     # every pair came back: nothing taken for padding
    return S


def _largest_slices(capi, symbol, m, n_items, dims, *extra):
    dims_c = (ctypes.c_int32 * len(dims))(*dims)
    fn = getattr(capi.load(), symbol)
    return max(s for s in range(1, 65) if fn(m, *extra, n_items, dims_c, len(dims) - 1, s) == s)


def _exclusions(k, route, n_items):
    """helpers.select_case_exclusions on this catalogue: user 0 has seen everything, user 1 all but k - 1, users 2..5 rows on the
    edges of 64-row groups and of the staged tile, plus — user 4 — the rows on either side of a step edge."""
    raw = helpers.select_case_exclusions(k, tile_rows=route['tile_items'], n=n_items, m=rf.N_USERS)
    step = 16 * route['pt']
    raw[4] = set(raw[4]) | {step - 1, step, route['tile_items'] - 1, route['tile_items']}
    return [{r for r in raw[u] if 0 <= r < n_items} for u in range(rf.N_USERS)]


def _check_values(form, head, S, label):
    case = head.case
    args = (case['tu'], case['ti'], case['layers'], case['acts'], case['in_act'])
    s32, s64 = rf.scores(*args, np.float32), rf.scores(*args, np.float64)
    assert not np.isnan(S).any(), label                                   # a read outside a strided window would land here
    tol = rf.bound(s32, s64)
    err = float(np.abs(S.astype(np.float64) - s64).max())
    print('rank form {:<20s} n_items {:>4d}  max |kernel - float64| {:.3e}  bound {:.3e}  (float32 restatement {:.3e})'.format(
        form.name, S.shape[1], err, tol, float(np.abs(s32.astype(np.float64) - s64).max())))
    assert err <= tol, (label, err, tol)
    if form.dot_act == 'relu':
        assert np.array_equal(S == 0, s64 == 0), label                    # tests/test_rank_forms_cpu.py: no pre-activation within tol of 0
        assert S.shape[1] == 1 or (S == 0).mean() > 0.25
    if form.dot_act is None and S.shape[1] > 1:
        assert (S < 0).any() and (S > 0).any()
    if S.shape[1] > 4:
        a, b, c = rf.TIE_ROWS(S.shape[1])
        assert np.array_equal(_bits(S[:, a]), _bits(S[:, b])) and np.array_equal(_bits(S[:, a]), _bits(S[:, c])), label


def _topk(S, excl, k):
    items, scores = np.full((len(S), k), -1, dtype=np.int64), np.full((len(S), k), -np.inf, dtype=np.float32)
    for u in range(len(S)):
        cand = np.array(sorted(set(range(S.shape[1])) - excl[u]), dtype=np.int64)
        order = cand[np.lexsort((cand, -S[u, cand].astype(np.float64)))][:k] if len(cand) else cand
        items[u, :len(order)], scores[u, :len(order)] = order, S[u, order]
    return items, scores


def _check_recommend(capi, form, head, S, route, label):
    n_users, n_items = S.shape
    slices = sorted({1, _largest_slices(capi, 'amar_recommend_slices', n_users, n_items, head.dims)})
    for k in KS:
        excl = _exclusions(k, route, n_items)
        e_ptr, e_items = _csr(excl)
        want_i, want_s = _topk(S, excl, k)
        for n_slices in slices:
            got_i, got_s = capi.recommend(*head.args(), k, excl_ptr=_dev(e_ptr), excl_items=_dev(e_items), n_slices=n_slices)
            got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
            assert np.array_equal(got_i.astype(np.int64), want_i), (label, k, n_slices)
            assert np.array_equal(_bits(got_s), _bits(want_s)), (label, k, n_slices)
            assert np.array_equal(got_i < 0, np.isneginf(got_s)) and (got_i[0] == -1).all()
        if form.dot_act is None and n_items > 1:                          # finite negative scores are list entries, not padding
            full = np.array([min(k, n_items - len(e)) for e in excl])
            assert np.array_equal((got_i >= 0).sum(1), full), (label, k)
            if k == 64 and n_items <= 80:                                 # nearly the whole catalogue is listed: its negative half too
                assert (got_s[got_i >= 0] < 0).sum() > n_users, (label, k)
            assert np.isfinite(got_s[got_i >= 0]).all()


def _check_rank_of(capi, form, head, S, route, label):
    n_users, n_items = S.shape
    rng = np.random.default_rng(17 + n_items)
    excl = _exclusions(10, route, n_items)
    pick = lambda n: sorted(rng.choice(n_items, size=min(n_items, n), replace=False).tolist())
    users = np.concatenate([np.arange(n_users), [3]])                     # every user, one of them twice
    targets = [pick(int(rng.integers(1, 9))) for _ in users]
    targets[0] = pick(3)                                                  # every item excluded: all counts 0
    targets[2] = pick(capi.RANK_OF_MAX_TARGETS)                           # a full entry
    targets[4] = sorted(set(pick(3)) | {min(excl[4])} if excl[4] else set(pick(3)))      # a target inside the exclusion row
    if n_items > 4:
        targets[6] = sorted(set(pick(4)) | set(rf.TIE_ROWS(n_items)))     # the tied rows themselves
    run_users = []
    if form.dot_act == 'relu' and n_items > 1:
        run_users = (7 + np.argsort(-(S[7:] == 0).sum(1), kind='stable')[:2]).tolist()     # the two users with the longest zero runs
        for j in run_users:                                               # the exact-zero run: targets inside it, and two above it
            zeros, above = np.nonzero(S[j] == 0)[0], np.nonzero(S[j] > 0)[0]
            assert n_items < 64 or len(zeros) >= 8, (label, j, len(zeros))
            targets[j] = sorted(set(zeros[:5].tolist()) | set(zeros[-2:].tolist()) | set(above[:2].tolist()))
    t_ptr, t_items = _csr(targets)
    e_ptr, e_items = _csr(excl)
    want = rank_of_ref.rank_of(S, users, excl, targets)
    m_split = len(capi.rank_of_entries(users, t_ptr)[0])
    for n_slices in sorted({1, _largest_slices(capi, 'amar_rank_of_slices', m_split, n_items, head.dims)}):
        got = tuple(t.cpu().numpy() for t in capi.rank_of(*head.args(), users, t_ptr, t_items, excl_ptr=_dev(e_ptr), excl_items=_dev(e_items),
                                                          n_slices=n_slices))
        assert np.array_equal(_bits(got[0]), _bits(want[0])), (label, n_slices)
        for g, w, what in zip(got[1:], want[1:], ('greater', 'eq_before', 'eq_after')):
            assert g.dtype == np.int32 and np.array_equal(g.astype(np.int64), w), (label, n_slices, what)
    lo, hi = t_ptr[0], t_ptr[1]
    assert not got[1][lo:hi].any() and not got[2][lo:hi].any() and not got[3][lo:hi].any()
    if n_items > 64:
        for j in run_users:                                               # the run was walked: ties counted on both sides
            assert got[2][t_ptr[j]:t_ptr[j + 1]].max() >= 3 and got[3][t_ptr[j]:t_ptr[j + 1]].max() >= 3, (label, j)


def _check_group(capi, form, head, S, route, label):
    n_users, n_items = S.shape
    excl = _exclusions(10, route, n_items)
    groups = [[u] for u in range(n_users)] + [[2, 9, 17]]
    g_excl = excl + [excl[6]]
    g_ptr, g_users = _csr(groups)
    e_ptr, e_items = _csr(g_excl)
    u_ptr, u_items = _csr(excl)
    n_slices = _largest_slices(capi, 'amar_recommend_group_slices', len(groups), n_items, head.dims, len(g_users))
    for k in (10, 64):
        one_i, one_s = capi.recommend(*head.args(), k, excl_ptr=_dev(u_ptr), excl_items=_dev(u_items))
        for strategy in STRATEGIES:
            for s in sorted({1, n_slices}):
                got_i, got_s = capi.recommend_group(*head.args(), k, _dev(g_ptr), _dev(g_users), strategy=strategy, excl_ptr=_dev(e_ptr),
                                                    excl_items=_dev(e_items), n_slices=s)
                got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
                want_i, want_s = group_ref.groups_topk(S, groups, g_excl, k, strategy)
                assert np.array_equal(got_i.astype(np.int64), want_i) and np.array_equal(_bits(got_s), _bits(want_s)), (label, k, strategy, s)
            if strategy == 'mean':                                        # a group of one is the member's own list, bit for bit
                assert np.array_equal(got_i[:n_users], one_i.cpu().numpy()) and np.array_equal(_bits(got_s[:n_users]), _bits(one_s.cpu().numpy()))


def _run_form(capi, form, dims=None, item_counts=None):
    dims = rf.dims_of(form) if dims is None else dims
    routes = {kind: capi.rank_route(kind, dims) for kind in ('recommend', 'group', 'rank_of')}
    route = routes['recommend']
    assert all(r['fits'] and (r['maxt'], r['pt'], r['tile_items']) == (route['maxt'], route['pt'], route['tile_items']) for r in routes.values())
    for n_items in (rf.item_counts(route) if item_counts is None else item_counts):
        label = '{} n_items={}'.format(form.name, n_items)
        head = Head(capi, form, rf.build(form, n_items, dims=dims))
        S = _score_matrix(capi, head)
        _check_values(form, head, S, label)
        _check_recommend(capi, form, head, S, route, label)
        _check_rank_of(capi, form, head, S, route, label)
        _check_group(capi, form, head, S, route, label)
    return routes


# ---- 1. every form of the grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', rf.FORM_NAMES)
def test_form(hip, name):
    """One head of the grid at 19 users and the three catalogue sizes of its route (1; one step + 3; one tile + one step + 3).
    Measured on the MI355X (max |kernel - float64| over the three sizes / the bound the test computed): see DESIGN.md, the table
    next to the score stage."""
    _run_form(hip, rf.FORMS[rf.FORM_NAMES.index(name)])


# ---- 1b. the variants of the one top-k body, where they must be amar_recommend_f32 ---------------------------------------------
@pytest.mark.parametrize('maxt', [1, 2, 4, 8])
def test_variants_that_add_nothing_equal_recommend(hip, maxt):
    """On each of the four kernel forms, item rows and score bits: (a) the cursor (+inf, -1), (b) the candidate list 0..n_items-1
    and (c) groups of one under `mean` return amar_recommend_f32's lists — 19 users, one tile + one step + 3 items, one slice and
    the most the *_slices query accepts, the exclusion rows of helpers.select_case_exclusions."""
    capi = hip
    forms = [f for f in rf.FORMS if capi.rank_route('recommend', rf.dims_of(f))['maxt'] == maxt]
    form = min(forms, key=lambda f: (max(rf.dims_of(f)), sum(rf.dims_of(f))))        # the narrowest head of the grid on this kernel form
    dims = rf.dims_of(form)
    route = capi.rank_route('recommend', dims)
    assert all(capi.rank_fits(kind, dims) for kind in ('recommend', 'among', 'group'))
    n_users, n_items = rf.N_USERS, route['tile_items'] + 16 * route['pt'] + 3
    head = Head(capi, form, rf.build(form, n_items, dims=dims))
    start = (_dev(np.full(n_users, -1)), _dev(np.full(n_users, np.inf), np.float32))
    ones = np.arange(n_users + 1), np.arange(n_users)                     # groups of one: the exclusion CSR over groups is the users'
    slices = sorted({1, _largest_slices(capi, 'amar_recommend_slices', n_users, n_items, dims)})
    group_slices = sorted({1, _largest_slices(capi, 'amar_recommend_group_slices', n_users, n_items, dims, n_users)})
    assert slices[-1] > 1 and group_slices[-1] > 1
    host = lambda pair: (pair[0].cpu().numpy(), _bits(pair[1].cpu().numpy()))
    same = lambda got, want: np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for k in KS:
        e_ptr, e_items = _csr(_exclusions(k, route, n_items))
        kw = dict(excl_ptr=_dev(e_ptr), excl_items=_dev(e_items))
        want = host(capi.recommend(*head.args(), k, n_slices=1, **kw))
        assert (want[0][0] == -1).all() and (want[0][2:] >= 0).any()
        for s in slices:
            assert same(host(capi.recommend(*head.args(), k, n_slices=s, **kw)), want), (form.name, k, s)
            assert same(host(capi.recommend_after(*head.args(), k, *start, n_slices=s, **kw)), want), (form.name, 'after', k, s)
            assert same(host(capi.recommend_among(*head.args(), k, np.arange(n_items), n_slices=s, **kw)), want), (form.name, 'among', k, s)
        for s in group_slices:
            got = capi.recommend_group(*head.args(), k, _dev(ones[0]), _dev(ones[1]), strategy='mean', n_slices=s, **kw)
            assert same(host(got), want), (form.name, 'group', k, s)


# ---- 2. capacity ---------------------------------------------------------------------------------------------------------------
def _raw_call(capi, kind, head, n_users, n_items, outs):
    """The entry point itself (ctypes), with valid arguments for a one-user, one-target call: its return code."""
    lib = capi.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dims_c = (ctypes.c_int32 * len(head.dims))(*head.dims)
    acts_c = (ctypes.c_int32 * len(head.acts))(*[capi.ACT_CODES[a] for a in head.acts])
    c1, n_layers = head.dims[0], len(head.acts)
    common = (p(head.tu), int(head.tu.stride(0)), n_users, p(head.ti), int(head.ti.stride(0)), n_items, c1, p(head.blob), dims_c, acts_c, n_layers,
              capi.ACT_CODES[head.in_act])
    ptr = _dev([0, 1])
    ids = _dev([0])
    o_i, o_s = outs
    if kind == 'recommend':
        return lib.amar_recommend_f32(*common, p(ids), 1, None, None, 4, 1, None, None, p(o_i), p(o_s), None)
    if kind == 'group':
        return lib.amar_recommend_group_f32(*common, p(ptr), p(ids), 1, 1, None, None, 0, float('-inf'), 4, 1, None, None, p(o_i), p(o_s), None)
    return lib.amar_rank_of_f32(*common, p(ids), 1, None, None, p(ptr), p(ids), 1, 1, 0, p(o_s), p(o_i), p(o_i[4:]), p(o_i[8:]), None)


@pytest.mark.parametrize('kind', ['recommend', 'group', 'rank_of'])
def test_capacity_limit(hip, kind):
    """The largest head the kernel takes (found by walking amar_rank_route, not from constants) runs through every check at the
    smallest catalogue that fills a tile and a ragged step of the next: the > 64 KB LDS attribute path at its limit.  The first
    head past it is refused by the entry point with AMAR_EUNSUPPORTED before any device call."""
    import torch
    capi = hip
    largest, past = rf.capacity_heads(lambda d: capi.rank_fits(kind, d))
    r = capi.rank_route(kind, largest)
    assert r['fits'] and r['large_lds'] and not capi.rank_route(kind, past)['fits']
    form = rf._f('capacity_' + kind, 128, largest[1:-1], 'the largest head ' + kind + ' takes')
    others = {k: capi.rank_fits(k, largest) for k in ('recommend', 'group', 'rank_of')}
    if all(others.values()):
        _run_form(capi, form, item_counts=[r['tile_items'], r['tile_items'] + 16 * r['pt'] + 3])
    else:                                                                 # recommend / group take heads rank_of does not
        assert kind != 'rank_of' and others['recommend'] and others['group']
        for n_items in (r['tile_items'], r['tile_items'] + 16 * r['pt'] + 3):
            head = Head(capi, form, rf.build(form, n_items))
            S = _score_matrix(capi, head)
            label = '{} n_items={}'.format(form.name, n_items)
            _check_values(form, head, S, label)
            _check_recommend(capi, form, head, S, r, label)
            _check_group(capi, form, head, S, r, label)
    # the first head past the limit
    form = rf._f('past_' + kind, 128, past[1:-1], 'the first head past ' + kind + "'s capacity")
    head_past = head = Head(capi, form, rf.build(form, 8, n_users=4))
    o_i, o_s = torch.full((16,), 7, dtype=torch.int32, device='cuda'), torch.full((16,), 7.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    lib = capi.load()
    before = lib.amar_last_hip_error()
    assert _raw_call(capi, kind, head, 4, 8, (o_i, o_s)) == EUNSUPPORTED
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert (o_i == 7).all() and (o_s == 7.0).all()                        # nothing was launched (rank_of: not even its memsets)
    # ... and the same call is served one unit narrower
    form = rf._f('at_' + kind, 128, largest[1:-1], 'the same call at the limit')
    head = Head(capi, form, rf.build(form, 8, n_users=4))
    assert _raw_call(capi, kind, head, 4, 8, (o_i, o_s)) == 0
    torch.cuda.synchronize()
    assert not (o_i == 7).all()
    with pytest.raises(capi.AmarError):                                   # the binding raises: it has no fallback of its own
        if kind == 'recommend':
            capi.recommend(*head_past.args(), 4)
        elif kind == 'group':
            capi.recommend_group(*head_past.args(), 4, _dev([0, 1]), _dev([0]))
        else:
            capi.rank_of(*head_past.args(), [0], [0, 1], [0])


# ---- 3. the models: a head the kernel refuses ranks by pairs ---------------------------------------------------------------------
class _Train:
    def __init__(self, ratings, n_users, n_items):
        self.ratings, self.users, self.items = ratings, np.arange(n_users), np.arange(n_items)


def _model(clf_units):
    import torch
    from deep_cbrs_amar_renaissance_amd.engine import set_seed
    from deep_cbrs_amar_renaissance_amd.models import basic
    set_seed(21)
    g = helpers.tiny_graph(n_users=40, n_items=60, n_ratings=500, seed=14)
    model = basic.BasicGCN(g['adj'], embedding_dim=8, n_hiddens=[8, 8], dense_units=[24, 24], clf_units=clf_units)
    helpers.randomize_biases(model, seed=2)
    with torch.no_grad():
        model.rs.clf.layers[-1].kernel.mul_(10.0)
    return model, _Train(g['ratings'], g['n_users'], g['n_items']), g


def _count(monkeypatch, capi, calls):
    for name in ('recommend', 'recommend_group', 'rank_of', 'topk_segmented'):
        fn = getattr(capi, name)
        monkeypatch.setattr(capi, name, (lambda fn, name: lambda *a, **kw: (calls.__setitem__(name, calls[name] + 1), fn(*a, **kw))[1])(fn, name))


@pytest.mark.parametrize('clf_units,fused', [([128, 128, 128], (False, False, False)), ([128, 128, 64], (True, True, False))])
def test_models_rank_heads_the_kernels_refuse(hip, monkeypatch, clf_units, fused):
    """clf_units [128, 128, 128]: no ranker takes the rest stack; [128, 128, 64]: recommend and group do, rank_of does not.  Every
    public ranking call answers, takes the route the query names, and returns what the pair route returns: bitwise where the
    call IS the pair route, and where it is fused the list a float32 score within 2e-6 of the pair route's must give (the bound
    the fused-against-pairs tests of test_recommend_gpu.py hold)."""
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    capi = hip
    model, train, g = _model(clf_units)
    nu, ni = g['n_users'], g['n_items']
    rest = [clf_units[0]] + clf_units[1:] + [1]
    assert tuple(capi.rank_fits(k, rest) for k in ('recommend', 'group', 'rank_of')) == fused
    assert model._recommend_route(train) == ('fused' if fused[0] else 'pairs')
    towers = model.rs.towers(*model._recommend_tables(train))
    score_fn = lambda u, i: model.rs.score_towers(towers, u, i)
    _, all_i, all_s = model._recommend_pairs(train, k=ni, exclude_seen=False)
    P = np.zeros((nu, ni), dtype=np.float32)                              # the pair route's score of every pair
    P[np.arange(nu)[:, None], all_i - nu] = all_s
    seen = [set() for _ in range(nu)]
    for u, i, _ in g['ratings'].tolist():
        seen[u].add(i - nu)
    calls = {name: 0 for name in ('recommend', 'recommend_group', 'rank_of', 'topk_segmented')}
    _count(monkeypatch, capi, calls)

    def took(name, is_fused, pairs_name='topk_segmented'):
        if is_fused:
            assert calls[name] >= 1 and calls['topk_segmented'] == 0, (name, calls)
        else:
            assert calls[name] == 0 and (pairs_name is None or calls[pairs_name] >= 1), (name, calls)
        for key in calls:
            calls[key] = 0

    def same_as_pairs(items, scores, want_i, want_s, table):
        """Bitwise, or — on the fused route — rank by rank the same pair-route score within 4e-6 and the kernel's own within 2e-6."""
        if np.array_equal(items, want_i) and np.array_equal(_bits(scores), _bits(want_s)):
            return True
        valid = want_i >= 0
        if not np.array_equal(items >= 0, valid):
            return False
        rows = np.nonzero(valid)[0]
        mine = table[rows, items[valid] - nu]
        return np.abs(scores[valid] - mine).max() <= 2e-6 and np.abs(mine - want_s[valid]).max() <= 4e-6

    # recommend
    _, got_i, got_s = model.recommend(train, k=10)
    took('recommend', fused[0])
    _, want_i, want_s = model._recommend_pairs(train, k=10)
    if fused[0]:
        assert same_as_pairs(got_i, got_s, want_i, want_s, P)
    else:
        assert np.array_equal(got_i, want_i) and np.array_equal(_bits(got_s), _bits(want_s))
    for key in calls:
        calls[key] = 0
    # group recommendation
    groups = [[0], [5, 3], [7, 8, 9, 30], list(range(0, 40, 3))]
    for strategy in STRATEGIES:
        got_i, got_s = model.recommend_group(train, groups, k=10, strategy=strategy)
        took('recommend_group', fused[1])
        ptr, members = rec.group_csr(groups, nu)
        excl = rec.group_exclusion_csr(train.ratings, ptr, members, nu, ni)
        rows, sc = rec.group_pairs(score_fn, ni, ptr, members, excl, 10, strategy, rec.check_min_score(None), towers[0].device)
        rows, sc = rows.cpu().numpy().astype(np.int64), sc.cpu().numpy()
        want_i = np.where(rows >= 0, rows + nu, -1)
        if fused[1]:
            union = [set().union(*[seen[u] for u in m]) for m in groups]
            agg_i, agg_s = group_ref.groups_topk(P, groups, union, 10, strategy)
            assert np.array_equal(np.where(agg_i >= 0, agg_i + nu, -1), want_i)
            assert np.array_equal(got_i >= 0, want_i >= 0) and np.abs(got_s[want_i >= 0] - sc[want_i >= 0]).max() <= 2e-6
            agg = np.stack([group_ref.aggregate(P, m, strategy) for m in groups])
            at = agg[np.nonzero(got_i >= 0)[0], got_i[got_i >= 0] - nu]
            assert np.abs(at - sc[want_i >= 0]).max() <= 4e-6
        else:
            assert np.array_equal(got_i, want_i) and np.array_equal(_bits(got_s), _bits(sc))
        for key in calls:
            calls[key] = 0
    # rank_items: the pair route for both heads
    pu, pi = np.repeat(np.arange(nu), ni), np.tile(np.arange(ni) + nu, nu)
    out = model.rank_items(train, pu, pi)
    took('rank_of', fused[2], pairs_name=None)
    rank, score = out['rank'].reshape(nu, ni), out['score'].reshape(nu, ni)
    assert np.array_equal(_bits(score), _bits(P))
    for u in range(nu):
        want = rank_of_ref.positions(P[u], seen[u])
        assert all(rank[u, i] == want.get(i, 0) for i in range(ni)), u
    # evaluate_ranking with the cut-off-free metrics, and one validated epoch
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_rank_metrics
    from tests.test_validation_gpu import _held_out
    test = _held_out(g, np.random.default_rng(2))
    relevant = [set() for _ in range(nu)]
    for u, i, y in test.tolist():
        if y == 1:
            relevant[u].add(i - nu)
    got = model.evaluate_ranking(train, test, [5], rank_metrics=('auc', 'mrr', 'map'))
    assert calls['rank_of'] == 0 and calls['recommend'] == (1 if fused[0] else 0)
    want = full_ranking_rank_metrics(P, relevant, seen)
    for key in ('auc', 'mrr', 'map'):
        assert abs(got[key] - want[key]) <= 1e-12, key
    assert got['rank_metrics_users'] == want['rank_metrics_users']
    if not fused[0]:                                                      # the cut-off metrics are the pair route's lists'
        from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics
        plain = full_ranking_metrics(*model._recommend_pairs(train, k=5)[:2], test, [5])
        assert {key: got[key] for key in plain} == plain


def test_fit_validates_a_head_the_kernels_refuse(hip):
    from tests.test_validation_gpu import _bce_model, _bce_sequence, _validation_args
    g, seq = _bce_sequence(shuffle=True)
    model = _bce_model(g, 'BasicGCN', clf_units=[128, 128, 128])
    _, ranking, test = _validation_args(g)
    ranking = dict(ranking, ks=[5], rank_metrics=['auc'])
    assert model._recommend_route(ranking['trainset']) == 'pairs'
    hist = model.fit(seq, epochs=1, verbose=False, validation_ranking=ranking)
    assert len(hist['val_auc']) == 1 and 0.0 <= hist['val_auc'][0] <= 1.0
    again = model.evaluate_ranking(ranking['trainset'], test, [5], rank_metrics=['auc'])
    assert hist['val_auc'][0] == again['auc']
    assert all(hist['val_' + key][0] == value for key, value in again.items() if key != 'rank_metrics_users' and 'val_' + key in hist)
