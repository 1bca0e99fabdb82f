"""GPU: recommendation from per-user candidate lists (csrc/amar_rank_lists.hip, recommend.py:recommend_from) — pytest -m gpu.

The yardstick of the kernel is the kernel it was made from, and the comparison is exact: for lists C_j,
capi.recommend_lists(lists=C, excl=E) must return the item rows and the score bits of capi.recommend(excl_u = E_u u complement(C_u))
— one score routine and one user fragment, so the same bits per pair; a strict total order, so the same lists.  One value check per
kernel form against the float64 restatement of tests/rank_forms_ref.py shows the gather reads inside its window.  The models are held
to their own complete rankings, struck down to every user's list on the host; evaluate_ranking_sampled to the host metrics."""
import ctypes

import numpy as np
import pytest

from tests import among_ref
from tests import helpers
from tests import rank_forms_ref as rf
from tests.test_recommend_among_gpu import Head, _bits, _case, _csr, _dev, _form_of, _model_case, _same
from tests.test_recommend_from_cpu import lists_lds_bytes

pytestmark = pytest.mark.gpu

KS = (1, 10, 64)
N_USERS = 24
EINVAL, EUNSUPPORTED = -1, -2


def _lists_csr(lists):
    """Host CSR (ptr, rows) of one ascending list per listed row."""
    ptr = np.cumsum([0] + [len(c) for c in lists])
    return ptr.astype(np.int64), (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int64)


_HEADS = {}


def _head(capi, maxt):
    """Head and route of a kernel form, built once and shared (nothing writes to it): 24 users, three steps + 5 items."""
    if maxt not in _HEADS:
        form = _form_of(maxt)
        route = capi.rank_route('lists', rf.dims_of(form))
        assert route['fits'] and route['maxt'] == maxt
        n_items = 3 * 16 * route['pt'] + 5
        _HEADS[maxt] = (form, route, n_items, Head(capi, rf.build(form, n_items, n_users=N_USERS)))
    return _HEADS[maxt]


# ---- 1. the kernel against the kernel it was made from ---------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('maxt', [1, 2, 4, 8])
def test_lists_equal_recommend_with_the_complement_excluded(hip, maxt, k):
    capi = hip
    form, route, n, head = _head(capi, maxt)
    step = 16 * route['pt']
    assert n == 3 * step + 5
    # the lengths, ordered so that each workgroup of four listed rows walks 0 / all / short / two steps, 1 / two steps / one ragged / one
    # (k - 1 candidates where the catalogue has that many: the <8, 1> form's 53 items cannot hold 63 distinct ones, there the list is all items)
    lengths = [0, n, min(k - 1, n), 2 * step, 1, step + 1, step - 1, step]
    rng = np.random.default_rng(50 + k)
    cand_of = [np.sort(rng.choice(n, size=lengths[u % 8], replace=False)) for u in range(N_USERS)]
    assert len(cand_of[22]) == step - 1 and len(cand_of[23]) == step
    excl = helpers.select_case_exclusions(k, tile_rows=step, n=n, m=N_USERS)
    excl = [set(r for r in excl[u] if 0 <= r < n) for u in range(N_USERS)]
    excl[22] = set(cand_of[22].tolist()) | {0, n - 1}                     # every candidate is seen
    excl[23] = set(cand_of[23].tolist()[1:])                              # ... all but one
    assert any(excl[u] - set(cand_of[u].tolist()) for u in range(N_USERS) if len(cand_of[u]))     # rows hold items outside the list
    everything = set(range(n))
    e_ptr, e_items = _csr(excl)
    w_ptr, w_items = _csr([excl[u] | (everything - set(cand_of[u].tolist())) for u in range(N_USERS)])
    c_ptr, c_items = _csr([everything - set(cand_of[u].tolist()) for u in range(N_USERS)])
    listed = 0
    for users in (None, np.array([23, 22, 17, 17, 5, 4, 1, 0], dtype=np.int32), np.array([20, 13, 13, 6, 2], dtype=np.int32),
                  np.array([9], dtype=np.int32)):
        u_dev = None if users is None else _dev(users)
        order = np.arange(N_USERS) if users is None else users
        m = len(order)
        want_i, want_s = capi.recommend(*head.args(), k, users=u_dev, excl_ptr=_dev(w_ptr), excl_items=_dev(w_items))
        want_i, want_s = want_i.cpu().numpy(), want_s.cpu().numpy()
        ptr, rows = _lists_csr([cand_of[u] for u in order])
        for on_device in (False, True):
            c = (_dev(ptr), _dev(rows)) if on_device else (ptr, rows)
            got_i, got_s = capi.recommend_lists(*head.args(), k, *c, users=u_dev, excl_ptr=_dev(e_ptr), excl_items=_dev(e_items))
            got_i, got_s = got_i.cpu().numpy(), got_s.cpu().numpy()
            assert got_i.dtype == np.int32 and got_i.shape == (m, k) == got_s.shape
            assert np.array_equal(got_i, want_i), (form.name, k, m, on_device)
            assert np.array_equal(_bits(got_s), _bits(want_s)), (form.name, k, m, on_device)
        for j, u in enumerate(order):
            assert set(want_i[j][want_i[j] >= 0].tolist()) <= set(cand_of[u].tolist()) - excl[u]
            assert (want_i[j] >= 0).sum() == min(k, len(set(cand_of[u].tolist()) - excl[u]))
        assert (want_i[order == 22] == -1).all() and ((want_i[order == 23] >= 0).sum(1) == 1).all()
        listed += int((want_i >= 0).sum())
        # without exclusions, too
        open_i, open_s = capi.recommend(*head.args(), k, users=u_dev, excl_ptr=_dev(c_ptr), excl_items=_dev(c_items))
        got_i, got_s = capi.recommend_lists(*head.args(), k, ptr, rows, users=u_dev)
        assert np.array_equal(got_i.cpu().numpy(), open_i.cpu().numpy()) and np.array_equal(_bits(got_s.cpu().numpy()), _bits(open_s.cpu().numpy()))
    assert listed > 0


# ---- 2. values: the gather reads inside its window ---------------------------------------------------------------------------------
@pytest.mark.parametrize('maxt', [1, 2, 4, 8])
def test_values_against_float64(hip, maxt):
    """k = 64 over 64 candidates per user without exclusions returns every candidate's score; against the float64 restatement within
    max(1e-6, 8 x the float32 restatement's own error), the rule of the among test.  Tu and Ti are windows of tensors whose padding is
    NaN: a gathered read outside a row's window would land in the scores."""
    capi = hip
    form, route, n, head = _case(capi, maxt)                              # the among test's case: two tiles + 37 items, ld = 2 c1
    case = head.case
    nu = case['tu'].shape[0]
    rng = np.random.default_rng(7)
    cand = [np.sort(rng.choice(n, size=64, replace=False)) for _ in range(nu)]
    cand[0][[0, -1]] = 0, n - 1
    got_i, got_s = (t.cpu().numpy() for t in capi.recommend_lists(*head.args(), 64, *_lists_csr(cand)))
    assert all((np.sort(got_i[u]) == cand[u]).all() for u in range(nu))   # every candidate, nothing else, nothing padded
    S = np.full((nu, n), np.nan, dtype=np.float32)
    S[np.arange(nu)[:, None], got_i] = got_s
    args = (case['tu'], case['ti'], case['layers'], case['acts'], case['in_act'])
    s32, s64 = rf.scores(*args, np.float32), rf.scores(*args, np.float64)
    at = (np.arange(nu)[:, None], np.stack(cand))
    assert not np.isnan(S[at]).any()
    tol = rf.bound(s32[at], s64[at])
    err = float(np.abs(S[at].astype(np.float64) - s64[at]).max())
    print('lists form {:<12s} max |kernel - float64| {:.3e}  bound {:.3e}'.format(form.name, err, tol))
    assert err <= tol, (form.name, err, tol)
    want_i, want_s = among_ref.topk_among(S, range(nu), None, cand, 64, per_user=True)            # the order, on the kernel's own bits
    assert np.array_equal(got_i.astype(np.int64), want_i) and np.array_equal(_bits(got_s), _bits(want_s))


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------------
def _raw(capi, h, n_users, n_items, k, cand_ptr, cand_items, outs, m=None, null=()):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dims_c = (ctypes.c_int32 * len(h.dims))(*h.dims)
    acts_c = (ctypes.c_int32 * len(h.acts))(*[capi.ACT_CODES[a] for a in h.acts])
    a = dict(Tu=p(h.tu), Ti=p(h.ti), wpack=p(h.blob), dims=dims_c, acts=acts_c)
    a.update({name: None for name in null})
    return capi.load().amar_recommend_lists_f32(a['Tu'], int(h.tu.stride(0)), n_users, a['Ti'], int(h.ti.stride(0)), n_items, h.dims[0],
                                                a['wpack'], a['dims'], a['acts'], len(h.acts), capi.ACT_CODES[h.in_act], None,
                                                n_users if m is None else m, None, None, p(cand_ptr), p(cand_items), k, p(outs[0]), p(outs[1]), None)


def test_capacity(hip):
    import torch
    capi = hip
    for dims in [rf.dims_of(f) for f in rf.FORMS] + [[128, 128, 1], [128, 128, 64, 1], [128, 128, 128, 1]]:
        assert capi.rank_route('lists', dims)['lds_bytes'] == lists_lds_bytes(dims), dims
    # a head 'recommend' has no room for and 'lists' has, found by asking: the grid's heads first, then 128 -> 128 -> w -> 1
    asked = [rf.dims_of(f) for f in rf.FORMS] + [[128, 128, w, 1] for w in range(16, 129, 16)]
    only = [d for d in asked if capi.rank_fits('lists', d) and not capi.rank_fits('recommend', d)]
    assert only, 'no head between the two capacities'
    dims = only[0]
    n, nu = 80, 6
    head = Head(capi, rf.build(rf._f('lists_only', dims[0], dims[1:-1], "past recommend's capacity, inside lists'"), n, n_users=nu))
    with pytest.raises(capi.AmarError):
        capi.recommend(*head.args(), 4)
    rng = np.random.default_rng(11)
    cand = [np.sort(rng.choice(n, size=c, replace=False)) for c in (40, 0, 17, 64, 1, 33)]
    got_i, got_s = (t.cpu().numpy() for t in capi.recommend_lists(*head.args(), 64, *_lists_csr(cand)))
    case = head.case
    args = (case['tu'], case['ti'], case['layers'], case['acts'], case['in_act'])
    s32, s64 = rf.scores(*args, np.float32), rf.scores(*args, np.float64)
    tol = rf.bound(s32, s64)
    S = np.full((nu, n), np.nan, dtype=np.float32)
    for u in range(nu):
        valid = got_i[u] >= 0
        assert sorted(got_i[u][valid].tolist()) == cand[u].tolist() and np.isneginf(got_s[u][~valid]).all()
        S[u, got_i[u][valid]] = got_s[u][valid]
        err = float(np.abs(S[u, cand[u]].astype(np.float64) - s64[u, cand[u]]).max()) if len(cand[u]) else 0.0
        print('lists-only head {} user {} max |kernel - float64| {:.3e}  bound {:.3e}'.format(dims, u, err, tol))
        assert err <= tol, (dims, u, err, tol)
    want_i, want_s = among_ref.topk_among(S, range(nu), None, cand, 64, per_user=True)
    assert np.array_equal(got_i.astype(np.int64), want_i) and np.array_equal(_bits(got_s), _bits(want_s))
    # a head that fits neither: refused before any launch
    neither = [128, 128, 128, 1]
    assert not capi.rank_fits('lists', neither) and not capi.rank_fits('recommend', neither)
    past = Head(capi, rf.build(rf._f('past_lists', 128, neither[1:-1], 'past every capacity'), 8, n_users=4))
    o_i = torch.full((4 * 4,), 7, dtype=torch.int32, device='cuda')
    o_s = torch.full((4 * 4,), 7.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    before = capi.load().amar_last_hip_error()
    assert _raw(capi, past, 4, 8, 4, _dev([0, 1, 2, 3, 3]), _dev([0, 1, 2]), (o_i, o_s)) == EUNSUPPORTED
    with pytest.raises(capi.AmarError):
        capi.recommend_lists(*past.args(), 4, [0, 1, 2, 3, 3], [0, 1, 2])
    assert capi.load().amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert (o_i == 7).all() and (o_s == 7.0).all()


# ---- 4. refusals: nothing is launched ------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import torch
    capi = hip
    lib = capi.load()
    form, route, n, head = _head(capi, 1)
    o_i = torch.full((N_USERS * 65,), 7, dtype=torch.int32, device='cuda')
    o_s = torch.full((N_USERS * 65,), 7.0, dtype=torch.float32, device='cuda')
    ptr, rows = _dev(np.minimum(np.arange(N_USERS + 1), 3)), _dev([0, 1, 2])
    torch.cuda.synchronize()
    before = lib.amar_last_hip_error()
    assert _raw(capi, head, N_USERS, n, 65, ptr, rows, (o_i, o_s)) == EUNSUPPORTED                     # k = 65
    assert _raw(capi, head, N_USERS, n, 0, ptr, rows, (o_i, o_s)) == EINVAL
    for name in ('Tu', 'Ti', 'wpack', 'dims', 'acts'):                                                 # null pointers
        assert _raw(capi, head, N_USERS, n, 4, ptr, rows, (o_i, o_s), null=(name,)) == EINVAL, name
    assert _raw(capi, head, N_USERS, n, 4, None, rows, (o_i, o_s)) == EINVAL                           # no cand_ptr with m > 0
    assert _raw(capi, head, N_USERS, n, 4, ptr, None, (o_i, o_s)) == EINVAL                            # cand_ptr without cand_items
    assert _raw(capi, head, N_USERS, n, 4, ptr, rows, (None, o_s)) == EINVAL and _raw(capi, head, N_USERS, n, 4, ptr, rows, (o_i, None)) == EINVAL
    assert _raw(capi, head, N_USERS, n, 4, ptr, rows, (o_i, o_s), m=N_USERS - 1) == EINVAL             # users == NULL needs m == n_users
    info = capi.RankRouteInfo()
    dims_c = (ctypes.c_int32 * len(head.dims))(*head.dims)
    assert lib.amar_rank_route(3, dims_c, len(head.dims) - 1, ctypes.byref(info)) == EINVAL            # kind 3 is still unknown
    assert lib.amar_rank_route(5, dims_c, len(head.dims) - 1, ctypes.byref(info)) == 0 and info.fits == 1
    with pytest.raises(capi.AmarError):
        capi.recommend_lists(*head.args(), 65, ptr.cpu().numpy(), [0, 1, 2])
    for bad_ptr, bad_rows in (([0, 3] + [3] * (N_USERS - 1), [2, 1, 0]), ([0, 2] + [2] * (N_USERS - 1), [1, 1]), ([0, 1] + [1] * (N_USERS - 1), [n]),
                              ([0, 1] + [1] * (N_USERS - 1), [-1]), ([0, 1], [0])):                    # checked before anything is uploaded
        with pytest.raises(ValueError, match='cand'):
            capi.recommend_lists(*head.args(), 4, bad_ptr, bad_rows)
    with pytest.raises(ValueError, match='excl'):
        capi.recommend_lists(*head.args(), 4, ptr, rows, excl_ptr=_dev(np.zeros(N_USERS + 1)))
    assert lib.amar_last_hip_error() == before == 0
    torch.cuda.synchronize()
    assert (o_i == 7).all() and (o_s == 7.0).all()                                                     # nothing was launched
    assert _raw(capi, head, 0, n, 4, None, None, (None, None)) == 0                                    # m == 0: OK with null outputs
    assert _raw(capi, head, N_USERS, n, 4, ptr, rows, (o_i, o_s)) == 0                                 # ... and the good call is served
    torch.cuda.synchronize()
    got = o_i[:N_USERS * 4].reshape(N_USERS, 4).cpu().numpy()
    assert sorted(got[0][got[0] >= 0].tolist()) == [0] and sorted(got[2][got[2] >= 0].tolist()) == [2] and (got[3:] == -1).all()
    assert (o_i[N_USERS * 4:] == 7).all()


# ---- 5. the models -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['BasicGCN', 'BasicRS', 'HybridCBRS'])
def test_models_against_their_own_full_ranking(hip, name, monkeypatch):
    """With <= 64 items a k = 64 call is every user's complete ranking; recommend_from must return it struck down to the user's own
    list and cut to k: items exactly, scores bit for bit.  The fused route is held to recommend(k=64), the pair-route models to
    their pair route's complete ranking."""
    import torch
    from deep_cbrs_amar_renaissance_amd import recommend as rec
    capi = hip
    model, train, g, route = _model_case(name)
    nu, ni = g['n_users'], g['n_items']
    assert ni <= 64 and model._group_route(train, kind='lists')[0] == route
    full = model.recommend(train, k=64) if route == 'fused' else model._recommend_pairs(train, k=64)
    open_full = model.recommend(train, k=64, exclude_seen=False) if route == 'fused' else model._recommend_pairs(train, k=64, exclude_seen=False)
    rng = np.random.default_rng(3)
    per = [nu + np.sort(rng.choice(ni, size=int(rng.integers(0, 40)), replace=False)) for _ in range(nu)]
    per[0], per[1], per[2] = per[0][:0], nu + np.arange(ni), per[2][:1]                               # empty, everything, one
    keep = [set(p.tolist()) for p in per]
    among_before = model.recommend_among(train, per, k=10)
    calls = {'fused': 0, 'pairs': 0, 'among': 0, 'plain': 0}
    count = lambda key, fn: (lambda *a, **kw: (calls.__setitem__(key, calls[key] + 1), fn(*a, **kw))[1])
    for key, attr in (('fused', 'recommend_lists'), ('pairs', 'topk_segmented'), ('among', 'recommend_among'), ('plain', 'recommend')):
        monkeypatch.setattr(capi, attr, count(key, getattr(capi, attr)))
    n_calls = 0
    for k in (1, 10, 64):
        got = model.recommend_from(train, per, k=k)
        n_calls += 1
        assert np.array_equal(got[0], np.arange(nu)) and got[1].dtype == np.int64 and got[2].dtype == np.float32 and got[1].shape == (nu, k)
        assert _same(got, *among_ref.filter_lists(full[1], full[2], keep, k)), (name, k)
    assert (got[1][0] == -1).all() and _same((None, got[1][1:2], got[2][1:2]), full[1][1:2], full[2][1:2])
    want = model.recommend_from(train, per, k=10)
    n_calls += 1
    # the [m, P] -1-padded array, on the host and on the device; shuffled and duplicated ids
    P = max(len(p) for p in per) + 3
    padded = np.full((nu, P), -1, dtype=np.int64)
    for u, p in enumerate(per):
        padded[u, :len(p)] = p
    shuffled = padded.copy()
    for u, p in enumerate(per):
        if len(p):
            shuffled[u, len(p):] = rng.choice(p, size=P - len(p))                                     # duplicates instead of padding
        shuffled[u] = shuffled[u][rng.permutation(P)]
    for form in (padded, padded.astype(np.int32), shuffled, torch.from_numpy(padded), torch.from_numpy(padded).cuda(),
                 torch.from_numpy(shuffled).cuda(), torch.from_numpy(shuffled.astype(np.int32)).cuda(), [p[::-1].tolist() + p[:2].tolist() for p in per]):
        assert _same(model.recommend_from(train, form, k=10), want[1], want[2])
        n_calls += 1
    assert calls == dict(among=0, plain=0, **({'fused': n_calls, 'pairs': 0} if route == 'fused' else {'fused': 0, 'pairs': n_calls})), calls
    # a subset of the users, in the caller's order, one of them twice with two lists
    users = [7, 3, 3, 39]
    lists = [per[7], per[3], per[5], per[39]]
    got = model.recommend_from(train, lists, k=10, users=users)
    assert np.array_equal(got[0], users) and _same(got, *among_ref.filter_lists(full[1][users], full[2][users], [set(c.tolist()) for c in lists], 10))
    # exclude_seen=False
    got = model.recommend_from(train, per, k=64, exclude_seen=False)
    assert _same(got, *among_ref.filter_lists(open_full[1], open_full[2], keep, 64)) and ((got[1] >= 0).sum(1) == [len(p) for p in per]).all()
    # device lists, and what recommend() hands out goes straight back in
    with rec.device_lists():
        u, rows, sc = model.recommend_from(train, per, k=10)
    assert rows.is_cuda and rows.dtype == torch.int32 and np.array_equal(np.where(rows.cpu().numpy() >= 0, rows.cpu().numpy() + nu, -1), want[1])
    top = model.recommend(train, k=20)
    again = model.recommend_from(train, top[1], k=5)
    if route == 'fused':
        assert _same(again, top[1][:, :5], top[2][:, :5])
    for bad in (dict(candidates=[[nu - 1]] * nu), dict(candidates=per, k=65), dict(candidates=[per[0]], users=[nu]), dict(candidates=per[:-1]),
                dict(candidates=per[0]), dict(candidates=torch.zeros((nu, 3), device='cuda'))):
        with pytest.raises(ValueError):
            model.recommend_from(train, **bad)
    # no side effects: recommend() and per-user recommend_among() return the bits they returned before
    after = model.recommend(train, k=64) if route == 'fused' else model._recommend_pairs(train, k=64)
    assert np.array_equal(full[1], after[1]) and np.array_equal(_bits(full[2]), _bits(after[2]))
    among_after = model.recommend_among(train, per, k=10)
    assert _same(among_after, among_before[1], among_before[2])


# ---- 6. evaluate_ranking_sampled ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['BasicGCN', 'BasicRS'])
def test_evaluate_ranking_sampled(hip, name):
    from deep_cbrs_amar_renaissance_amd.utilities.metrics import full_ranking_metrics, sampled_negatives
    from tests.test_validation_gpu import _held_out
    model, train, g, route = _model_case(name)
    nu, ni = g['n_users'], g['n_items']
    test = _held_out(g, np.random.default_rng(3), n=300)
    liked = test.copy()
    liked[:, 2] = 1
    ks = [1, 5, 10]
    keys = ['{}_at_{}'.format(q, k) for q in ('precision', 'recall', 'ndcg', 'hit') for k in ks]
    for users in (None, np.array([5, 3, 3, 17, 0, 39])):
        got = model.evaluate_ranking_sampled(train, test, ks, n_negatives=9, seed=2, users=users)
        drawn_users, drawn = sampled_negatives(train, test, 9, 2)
        listed = np.arange(nu) if users is None else users
        lists = [drawn[drawn_users == u][0] if u in drawn_users else np.zeros(0, dtype=np.int64) for u in listed]
        ru, ri, _ = model.recommend_from(train, [c[c >= 0] for c in lists], k=10, users=users)
        want = full_ranking_metrics(ru, ri, test, ks)
        assert set(got) == set(want) == set(model.evaluate_ranking(train, test, ks, users=users))
        assert (got['users_evaluated'], got['users_skipped']) == (want['users_evaluated'], want['users_skipped']) and want['users_evaluated'] > 0
        for key in keys:
            print('{:<16s} sampled {:.15f}  host {:.15f}'.format(key, got[key], want[key]))
            assert abs(got[key] - want[key]) <= 1e-12, (key, got[key], want[key])
        assert got == model.evaluate_ranking_sampled(train, test, ks, n_negatives=9, seed=2, users=users)      # the same bits again
        if users is None:
            assert 0.0 < got['hit_at_10'] and got['ndcg_at_10'] < 1.0
        # every free item drawn: the full ranking's evaluation.  The protocol never draws an item the user rated in test, so the
        # lists are the whole unseen catalogue only where every held-out pair is a positive: the same pairs, all with label 1
        everything = model.evaluate_ranking_sampled(train, liked, ks, n_negatives=ni, seed=5, users=users)
        plain = model.evaluate_ranking(train, liked, ks, users=users)
        assert plain['users_evaluated'] > 0 and plain['hit_at_10'] > 0.0
        if route == 'fused':
            assert everything == plain
        else:
            assert all(abs(everything[key] - plain[key]) <= 1e-12 for key in keys) and everything['users_evaluated'] == plain['users_evaluated']
    with pytest.raises(ValueError):
        model.evaluate_ranking_sampled(train, test, [])
    with pytest.raises(ValueError):
        model.evaluate_ranking_sampled(train, test, [65])
