"""amar_rowwise_xw_route and amar_sage_tail_route on the host (no GPU): which of its four kernels the row-wise X.W prologue takes for a
call, and how the capped grids of the prologue and of the GraphSAGE tail walk the rows.  The addresses are made up: the functions look at
alignment and NULL only, nothing is dereferenced.  The launchers call the same functions, so these are the launchers' rules; their
refusals are checked on the launchers themselves too, on arguments they refuse before they touch the device.  And the references and
the case table of tests/xw_ref.py: every case of the GPU file takes the route it names."""
import ctypes

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from tests import xw_ref as ref

BASE = 0x7F0000100000                                                  # 16-byte aligned, never dereferenced
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
CAP = 8192


def xroute(n_rows=1000, F=8, C=8, ldx=None, ldh=None, copy=False, ld_copy=None, x_off=0, w_off=0, h_off=0, copy_off=0, attn=False,
           ids=False, code=False, null=()):
    """The route of a prologue call at made-up addresses (X, W, H, copy_to 16-byte aligned plus the byte offsets given); ldx = F,
    ldh = C, ld_copy = F unless given."""
    addr = {name: BASE + 0x10000000 * i for i, name in enumerate(('X', 'W', 'H', 'copy'))}
    p = {'X': addr['X'] + x_off, 'W': addr['W'] + w_off, 'H': addr['H'] + h_off, 'copy': addr['copy'] + copy_off if copy else None}
    for name in null:
        p[name] = None
    info = capi.XwRouteInfo()
    rc = capi.load().amar_rowwise_xw_route(p['X'], F if ldx is None else ldx, F, p['W'], C, p['H'], C if ldh is None else ldh, p['copy'],
                                           (F if ld_copy is None else ld_copy) if copy else 0, int(attn), int(ids), n_rows, ctypes.byref(info))
    if code:
        return rc
    assert rc == OK, rc
    return info.as_dict()


def kernel_of(**kw):
    return xroute(**kw)['kernel']


def test_the_pieces_form_and_every_condition_that_leaves_it(monkeypatch):
    monkeypatch.delenv('AMAR_XW_FORM', raising=False)
    assert xroute() == dict(kernel='pieces8', cp=8, rows_per_block=512, blocks=2, trips=1)
    assert kernel_of(copy=True) == 'pieces8' and kernel_of(ldx=24, ldh=12, copy=True, ld_copy=40) == 'pieces8'
    # what keeps the alignment but not the pieces: the one-thread-per-row kernel
    assert kernel_of(attn=True) == 'vec8' and kernel_of(ids=True) == 'vec8' and kernel_of(attn=True, ids=True) == 'vec8'
    for off in (4, 8, 12):
        assert kernel_of(w_off=off) == 'vec8'
    # what breaks the float4 accesses of both: the generic kernel
    for off in (4, 8, 12):
        assert kernel_of(x_off=off) == 'generic' and kernel_of(h_off=off) == 'generic' and kernel_of(copy=True, copy_off=off) == 'generic'
        assert kernel_of(copy_off=off) == 'pieces8'                     # (no copy_to: its address is not looked at)
    for r in (1, 2, 3):
        assert kernel_of(ldx=16 + r) == 'generic' and kernel_of(ldh=16 + r) == 'generic' and kernel_of(copy=True, ld_copy=16 + r) == 'generic'
        assert kernel_of(attn=True, ldh=8 + r) == 'generic' and kernel_of(ids=True, ldx=8 + r) == 'generic'
    # shapes
    assert xroute(F=8, C=16) == dict(kernel='generic', cp=16, rows_per_block=16, blocks=63, trips=1)
    assert kernel_of(F=16, C=8) == 'generic' and kernel_of(F=12, C=12) == 'generic' and kernel_of(F=4, C=4) == 'generic'
    assert kernel_of(F=32, C=32) == 'generic' and kernel_of(F=64, C=64) == 'generic'
    # the 16-wide kernel: the same alignment rules, W's address is not among them
    assert xroute(F=16, C=16) == dict(kernel='vec16', cp=16, rows_per_block=256, blocks=4, trips=1)
    assert kernel_of(F=16, C=16, attn=True, ids=True, copy=True, w_off=4) == 'vec16'
    assert kernel_of(F=16, C=16, x_off=4) == 'generic' and kernel_of(F=16, C=16, ldh=18) == 'generic'
    assert kernel_of(F=16, C=16, copy=True, ld_copy=17) == 'generic' and kernel_of(F=16, C=16, copy=True, copy_off=8) == 'generic'


def test_the_env_switch_is_read_at_every_call(monkeypatch):
    monkeypatch.setenv('AMAR_XW_FORM', 'rows')
    assert xroute() == dict(kernel='vec8', cp=8, rows_per_block=512, blocks=2, trips=1)
    assert kernel_of(F=16, C=16) == 'vec16' and kernel_of(x_off=4) == 'generic'
    monkeypatch.setenv('AMAR_XW_FORM', 'pieces')                        # any other value: not the switch
    assert kernel_of() == 'pieces8'
    monkeypatch.delenv('AMAR_XW_FORM')
    assert kernel_of() == 'pieces8'


KERNEL_SHAPES = [('pieces8', dict(), 512), ('vec8', dict(attn=True), 512), ('vec16', dict(F=16, C=16), 256),
                 ('generic', dict(F=4, C=64), 4), ('generic', dict(F=4, C=24), 8), ('generic', dict(F=8, C=8, ldh=9), 32),
                 ('generic', dict(F=5, C=3), 64), ('generic', dict(F=2, C=1), 256)]


@pytest.mark.parametrize('kernel,kw,rpb', KERNEL_SHAPES)
def test_grid_and_trips(monkeypatch, kernel, kw, rpb):
    monkeypatch.delenv('AMAR_XW_FORM', raising=False)
    C = kw.get('C', 8)
    cp = 256 // ref.rows_per_block('generic', C)
    assert cp >= C and cp < 2 * C and cp & (cp - 1) == 0
    assert xroute(n_rows=0, **kw) == dict(kernel=kernel, cp=cp, rows_per_block=rpb, blocks=0, trips=0)
    assert xroute(n_rows=1, **kw) == dict(kernel=kernel, cp=cp, rows_per_block=rpb, blocks=1, trips=1)
    assert xroute(n_rows=rpb, **kw)['blocks'] == 1 and xroute(n_rows=rpb + 1, **kw)['blocks'] == 2
    per_trip = CAP * rpb
    assert per_trip == ref.trip_rows(kernel, C)
    for n, blocks, trips in ((per_trip - rpb, CAP - 1, 1), (per_trip - rpb + 1, CAP, 1), (per_trip - 1, CAP, 1), (per_trip, CAP, 1),
                             (per_trip + 1, CAP, 2), (2 * per_trip, CAP, 2), (2 * per_trip + 1, CAP, 3)):
        r = xroute(n_rows=n, **kw)
        assert r == dict(kernel=kernel, cp=cp, rows_per_block=rpb, blocks=blocks, trips=trips), n
        assert r == ref.expected_route(kernel, C, n)
    top = xroute(n_rows=2 ** 31 - 1, **kw)
    assert top['blocks'] == CAP and top['trips'] == -(-(2 ** 31 - 1) // per_trip)


def test_trip_thresholds_in_rows():
    assert ref.trip_rows('pieces8', 8) == ref.trip_rows('vec8', 8) == 4194304 and ref.trip_rows('vec16', 16) == 2097152
    assert ref.trip_rows('generic', 64) == 32768 and ref.trip_rows('generic', 24) == 65536 and ref.trip_rows('generic', 16) == 131072


def test_heads_entry_lands_where_the_flat_product_does(monkeypatch):
    """amar_rowwise_xw_heads_f32 runs the product with C = heads * C, no attention operands, H dense or a slice with ldh % 4 == 0."""
    monkeypatch.delenv('AMAR_XW_FORM', raising=False)
    for heads, C, F, want in ((2, 4, 8, 'pieces8'), (1, 8, 8, 'pieces8'), (2, 8, 16, 'vec16'), (4, 4, 16, 'vec16'), (1, 16, 16, 'vec16'),
                              (4, 4, 4, 'generic'), (2, 4, 16, 'generic'), (4, 4, 8, 'generic'), (3, 4, 12, 'generic'), (4, 16, 64, 'generic'),
                              (2, 16, 32, 'generic'), (1, 4, 4, 'generic')):
        assert capi.gat_heads_supported(heads, C)
        assert kernel_of(F=F, C=heads * C) == want, (heads, C, F)
    monkeypatch.setenv('AMAR_XW_FORM', 'rows')
    assert kernel_of(F=8, C=2 * 4) == 'vec8'
    monkeypatch.delenv('AMAR_XW_FORM')
    assert kernel_of(F=8, C=8, x_off=4) == 'generic' and kernel_of(F=8, C=8, ldx=9) == 'generic'        # X of the heads call may be anything
    r = xroute(n_rows=524291, F=4, C=16)
    assert (r['kernel'], r['rows_per_block'], r['trips']) == ('generic', 16, 5)
    assert -(-524291 * 4 // (CAP * 256)) == 2                           # the scalars kernel: one thread per (row, head), the same cap


def test_refusals_of_the_query_in_the_launchers_order():
    info = capi.XwRouteInfo()
    assert capi.load().amar_rowwise_xw_route(BASE, 8, 8, BASE, 8, BASE, 8, None, 0, 0, 0, 10, None) == EINVAL
    assert xroute(n_rows=-1, code=True) == EINVAL
    for name in ('X', 'W', 'H'):
        assert xroute(null=(name,), code=True) == EINVAL
    assert xroute(F=0, code=True) == EINVAL and xroute(C=0, code=True) == EINVAL
    assert xroute(ldx=7, code=True) == EINVAL and xroute(ldh=7, code=True) == EINVAL
    assert xroute(F=65, C=8, code=True) == EUNSUPPORTED and xroute(F=8, C=65, code=True) == EUNSUPPORTED
    assert xroute(F=64, C=64, code=True) == OK
    assert xroute(copy=True, ld_copy=7, code=True) == EINVAL
    # order: a null pointer or a short leading dimension before the width, the width before the copy's leading dimension
    assert xroute(F=65, ldx=8, code=True) == EINVAL and xroute(F=65, null=('X',), code=True) == EINVAL
    assert xroute(F=65, ldx=65, copy=True, ld_copy=7, code=True) == EUNSUPPORTED
    assert xroute(n_rows=0, copy=True, ld_copy=7, code=True) == EINVAL  # an empty call is still checked
    # a refused call leaves no stale plan behind
    assert capi.load().amar_rowwise_xw_route(BASE, 8, 65, BASE, 8, BASE, 8, None, 0, 0, 0, 10, ctypes.byref(info)) == EINVAL
    assert info.as_dict() == dict(kernel='generic', cp=0, rows_per_block=0, blocks=0, trips=0)


def xw_code(n_rows=10, F=8, C=8, ldx=8, ldh=8, X=BASE, W=BASE, H=BASE, copy=None, ld_copy=0, attn=(None, None, None, None), scale=None):
    return capi.load().amar_rowwise_xw_f32(X, ldx, F, W, C, H, ldh, copy, ld_copy, *attn, scale, n_rows, None)


def test_launcher_refusals_are_unchanged():
    """rowwise_xw_run's refusals, codes and order, on calls it turns down before any device call."""
    a = BASE
    assert xw_code(n_rows=-1) == EINVAL and xw_code(X=None) == EINVAL and xw_code(W=None) == EINVAL and xw_code(H=None) == EINVAL
    assert xw_code(F=0) == EINVAL and xw_code(C=0) == EINVAL and xw_code(ldx=7) == EINVAL and xw_code(ldh=7) == EINVAL
    assert xw_code(F=65, ldx=65) == EUNSUPPORTED and xw_code(C=65, ldh=65) == EUNSUPPORTED
    assert xw_code(F=65, ldx=8) == EINVAL and xw_code(F=65, ldx=65, copy=a, ld_copy=7) == EUNSUPPORTED
    assert xw_code(copy=a, ld_copy=7) == EINVAL
    for partial in ((a, None, None, None), (a, a, None, None), (a, a, a, None), (None, None, None, a), (None, a, a, a)):
        assert xw_code(attn=partial) == EINVAL
    assert xw_code(copy=a, ld_copy=7, attn=(a, None, None, None)) == EINVAL
    assert xw_code(F=65, ldx=65, attn=(a, None, None, None)) == EUNSUPPORTED      # the width before the attention operands
    assert xw_code(n_rows=0) == OK and xw_code(n_rows=0, attn=(a, a, a, a), scale=a) == OK   # empty: before the scale refusal
    assert xw_code(n_rows=0, attn=(a, None, None, None)) == EINVAL                # ... and after the attention operands
    assert xw_code(attn=(a, a, a, a), scale=a) == EINVAL
    lib = capi.load()
    assert lib.amar_rowwise_xw_gather_f32(a, 8, 8, None, a, 8, a, 8, None, 10, None) == EINVAL
    assert lib.amar_rowwise_xw_gather_f32(a, 8, 8, a, a, 8, a, 7, None, 10, None) == EINVAL
    assert lib.amar_rowwise_xw_gather_f32(a, 8, 8, a, a, 65, a, 65, None, 10, None) == EUNSUPPORTED
    assert lib.amar_rowwise_xw_gather_f32(a, 8, 8, a, a, 8, a, 8, None, 0, None) == OK
    # the heads entry: its own checks, then the product's
    heads = lib.amar_rowwise_xw_heads_f32
    assert heads(a, 8, 8, a, 2, 4, a, 8, a, a, a, 0, None) == OK
    assert heads(a, 8, 8, a, 2, 4, a, 8, a, a, None, 10, None) == EINVAL and heads(a, 7, 8, a, 2, 4, a, 8, a, a, a, 10, None) == EINVAL
    assert heads(a, 8, 8, a, 2, 6, a, 12, a, a, a, 10, None) == EUNSUPPORTED and heads(a, 8, 8, a, 5, 16, a, 80, a, a, a, 10, None) == EUNSUPPORTED
    assert heads(a, 65, 65, a, 2, 4, a, 8, a, a, a, 10, None) == EUNSUPPORTED
    assert heads(a, 8, 8, a, 2, 4, a, 9, a, a, a, 10, None) == EINVAL and heads(a, 8, 8, a, 2, 4, a + 4, 8, a, a, a, 10, None) == EINVAL


# ---- the GraphSAGE tail -----------------------------------------------------------------------------------------------------------------
def test_sage_tail_route():
    for C, cp in ((4, 4), (8, 8), (12, 16), (16, 16), (20, 32), (32, 32), (36, 64), (48, 64), (64, 64)):
        for F in (4, 24, 64):
            assert capi.sage_tail_route(F, C, 777) == dict(cp=cp, blocks=4, trips=1)
    assert capi.sage_tail_route(4, 4, 0) == dict(cp=4, blocks=0, trips=0) and capi.sage_tail_route(4, 4, 1) == dict(cp=4, blocks=1, trips=1)
    assert capi.sage_tail_route(4, 4, 256)['blocks'] == 1 and capi.sage_tail_route(4, 4, 257)['blocks'] == 2
    per_trip = CAP * 256
    assert per_trip == 2097152
    for n, blocks, trips in ((per_trip - 256, CAP - 1, 1), (per_trip - 1, CAP, 1), (per_trip, CAP, 1), (per_trip + 1, CAP, 2),
                             (per_trip + 300, CAP, 2), (2 * per_trip, CAP, 2), (2 * per_trip + 1, CAP, 3), (2 ** 40, CAP, 2 ** 19)):
        assert capi.sage_tail_route(8, 12, n) == dict(cp=16, blocks=blocks, trips=trips), n


def tail_code(F=8, C=8, n_rows=10, ldx=8, lda=8, ldy=8, X=BASE, AGG=BASE, Y=BASE, W=BASE, bias=BASE):
    return capi.load().amar_sage_tail_f32(X, ldx, AGG, lda, F, W, bias, C, Y, ldy, n_rows, None)


def test_sage_tail_refusals_are_unchanged():
    lib, info = capi.load(), capi.SageTailRouteInfo()
    q = lambda F, C, n: lib.amar_sage_tail_route(F, C, n, ctypes.byref(info))
    assert lib.amar_sage_tail_route(8, 8, 10, None) == EINVAL
    for F, C, n, want in ((8, 8, -1, EINVAL), (0, 8, 10, EINVAL), (8, 0, 10, EINVAL), (6, 8, 10, EINVAL), (8, 10, 10, EINVAL), (3, 8, 10, EINVAL),
                          (68, 68, 10, EUNSUPPORTED), (68, 8, 10, EUNSUPPORTED), (8, 68, 10, EUNSUPPORTED), (66, 8, 10, EINVAL),
                          (64, 64, 10, OK), (4, 4, 0, OK)):
        assert q(F, C, n) == want, (F, C, n)
        if want == OK and n > 0:
            continue                                                    # a well-formed call: it would launch
        assert tail_code(F=F, C=C, n_rows=n, ldx=max(F, 4) + (-F) % 4, lda=max(F, 4) + (-F) % 4, ldy=max(C, 4) + (-C) % 4) == want, (F, C, n)
    with pytest.raises(ValueError):
        capi.sage_tail_route(6, 8, 10)
    with pytest.raises(capi.AmarError):
        capi.sage_tail_route(8, 68, 10)
    # the launcher looks at its operands between the two shape checks
    a = BASE
    for kw in (dict(X=None), dict(AGG=None), dict(W=None), dict(bias=None), dict(Y=None), dict(ldx=4), dict(lda=9), dict(ldy=10),
               dict(X=a + 4), dict(AGG=a + 8), dict(Y=a + 4)):
        assert tail_code(**kw) == EINVAL, kw
    assert tail_code(F=68, ldx=68, lda=68, X=a + 4) == EINVAL and tail_code(F=68, ldx=68, lda=68) == EUNSUPPORTED
    assert tail_code(n_rows=0) == OK


# ---- the references and the case table --------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_every_case_names_its_route(monkeypatch):
    cases = ref.FORM_CASES + ref.FALLBACK_CASES + ref.TRIP_CASES
    assert len({c['id'] for c in cases}) == len(cases)
    for c in cases:
        if c['env']:
            monkeypatch.setenv('AMAR_XW_FORM', 'rows')
        else:
            monkeypatch.delenv('AMAR_XW_FORM', raising=False)
        F, C = c['F'], c['C']
        kw = dict(F=F, C=C, ldx=c['ldx'] or F + 8, ldh=c['ldh'] or C + 8, copy=c['copy'], ld_copy=c['ld_copy'] or F + 8,
                  x_off=4 * c['x_off'], w_off=4 * c['w_off'], h_off=4 * c['h_off'], copy_off=4 * c['copy_off'], attn=c['attn'], ids=c['ids'])
        for n in ((c['n'],) if 'n' in c else ref.SMALL_N):
            r = xroute(n_rows=n, **kw)
            assert r == ref.expected_route(c['kernel'], C, n), c['id']
            if 'trips' in c:
                assert r['trips'] == c['trips'] >= 2 and n % (r['blocks'] * r['rows_per_block']) != 0, c['id']      # a ragged last trip
    assert {c['kernel'] for c in ref.FORM_CASES} == {c['kernel'] for c in ref.TRIP_CASES} == set(capi.XW_KERNELS)
    for F, routes in ref.SAME_BITS.items():
        for kernel, kw in routes:
            monkeypatch.setenv('AMAR_XW_FORM', 'rows') if kw.get('env') else monkeypatch.delenv('AMAR_XW_FORM', raising=False)
            assert kernel_of(F=F, C=F, ldh=kw.get('ldh')) == kernel
    assert capi.sage_tail_route(ref.SAGE_TAIL_TRIP['F'], ref.SAGE_TAIL_TRIP['C'], ref.SAGE_TAIL_TRIP['M'])['trips'] == 2
    assert sorted({capi.sage_tail_route(4, C, 777)['cp'] for C in ref.SAGE_TAIL_C}) == [4, 8, 16, 32, 64]


def test_ids_of_the_cases_hold_what_the_kernels_branch_on():
    for n in ref.SMALL_N:
        ids = ref.make_ids(n, 50, seed=n)
        assert ids.dtype == np.int32 and len(ids) == n and ids[0] < 0 and ids.max() < 50
        if n > 4:
            assert (ids == 0).any() and (ids < 0).sum() >= 2 and len(np.unique(ids[ids >= 0])) < (ids >= 0).sum()
    edge = ref.trip_rows('vec8', 8)
    ids = ref.make_ids(edge + 257, 1000, seed=1, edges=(edge,))
    assert ids[edge - 1] < 0 and ids[edge] < 0 and ids[0] < 0 and ids[-1] == 0
    assert ref.boundary_rows(edge + 257, edge) == [edge - 1, edge, edge + 256]
    assert ref.boundary_rows(65537, 32768) == [32767, 32768, 65535, 65536]
    assert ref.boundary_rows(5, 32768) == [4]


def test_references_against_plain_float32():
    """numpy's float32 evaluation in the kernels' order (without fused multiply-add: two roundings a term where the kernels make one)
    satisfies twice the bound, and the float64 references agree with their definitions element by element."""
    for F, C in ((8, 8), (16, 16), (7, 12), (64, 64), (5, 3)):
        d = ref.draw('cpu-{}-{}'.format(F, C), 300, F, C)
        x, w, sc = d['x'], d['w'], d['scale']
        want, bound = ref.product(x, w), ref.product_bound(x, w)
        assert want.shape == (300, C) and np.allclose(want[5], x[5].astype(np.float64) @ w.astype(np.float64), rtol=1e-14)
        assert ref.within(ref.product_f32(x, w), want, 2 * bound) and ref.worst(ref.product_f32(x, w), want, bound) > 0
        assert not ref.within(ref.product_f32(x, w) * np.float32(1 + 2.0 ** -16), want, 2 * bound)        # the bound is tight enough to see 2^-16
        ids = ref.make_ids(300, 300, seed=F)
        hi = ref.product(x, w, row_ids=ids, row_scale=sc)
        assert np.all(hi[ids < 0] == 0) and np.allclose(hi[ids >= 0], (want[ids[ids >= 0]].T * sc[ids >= 0].astype(np.float64)).T, rtol=1e-14)
        assert np.all(ref.product_bound(x, w, ids, sc)[ids < 0] == 0)
        with pytest.raises(ValueError):
            ref.product(x, w, row_ids=ids, copy_to=True)
        h, cp = ref.product(x, w, copy_to=True)
        assert np.array_equal(cp, x) and np.array_equal(h, want)
        ss, sn = ref.scalars(x, w, d['a_self'], d['a_neigh'])
        assert np.allclose(ss, want @ d['a_self'].astype(np.float64), rtol=1e-14) and ss.shape == (300,)
        s32 = (ref.product_f32(x, w) * d['a_self'][None, :]).astype(np.float32)
        acc = np.zeros(300, dtype=np.float32)
        for c in range(C):
            acc = (acc + s32[:, c]).astype(np.float32)
        assert ref.within(acc, ss, 2 * ref.scalars_bound(x, w, d['a_self']))


def test_heads_reference_layout():
    rng = np.random.default_rng(3)
    F, H, C, n = 4, 4, 4, 37
    x, w3 = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((F, H, C)).astype(np.float32)
    a_s, a_n = rng.standard_normal((C, H)).astype(np.float32), rng.standard_normal((C, H)).astype(np.float32)
    hd, S = ref.heads(x, w3, a_s, a_n)
    bound = ref.heads_bound(x, w3, a_s, a_n)
    assert hd.shape == (n, H * C) and S.shape == bound.shape == (n, 2 * H) and (bound > 0).all()
    for h in range(H):
        hh = x.astype(np.float64) @ w3[:, h, :].astype(np.float64)
        assert np.allclose(hd[:, h * C:(h + 1) * C], hh, rtol=1e-14)
        assert np.allclose(S[:, h], hh @ a_s[:, h].astype(np.float64), rtol=1e-13) and np.allclose(S[:, H + h], hh @ a_n[:, h].astype(np.float64), rtol=1e-13)
        assert np.allclose(bound[:, h], ref.scalars_bound(x, w3[:, h, :], a_s[:, h]), rtol=1e-13)   # one head: the one-head bound


def test_sage_tail_reference():
    rng = np.random.default_rng(5)
    F, C, n = 8, 12, 50
    x, g = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((n, F)).astype(np.float32)
    w, b = rng.uniform(-0.5, 0.5, (2 * F, C)).astype(np.float32), rng.uniform(-0.1, 0.1, C).astype(np.float32)
    x[7], g[7] = 0, 0
    y = ref.sage_tail(x, g, w, b)
    z7 = b.astype(np.float64)
    assert np.allclose(y[7], np.maximum(z7 / np.linalg.norm(z7), 0), rtol=1e-14)
    assert np.allclose((y ** 2).sum(1) <= 1 + 1e-12, True) and (y >= 0).all()
    zero = ref.sage_tail(np.zeros((2, F), np.float32), np.zeros((2, F), np.float32), w, np.zeros(C, np.float32))
    assert np.all(zero == 0)                                            # the clamp: 0 / sqrt(1e-12), not 0 / 0
    z = np.concatenate([x, g], 1).astype(np.float32) @ w + b            # float32 evaluation: inside the tolerance of the GPU test
    y32 = np.maximum(z / np.sqrt(np.maximum((z * z).sum(1, keepdims=True), np.float32(1e-12))), 0)
    assert ref.rel_err(y32, y) < ref.SAGE_TAIL_TOL
