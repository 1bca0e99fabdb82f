"""Every kernel form of amar_dense_bwd_f32 against float64 (tests/dense_bwd_ref.py), at the smallest shapes that select it (pytest -m gpu).

Each case first ASKS the launcher's own route function (capi.dense_bwd_route) which kernel its operands select and asserts the form it
claims to test.  Operands are column slices of wider, taller buffers whose slack is NaN: a read outside the operand that is used
shows up in the result, a store outside the output shows up in the slack.

Bounds (dense_bwd_ref.dx_bound / dz_bound; U = 2^-24):
  dX   per element  |got - want| <= (N + 2) U (|dZ| . |W|^T)   — a float32 sum of N <= 128 products, any order
  dZ   per element  exact for None and relu; 4 U |want| for sigmoid' (three roundings)
  dW, db            helpers.rel_err < 3e-6 against float64 (the suite's bound for these sums over M rows)
Every row-walking or 16-byte-load case runs a second time on a deliberately misaligned copy of the same data — the scalar tile kernel,
a second implementation — and the two must agree within twice those bounds.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dense_bwd_ref as ref
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 3                                                                # rows past M in every buffer
TOL = 3e-6                                                             # dW / db against float64


@functools.lru_cache(maxsize=4)
def host_case(M, K, N, act):
    """Float32 operands (read-only) and their float64 reverse pass, computed once per shape."""
    rng = np.random.default_rng(1000003 * K + 1009 * N + M)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    z = x.astype(np.float64) @ w + rng.standard_normal(N) * 0.1
    y = (np.maximum(z, 0) if act == 'relu' else 1 / (1 + np.exp(-z))).astype(np.float32)
    if act == 'relu':                                                  # exact zeros (about half of them already), and a negative zero
        y.flat[0], y.flat[-1] = -0.0, 0.0
        assert np.signbit(y.flat[0]) and (y == 0).sum() >= 2
        if M * N > 2:
            y.flat[1] = 0.75
    elif act == 'sigmoid':                                             # a saturated 1 and 0: sigmoid' is exactly 0 at both
        y.flat[0], y.flat[-1] = 1.0, 0.0
    init = rng.standard_normal((M, K)).astype(np.float32)              # what dX holds before an accumulating call
    for a in (x, w, dy, y, init):
        a.setflags(write=False)
    return dict(x=x, w=w, dy=dy, y=y if act is not None else None, init=init, want=ref.dense_bwd(x, y, dy, w, act))


def _host(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, copy=True))  # (the cached operands are read-only)


def _slice(data, misaligned, fill=float('nan')):
    """(buffer, view): `data` [M, C] as a column slice of a wider, taller buffer of `fill`.  Aligned: offset 4 floats, a leading dimension
    that is a multiple of 4; misaligned: offset 2 floats (8 bytes off a 16-byte boundary) and an odd leading dimension."""
    M, C = data.shape
    off = 2 if misaligned else 4
    width = (off + C + 3) | 1 if misaligned else (C + 3) // 4 * 4 + 8
    buf = torch.full((M + PAD, width), fill, dtype=torch.float32, device=DEV)
    view = buf[:M, off:off + C]
    view.copy_(_host(data))
    assert (view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0) != misaligned
    return buf, view


def _slack_untouched(buf, view, fill):
    """Everything of `buf` outside `view` still holds `fill` (NaN compares by isnan)."""
    M, C = view.shape
    off = view.storage_offset() - buf.storage_offset()
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:M, off:off + C] = False
    rest = buf[mask]
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


class Operands:
    """The device operands of one case.  x_form: 'slice' (like the rest), 'unaligned' (X alone 4 bytes off, the rest aligned),
    'column' (X one contiguous column, ldx = 1: a GAT layer's ds.view(n, 1))."""

    def __init__(self, case, K, N, misaligned, x_form='slice'):
        self.misaligned = misaligned
        x, w = case['x'], case['w']
        if x_form == 'column':
            assert K == 1
            self.x_buf = torch.full((x.shape[0] + PAD,), float('nan'), dtype=torch.float32, device=DEV)
            self.x_buf[:x.shape[0]] = _host(x[:, 0])
            self.X = self.x_buf[:x.shape[0]].view(-1, 1)
        elif x_form == 'unaligned' and not misaligned:
            self.x_buf = torch.full((x.shape[0] + PAD, K + 8), float('nan'), dtype=torch.float32, device=DEV)
            self.X = self.x_buf[:x.shape[0], 1:1 + K]
            self.X.copy_(_host(x))
        else:
            self.x_buf, self.X = _slice(x, misaligned)
        self.dy_buf, self.dY = _slice(case['dy'], misaligned)
        self.Y = _slice(case['y'], misaligned)[1] if case['y'] is not None else None
        flat = torch.zeros(K * N + 4, dtype=torch.float32, device=DEV)  # W is contiguous [K, N]: misaligned = 8 bytes into a buffer
        self.W = flat[2:2 + K * N].view(K, N) if misaligned else flat[:K * N].view(K, N)
        self.W.copy_(_host(w))


def call(hip, case, ops, act, ws, outputs, accumulate=False, defer=False, use_x=True, use_w=True, route_only=False):
    """One dense_bwd call into fresh output buffers (dX / dZ slices of NaN-filled — or, accumulating, 7.5-and-init-filled — buffers)."""
    M, N = ops.dY.shape
    K = case['x'].shape[1]
    out = {}
    if 'dX' in outputs:
        fill = 7.5 if accumulate else float('nan')
        out['dX_buf'], out['dX'] = _slice(case['init'] if accumulate else np.full((M, K), np.nan, np.float32), ops.misaligned, fill)
        out['dX_fill'] = fill
    if 'dZ' in outputs:
        out['dZ_buf'], out['dZ'] = _slice(np.full((M, N), np.nan, np.float32), ops.misaligned)
    if 'dW' in outputs:
        out['dW'] = torch.full((K, N), float('nan'), device=DEV)
    if 'db' in outputs:
        out['db'] = torch.full((N,), float('nan'), device=DEV)
    args = (ops.X if use_x else None, ops.Y if act is not None else None, ops.dY, ops.W if use_w else None, act, ws)
    kwargs = dict(dX=out.get('dX'), dW=out.get('dW'), db=out.get('db'), dZ=out.get('dZ'), accumulate_dx=accumulate, defer=defer,
                  K=None if (use_x or use_w) else K)
    if route_only:
        return hip.dense_bwd_route(*args, **kwargs)
    out['lazy'] = hip.dense_bwd(*args, **kwargs)
    return out


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _within(name, got, want, bound):
    """Per element |got - want| <= bound (a NaN anywhere fails); prints the worst ratio first."""
    err = np.abs(got - want)
    exact = bound == 0
    worst = float(np.max(np.where(exact, np.where(err == 0, 0.0, np.inf), err / np.where(exact, 1.0, bound)))) if err.size else 0.0
    print('{}: worst |got - want| / bound = {:.3f} (max |want| {:.3e})'.format(name, worst, float(np.abs(want).max())))
    assert not np.isnan(got).any(), name + ': NaN (a read outside the operand?)'
    assert np.all(err <= bound), '{}: {} elements beyond the bound, worst ratio {}'.format(name, int((err > bound).sum()), worst)


def verify(name, out, case, K, N, act, accumulate):
    """One call's outputs against float64, and its slack."""
    want = case['want']
    if 'dX' in out:
        init = case['init'].astype(np.float64) if accumulate else 0.0
        _within(name + ' dX', _np(out['dX']), want['dx'] + init, ref.dx_bound(N, want['dx_mag'], np.abs(init)))
        assert _slack_untouched(out['dX_buf'], out['dX'], out['dX_fill']), name + ': a store outside dX'
    if 'dZ' in out:
        _within(name + ' dZ', _np(out['dZ']), want['dz'], ref.dz_bound(want['dz'], act))
        assert _slack_untouched(out['dZ_buf'], out['dZ'], float('nan')), name + ': a store outside dZ'
    if 'dW' in out:
        e = helpers.rel_err(_np(out['dW']), want['dw'][:K])
        print('{} dW: rel_err {:.3e}'.format(name, e))
        assert e < TOL
    if 'db' in out:
        e = helpers.rel_err(_np(out['db']), want['db'])
        print('{} db: rel_err {:.3e}'.format(name, e))
        assert e < TOL


def same_bits(a, b, keys=('dX', 'dZ', 'dW', 'db')):
    return all(torch.equal(a[k], b[k]) for k in keys if k in a)


def check_case(hip, M, K, N, act, expect, outputs=('dX', 'dW', 'db', 'dZ'), x_form='slice', accumulate=False, use_x=True, use_w=True,
               aligned=True):
    """The whole protocol for one case: route asserted, float64 per element, slack, called twice with identical bits, deferred partials
    materialised bit for bit, and (for a row-walking or 16-byte-load route) agreement with the scalar tile kernel on a misaligned copy."""
    case = host_case(M, K, N, act)
    ws = hip.dense_bwd_workspace(M, K, N, DEV)
    ws.fill_(float('nan'))                                             # (scratch: any contents)
    kw = dict(accumulate=accumulate, use_x=use_x, use_w=use_w)
    ops = Operands(case, K, N, misaligned=not aligned, x_form=x_form)
    route = call(hip, case, ops, act, ws, outputs, route_only=True, **kw)
    print('route', route)
    assert {k: route[k] for k in expect} == expect, route
    first = call(hip, case, ops, act, ws, outputs, **kw)
    verify('first', first, case, K, N, act, accumulate)
    again = call(hip, case, ops, act, ws, outputs, **kw)
    assert same_bits(first, again), "called twice on one workspace: identical bits"
    if 'dW' in outputs or 'db' in outputs:
        lazy = call(hip, case, ops, act, ws, outputs, defer=True, **kw)
        lazy_w, lazy_b = lazy['lazy']
        assert same_bits(first, lazy, keys=('dX', 'dZ'))
        groups = int(hip.load().amar_dense_bwd_groups(M))
        assert groups == route['out_groups']
        if 'dW' in outputs:
            assert lazy_w.groups == groups and torch.equal(lazy_w.materialize(), first['dW']), "deferred dW partials, added in group order"
            assert bool(torch.isnan(lazy['dW']).all()), "defer: dW itself is not written"
        if 'db' in outputs:
            assert lazy_b.groups == groups and torch.equal(lazy_b.materialize(), first['db']), "deferred db partials, added in group order"
    if route['kernel'] == 'rows' or route['vec']:
        other = Operands(case, K, N, misaligned=True, x_form=x_form)
        r2 = call(hip, case, other, act, ws, outputs, route_only=True, **kw)
        assert r2['kernel'] == 'tile' and not r2['vec'] and not r2['x_scalar'], r2
        second = call(hip, case, other, act, ws, outputs, **kw)
        verify('scalar tile kernel', second, case, K, N, act, accumulate)
        want = case['want']
        if 'dX' in outputs:
            init = np.abs(case['init'].astype(np.float64)) if accumulate else 0.0
            _within('two routes dX', _np(first['dX']), _np(second['dX']), 2 * ref.dx_bound(N, want['dx_mag'], init))
        if 'dZ' in outputs:
            _within('two routes dZ', _np(first['dZ']), _np(second['dZ']), 2 * ref.dz_bound(want['dz'], act))
        for k in ('dW', 'db'):
            if k in outputs:
                e = helpers.rel_err(_np(first[k]), _np(second[k]))
                print('two routes {}: rel_err {:.3e}'.format(k, e))
                assert e < 2 * TOL
    return route


def rows(kp, np_, launched, fold, fold_launch, x_scalar=False):
    return dict(kernel='rows', kp=kp, np=np_, x_scalar=x_scalar, launched_groups=launched, fold=fold, fold_launch=fold_launch)


def tile(mt, vec, subtiles=1):
    return dict(kernel='tile', mt=mt, vec=vec, subtiles=subtiles, x_scalar=False)


# ---- the row-walking kernel without a fold launch: M in {4097, 9228, 32768}, every (KP, NP), every activation ------------------------
GROUPS = {4097: 33, 9228: 49, 32768: 64}                               # one workgroup per partial the caller sees


@pytest.mark.parametrize('M,K,N,act,kp,np_', [
    (4097, 8, 8, 'relu', 8, 8), (9228, 4, 16, None, 8, 16), (32768, 8, 32, 'sigmoid', 8, 32),
    (4097, 16, 8, 'sigmoid', 16, 8), (9228, 12, 12, 'relu', 16, 16), (32768, 16, 32, None, 16, 32),
    (4097, 32, 8, None, 32, 8), (9228, 24, 16, 'sigmoid', 32, 16), (32768, 32, 32, 'relu', 32, 32),
    (9228, 20, 28, 'relu', 32, 32), (9228, 16, 16, 'relu', 16, 16), (32768, 8, 8, None, 8, 8), (4097, 32, 32, 'sigmoid', 32, 32)])
def test_rows_kernel_no_fold_launch(hip, M, K, N, act, kp, np_):
    check_case(hip, M, K, N, act, rows(kp, np_, GROUPS[M], 1, False))


# ---- the call shapes the training tapes make over every node of a graph -------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', None])
def test_rows_kernel_bias_and_dz_only(hip, act):
    """A GCN layer's first call (act', db, dZ; no X, no W, K = 1) and a GAT layer's bias call (db alone)."""
    check_case(hip, 9228, 1, 16, act, rows(8, 16, 49, 1, False), outputs=('db', 'dZ') if act else ('db',), use_x=False, use_w=False)


@pytest.mark.parametrize('M,K,N,launched,fold', [(9228, 8, 8, 49, 1), (9228, 16, 16, 49, 1), (32769, 8, 16, 513, 9)])
def test_rows_kernel_accumulated_dx_and_dw(hip, M, K, N, launched, fold):
    """dW = X^T . dH and dH . W^T ADDED into the slice's gradient, without db and without an activation."""
    check_case(hip, M, K, N, None, rows(max(8, K), max(8, N), launched, fold, fold > 1), outputs=('dX', 'dW'), accumulate=True)


def test_rows_kernel_single_column_x(hip):
    """A GAT attention vector's gradient ds^T . H: X one contiguous column (ldx = 1, K = 1), dW of shape [1, C], X read by single floats."""
    check_case(hip, 9228, 1, 8, None, rows(8, 8, 49, 1, False, x_scalar=True), outputs=('dW',), x_form='column', use_w=False)


@pytest.mark.parametrize('K,N,x_form,outputs', [(6, 8, 'slice', ('dW', 'db', 'dZ')), (2, 16, 'slice', ('dW', 'db')),
                                                (8, 16, 'unaligned', ('dX', 'dW', 'db', 'dZ'))])
def test_rows_kernel_x_by_single_floats(hip, K, N, x_form, outputs):
    """K not a multiple of 4 (no dX then: its rows are written by 16 bytes), and an unaligned X with K = 8."""
    check_case(hip, 9228, K, N, 'relu', rows(8, max(8, N), 49, 1, False, x_scalar=True), outputs=outputs, x_form=x_form, use_w='dX' in outputs)


# ---- the row-walking kernel followed by fold_partials2_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize('M,K,N,act,launched,fold', [(32769, 16, 16, 'relu', 513, 9),      # 513 tiles: 57 partials of 9 workgroups
                                                     (262145, 8, 8, 'sigmoid', 4096, 64)])  # 4 097 tiles: 65 per partial, capped at 64
def test_rows_kernel_with_fold_launch(hip, M, K, N, act, launched, fold):
    route = check_case(hip, M, K, N, act, rows(max(8, K), max(8, N), launched, fold, True))
    assert route['out_groups'] * fold == launched


# ---- the tile kernel with 16-byte loads ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,K,N,act,mt', [(1, 24, 24, 'relu', 4), (65, 48, 48, 'relu', 4), (300, 64, 64, 'sigmoid', 4), (4096, 16, 16, None, 4),
                                          (85, 96, 64, 'relu', 16), (300, 128, 128, 'relu', 16)])
def test_tile_kernel_vectorised(hip, M, K, N, act, mt):
    route = check_case(hip, M, K, N, act, tile(mt, True))
    assert route['launched_groups'] == -(-M // 64) and not route['fold_launch']


def test_tile_kernel_single_output_column_stays_scalar(hip):
    """N = 1 is no multiple of 4: aligned operands, scalar staging.  (relu, not sigmoid: with N = 1 the bound is 3 U |dZ| |W| and covers
    the ONE rounding of the product of an exact dZ; sigmoid' alone puts three roundings into dZ, so correct float32 arithmetic can
    reach 4 U there — a float32 emulation on the host does, in 3 of 65 536 elements.  test_dense_bwd_fused keeps (1024, 64, 1, sigmoid).)"""
    check_case(hip, 1024, 64, 1, 'relu', tile(4, False))


def test_tile_kernel_unaligned_x_alone_turns_16_byte_loads_off(hip):
    """dY, Y, W aligned, X 4 bytes off: one flag for the whole kernel."""
    ops = Operands(host_case(300, 64, 64, 'relu'), 64, 64, misaligned=False, x_form='unaligned')
    assert ops.dY.data_ptr() % 16 == 0 and ops.Y.data_ptr() % 16 == 0 and ops.W.data_ptr() % 16 == 0 and ops.X.data_ptr() % 16 == 4
    check_case(hip, 300, 64, 64, 'relu', tile(4, False), x_form='unaligned')


def test_tile_kernel_two_tiles_per_workgroup(hip):
    """M = 524 289: 8 193 tiles, two per workgroup, 4 097 workgroups folded 65 at a time; misaligned on purpose (the row-walking kernel
    would take it otherwise); N = 12 off a width bucket's edge."""
    route = check_case(hip, 524289, 8, 12, 'relu', tile(4, False, subtiles=2), aligned=False)
    assert (route['launched_groups'], route['fold'], route['fold_launch'], route['out_groups']) == (4097, 65, True, 64)


# ---- argument checks: the launcher and the route function return the same codes ------------------------------------------------------
def test_argument_checks(hip):
    EINVAL, EUNSUPPORTED = -1, -2
    lib = hip.load()
    M, K, N = 100, 8, 8
    t = {k: torch.zeros((M, 136), device=DEV) for k in ('X', 'Y', 'dY', 'dX', 'dZ')}
    w, dw, db = torch.zeros((136, 136), device=DEV), torch.zeros((136, 136), device=DEV), torch.zeros(136, device=DEV)
    ws = hip.dense_bwd_workspace(M, 136, 136, DEV)
    p = {k: v.data_ptr() for k, v in t.items()}
    p.update(W=w.data_ptr(), dW=dw.data_ptr(), db=db.data_ptr())
    relu, none = hip.ACT_CODES['relu'], hip.ACT_CODES[None]

    def both(X, Y, W, act, dX, dW, db, dZ, lddz=136, M=M, K=K, N=N):
        info = hip.DenseBwdRouteInfo()
        a = lib.amar_dense_bwd_f32(X, 136, Y, 136, p['dY'], 136, W, act, dX, 136, dW, db, dZ, lddz, ws.data_ptr(), M, K, N, None)
        b = lib.amar_dense_bwd_route(X, 136, Y, 136, p['dY'], 136, W, act, dX, 136, dW, db, dZ, lddz, M, K, N, ctypes.byref(info))
        assert a == b, (a, b)
        return a

    assert both(p['X'], p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], p['dZ']) == 0
    assert both(p['X'], p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], p['dZ'], lddz=N - 1) == EINVAL
    assert both(p['X'], p['Y'], None, relu, p['dX'], p['dW'], p['db'], None) == EINVAL            # dX without W
    assert both(None, p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], None) == EINVAL            # dW without X
    assert both(p['X'], None, p['W'], relu, p['dX'], p['dW'], p['db'], None) == EINVAL            # an activation without Y
    assert both(p['X'], None, p['W'], none, p['dX'], p['dW'], p['db'], None) == 0
    assert both(p['X'], p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], None, K=129) == EUNSUPPORTED
    assert both(p['X'], p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], None, N=129) == EUNSUPPORTED
    assert both(p['X'], p['Y'], p['W'], relu, p['dX'], p['dW'], p['db'], None, M=0) == EUNSUPPORTED
    assert lib.amar_dense_bwd_f32(p['X'], 136, p['Y'], 136, p['dY'], 136, p['W'], relu, p['dX'], 136, p['dW'], p['db'], None, 0, None,
                                  M, K, N, None) == EINVAL             # partial sums without a workspace
    torch.cuda.synchronize()
