"""amar_dense_bwd_route on the host (no GPU): which kernel amar_dense_bwd_f32 takes for a call, asked with made-up addresses — the
function looks at alignment and NULL only, nothing is dereferenced.  The launcher calls the same function, so these are the
launcher's thresholds: tile kernel <-> row-walking kernel, with / without a fold launch, the cap of `fold`, two tiles per workgroup,
the compile-time widths, and the room the raw partials need in the workspace."""
import ctypes

import pytest

from deep_cbrs_amar_renaissance_amd import capi

BASE = 0x7F0000100000                                                  # 16-byte aligned; + 8: half way between two boundaries
NONE, RELU, SIGMOID = (capi.ACT_CODES[a] for a in (None, 'relu', 'sigmoid'))
OPERANDS = ('X', 'Y', 'dY', 'W', 'dX', 'dW', 'db', 'dZ')


def route(M, K, N, act=RELU, outputs=('dX', 'dW', 'db'), misaligned=(), ld=None, code=False):
    """The route of a call that asks for `outputs`, every operand a row-major matrix at an aligned made-up address with its width
    rounded up to a multiple of 4 (+ 4) as leading dimension, except the operands in `misaligned` (address + 8 bytes) and the leading dimensions in `ld`."""
    lead = {'X': (K + 3) // 4 * 4 + 4, 'Y': (N + 3) // 4 * 4 + 4, 'dY': (N + 3) // 4 * 4 + 4, 'dX': (K + 3) // 4 * 4 + 4, 'dZ': (N + 3) // 4 * 4 + 4}
    lead.update(ld or {})
    given = {'dY', 'X', 'W'} | set(outputs) | ({'Y'} if act != NONE else set())
    addr = {name: (BASE + 0x100000 * i + (8 if name in misaligned else 0)) if name in given else None for i, name in enumerate(OPERANDS)}
    info = capi.DenseBwdRouteInfo()
    rc = capi.load().amar_dense_bwd_route(addr['X'], lead['X'], addr['Y'], lead['Y'], addr['dY'], lead['dY'], addr['W'], act, addr['dX'], lead['dX'],
                                          addr['dW'], addr['db'], addr['dZ'], lead['dZ'], M, K, N, ctypes.byref(info))
    if code:
        return rc
    assert rc == 0, rc
    return info.as_dict()


def plan(M):
    """DESIGN.md's cut of M rows, restated: 64-row tiles, at most 8 192 workgroups, at most 64 partials for the consumer."""
    tiles = -(-M // 64)
    sub = max(1, -(-tiles // 8192))
    launch = -(-tiles // sub)
    fold = -(-launch // 64) if launch > 64 else 1
    return sub, launch, fold, -(-launch // fold)


def test_tile_to_rows_threshold():
    r = route(4096, 8, 8)
    assert r['kernel'] == 'tile' and r['mt'] == 4 and r['vec'] and r['subtiles'] == 1
    assert (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (64, 1, False, 64)
    r = route(4097, 8, 8)
    assert r['kernel'] == 'rows' and (r['kp'], r['np']) == (8, 8) and not r['x_scalar']
    assert (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (33, 1, False, 33)     # 65 tiles, two per partial
    r = route(4097, 8, 8, misaligned=('dY',))                          # the same call on the tile kernel: a fold launch from 65 tiles on
    assert r['kernel'] == 'tile' and not r['vec'] and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (65, 2, True, 33)


def test_rows_fold_launch_threshold_and_cap():
    r = route(32768, 16, 16)
    assert r['kernel'] == 'rows' and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (64, 1, False, 64)
    r = route(32769, 16, 16)
    assert r['kernel'] == 'rows' and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (513, 9, True, 57)
    r = route(32769, 16, 16, outputs=('dX',))                          # nothing to fold without dW / db
    assert r['kernel'] == 'rows' and not r['fold_launch']
    r = route(262144, 8, 8)
    assert r['kernel'] == 'rows' and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (4096, 64, True, 64)
    r = route(262145, 8, 8)                                            # 4 097 tiles: 65 per partial, capped at 64 workgroups
    assert r['kernel'] == 'rows' and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (4096, 64, True, 64)
    r = route(262145, 8, 8, misaligned=('dY',))                        # ... the tile kernel is not capped
    assert r['kernel'] == 'tile' and (r['launched_groups'], r['fold'], r['fold_launch'], r['out_groups']) == (4097, 65, True, 64)


def test_tile_kernel_two_tiles_per_workgroup():
    r = route(524288, 8, 12, misaligned=('dY',))
    assert r['kernel'] == 'tile' and r['subtiles'] == 1 and (r['launched_groups'], r['fold'], r['out_groups']) == (8192, 128, 64)
    r = route(524289, 8, 12, misaligned=('dY',))
    assert r['kernel'] == 'tile' and r['subtiles'] == 2 and (r['launched_groups'], r['fold'], r['out_groups']) == (4097, 65, 64)
    r = route(524289, 8, 12)
    assert r['kernel'] == 'rows' and r['subtiles'] == 0 and (r['launched_groups'], r['fold'], r['out_groups']) == (4096, 64, 64)


@pytest.mark.parametrize('what,kwargs', [
    ('K > 32', dict(K=36)), ('N > 32', dict(N=36)), ('N % 4', dict(N=6)),
    ('dY', dict(misaligned=('dY',))), ('Y', dict(misaligned=('Y',))), ('W', dict(misaligned=('W',))), ('dX', dict(misaligned=('dX',))),
    ('dZ', dict(misaligned=('dZ',))), ('lddx % 4', dict(ld={'dX': 18})), ('lddz % 4', dict(ld={'dZ': 18})), ('lddy % 4', dict(ld={'dY': 18})),
    ('ldy % 4', dict(ld={'Y': 18}))])
def test_back_to_the_tile_kernel(what, kwargs):
    kw = dict(M=9228, K=16, N=16, outputs=('dX', 'dW', 'db', 'dZ'))
    assert route(**kw)['kernel'] == 'rows'
    kw.update(kwargs)
    r = route(**kw)
    assert r['kernel'] == 'tile' and r['kp'] == r['np'] == 0 and not r['x_scalar'], what
    # the tile kernel loads dY / Y / W / X by 16 bytes under the same conditions and stores dX / dZ by single floats
    assert r['vec'] == (what in ('K > 32', 'N > 32', 'dX', 'dZ', 'lddx % 4', 'lddz % 4')), what
    # an operand the call does not use is not looked at
    assert route(9228, 16, 16, act=NONE, outputs=('dX', 'dW'), misaligned=('Y', 'dZ'))['kernel'] == 'rows'
    assert route(9228, 6, 16, outputs=('dW', 'db'), misaligned=('W', 'dX'))['kernel'] == 'rows'


def test_x_read_by_single_floats_keeps_the_rows_kernel():
    assert not route(9228, 8, 16, outputs=('dW', 'db'))['x_scalar']
    for kwargs in (dict(K=8, misaligned=('X',)), dict(K=8, ld={'X': 9}), dict(K=6), dict(K=2), dict(K=1, ld={'X': 1})):
        r = route(M=9228, N=16, outputs=('dW', 'db'), **kwargs)
        assert r['kernel'] == 'rows' and r['x_scalar'] and r['vec'], kwargs
    # with dX, K must be a multiple of 4 (W and dX rows are read and written by 16 bytes)
    assert route(9228, 6, 16)['kernel'] == 'tile'
    # X is only read for dW
    assert not route(9228, 8, 16, outputs=('dX', 'db'), misaligned=('X',))['x_scalar']
    # on the tile kernel an unaligned X alone turns the 16-byte loads off
    r = route(300, 64, 64, misaligned=('X',))
    assert r['kernel'] == 'tile' and not r['vec'] and not r['x_scalar']


@pytest.mark.parametrize('K,kp', [(1, 8), (4, 8), (8, 8), (9, 16), (12, 16), (16, 16), (17, 32), (20, 32), (32, 32)])
@pytest.mark.parametrize('N,np_', [(4, 8), (8, 8), (12, 16), (16, 16), (20, 32), (32, 32)])
def test_rows_kernel_widths(K, kp, N, np_):
    r = route(9228, K, N, outputs=('dW', 'db', 'dZ'))
    assert r['kernel'] == 'rows' and (r['kp'], r['np']) == (kp, np_) and r['mt'] == 0


@pytest.mark.parametrize('K,N,mt', [(1, 1, 4), (64, 64, 4), (16, 128, 4), (128, 32, 4), (65, 64, 16), (64, 65, 16), (96, 64, 16), (48, 81, 16),
                                    (128, 128, 16), (32, 128, 4), (33, 128, 16)])
def test_tile_kernel_accumulator_count(K, N, mt):
    """(K rounded up to 16 / 16) x (N rounded up to 16 / 16) tiles of dW over four waves: up to 16 tiles -> 4 per wave, else 16."""
    r = route(300, K, N)
    assert r['kernel'] == 'tile' and r['mt'] == mt and r['vec'] == (K % 4 == 0 and N % 4 == 0)
    assert r['mt'] == (4 if -(-K // 16) * -(-N // 16) <= 16 else 16)


@pytest.mark.parametrize('M', [1, 64, 65, 4096, 4097, 9228, 32768, 32769, 40000, 262144, 262145, 524288, 524289, 590592, 600001, 5_000_000])
@pytest.mark.parametrize('rows', [True, False])
def test_groups_fit_the_workspace(M, rows):
    """The visible partials [out_groups] come first in the workspace, the raw ones [launched_groups] behind them where a fold launch
    follows: both must fit in amar_dense_bwd_workspace_floats, every visible partial must have at least one raw partial, and `fold`
    of them at most."""
    lib = capi.load()
    K, N = 16, 8
    r = route(M, K, N, misaligned=() if rows else ('dY',))
    sub, launch, fold, out = plan(M)
    assert r['kernel'] == ('rows' if rows and M > 4096 else 'tile')
    assert r['out_groups'] == out == lib.amar_dense_bwd_groups(M) and 1 <= out <= 64
    per = K * N + N
    floats = lib.amar_dense_bwd_workspace_floats(M, K, N)
    if r['fold_launch']:
        assert r['fold'] > 1 and 4 + (out + r['launched_groups']) * per <= floats
        assert (out - 1) * r['fold'] < r['launched_groups'] <= out * r['fold']
    else:
        assert r['fold'] == 1 and r['launched_groups'] == out and 4 + out * per <= floats
    if r['kernel'] == 'tile':
        assert (r['subtiles'], r['launched_groups'], r['fold']) == (sub, launch, fold)
        assert r['launched_groups'] * r['subtiles'] * 64 >= M          # every row has a tile
    else:
        assert r['fold'] == (1 if M <= 32768 else min(fold, 64)) and r['launched_groups'] == out * r['fold'] <= 4096


def test_route_argument_checks():
    """The codes of amar_dense_bwd_f32's own argument checks."""
    EINVAL, EUNSUPPORTED = -1, -2
    assert route(100, 8, 8, code=True) == 0
    assert route(100, 8, 8, ld={'dZ': 7}, outputs=('dZ', 'db'), code=True) == EINVAL
    assert route(100, 8, 8, ld={'dY': 7}, code=True) == EINVAL and route(100, 8, 8, ld={'Y': 7}, code=True) == EINVAL
    assert route(100, 8, 8, ld={'dX': 7}, code=True) == EINVAL and route(100, 8, 8, ld={'X': 7}, code=True) == EINVAL
    assert route(100, 8, 8, outputs=(), code=True) == EINVAL and route(-1, 8, 8, code=True) == EINVAL and route(100, 0, 8, code=True) == EINVAL
    assert route(100, 8, 8, act=7, code=True) == EINVAL
    lib, info = capi.load(), capi.DenseBwdRouteInfo()
    a = BASE
    assert lib.amar_dense_bwd_route(a, 8, a, 8, a, 8, None, NONE, a, 8, None, None, None, 0, 100, 8, 8, ctypes.byref(info)) == EINVAL    # dX without W
    assert lib.amar_dense_bwd_route(None, 8, a, 8, a, 8, a, NONE, None, 8, a, None, None, 0, 100, 8, 8, ctypes.byref(info)) == EINVAL    # dW without X
    assert lib.amar_dense_bwd_route(a, 8, None, 0, a, 8, a, RELU, a, 8, a, a, None, 0, 100, 8, 8, ctypes.byref(info)) == EINVAL          # an activation without Y
    assert lib.amar_dense_bwd_route(a, 8, a, 8, None, 8, a, NONE, a, 8, a, a, None, 0, 100, 8, 8, ctypes.byref(info)) == EINVAL          # no dY
    assert lib.amar_dense_bwd_route(a, 8, a, 8, a, 8, a, NONE, a, 8, a, a, None, 0, 100, 8, 8, None) == EINVAL
    assert route(100, 129, 8, code=True) == EUNSUPPORTED and route(100, 8, 129, code=True) == EUNSUPPORTED and route(0, 8, 8, code=True) == EUNSUPPORTED
    assert route(100, 128, 128, code=True) == 0
    # the flags a caller ORs into `act` do not change the route
    assert route(9228, 8, 8, act=RELU | capi.DENSE_BWD_DEFER | capi.DENSE_BWD_ACCUM_DX) == route(9228, 8, 8)
