"""CPU: how BasicRS.towers launches its two stacks (capi.towers_route / amar_chain_rows2_route) — the decisions on the cases of
tests/test_towers_one_launch_gpu.py and the way the workgroups of the one grid are dealt.  Host only: nothing is launched; the
launcher starts from the same route function, and its refusals return before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOWER = ['relu', 'relu', None]
G1, G2 = [24, 24, 24, 48], [48, 48, 48, 64]
ROWS = [(1, 1), (15, 17), (64, 1), (129, 4097), (4097, 129)]


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv('AMAR_TOWERS_LAUNCH', raising=False)


def test_entry_points_are_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for name in ('amar_chain_rows2_f32', 'amar_chain_rows2_route'):
        assert name in capi.SIGNATURES and re.search(r'\bint\s+' + name + r'\s*\(', header)
    m = re.search(r'typedef struct amar_chain_rows2_route_info \{\s*int32_t ([^;]+);\s*int64_t ([^;]+);', header)
    fields = [f.strip().split('[')[0] for f in (m.group(1) + ',' + m.group(2)).split(',')]
    assert fields == [n for n, _ in capi.ChainRows2RouteInfo._fields_]


@pytest.mark.parametrize('dims', [G1, G2], ids=['grid1', 'grid2'])
@pytest.mark.parametrize('rows', ROWS, ids=lambda r: '{}x{}'.format(*r))
def test_one_launch_on_the_gpu_cases(rows, dims):
    from deep_cbrs_amar_renaissance_amd import capi
    route, r = capi.towers_route(dims, TOWER, rows[0], dims, TOWER, rows[1], info=True)
    tiles = [-(-n // 128) for n in rows]
    assert route == 'one' and r['one_launch'] and r['lastlin'] and r['threads'] == 256
    assert r['shape'] == capi.chain_shape(*[-(-w // 16) for w in dims])
    assert list(r['blocks']) == tiles                                     # below the cap: a workgroup per 128-row tile, as the two launches
    assert r['lds_bytes'] == 4 * capi.load().amar_chain_pack_floats((ctypes.c_int32 * 4)(*dims), 3)


def test_declines():
    from deep_cbrs_amar_renaissance_amd import capi
    route = capi.towers_route
    assert route(G1, TOWER, 100, G1, TOWER, 100) == 'one'
    assert route(G1, TOWER, 100, G1, TOWER, 100, u_ids=True) == 'two' and route(G1, TOWER, 100, G1, TOWER, 100, i_ids=True) == 'two'
    assert route(G1, TOWER, 100, G2, TOWER, 100) == 'two'                 # unequal shapes
    assert route(G1, TOWER, 100, [8, 24, 24, 48], TOWER, 100) == 'two'    # same widths behind another input tile count
    assert route(G1, TOWER, 100, G1, ['relu'] * 3, 100) == 'two'          # a linear last layer on one side only
    assert route(G1, ['relu'] * 3, 100, G1, ['relu'] * 3, 100) == 'one'
    assert route(G1, TOWER, 0, G1, TOWER, 100) == 'two' and route(G1, TOWER, 100, G1, TOWER, 0) == 'two'          # an empty side
    assert route(G1, [None] * 3, 100, G1, [None] * 3, 100) == 'two'       # no tower kernel for the stack
    assert route([32, 24, 24, 48], TOWER, 100, [32, 24, 24, 48], TOWER, 100) == 'one'                              # 2 tiles like grid1
    assert route([24, 24, 24, 24, 48], ['relu'] * 3 + [None], 100, [24, 24, 24, 24, 48], ['relu'] * 3 + [None], 100) == 'two'   # four layers
    assert route(G1, TOWER, 100, G1[:-1], TOWER[:-1], 100) == 'two'       # another layer count
    assert route([22, 24, 24, 48], TOWER, 100, G1, TOWER, 100) == 'two'   # an argument the launcher refuses: two launches report it
    # 32-bit row positions: a side too long for the tower kernel
    top = (1 << 30) - (4 << 20)
    assert route(G1, TOWER, top - 1, G1, TOWER, 100) == 'one' and route(G1, TOWER, top, G1, TOWER, 100) == 'two'


def test_switch_keeps_two_launches(monkeypatch):
    from deep_cbrs_amar_renaissance_amd import capi
    monkeypatch.setenv('AMAR_TOWERS_LAUNCH', 'two')
    assert capi.towers_route(G1, TOWER, 100, G1, TOWER, 100) == 'two'
    monkeypatch.setenv('AMAR_TOWERS_LAUNCH', 'one')                        # only 'two' is a switch
    assert capi.towers_route(G1, TOWER, 100, G1, TOWER, 100) == 'one' and capi.towers_route(G1, TOWER, 100, G2, TOWER, 100) == 'two'


@pytest.mark.parametrize('dims,cap', [(G1, 768), (G2, 1024)], ids=['grid1', 'grid2'])
def test_workgroups_are_dealt_by_rows(dims, cap):
    from deep_cbrs_amar_renaissance_amd import capi
    blocks = lambda a, b: capi.towers_route(dims, TOWER, a, dims, TOWER, b, info=True)[1]['blocks']                   # noqa: E731
    assert blocks(128 * (cap - 300), 128 * 300) == (cap - 300, 300)        # exactly the cap: still a workgroup per tile
    assert blocks(128 * (cap - 300) + 1, 128 * 300) == (cap - 300, 300)    # one tile more: the cap, dealt by tiles (rounded)
    b = blocks(386560, 204032)                                             # ml1m(s=64)
    assert sum(b) == cap and abs(b[0] - cap * 3020 / (3020 + 1594)) <= 1
    assert blocks(10 ** 6, 100) == (cap - 1, 1) and blocks(100, 10 ** 6) == (1, cap - 1)     # at least one each
    for a, c in ((5 * 10 ** 5, 3 * 10 ** 5), (10 ** 6, 128 * 40), (128 * 3, 10 ** 7)):
        b = blocks(a, c)
        assert sum(b) == cap and 1 <= b[0] <= -(-a // 128) and 1 <= b[1] <= -(-c // 128), (a, c, b)


def test_launcher_refuses_like_the_route():
    """amar_chain_rows2_f32 on made-up addresses, only where it cannot launch: EUNSUPPORTED where the route says two launches, EINVAL
    on a bad argument of either problem, on NULL arrays and on a NULL info."""
    from deep_cbrs_amar_renaissance_amd import capi
    lib = capi.load()
    base = 0x7F0000100000

    def args(dims, acts, rows, lda=None, misalign=0):
        a, keep = capi._chain2_raw([base + misalign, base + (1 << 40)], lda or [d[0] for d in dims], [base + (2 << 40), base + (3 << 40)], dims, acts,
                                   [base + (4 << 40), base + (5 << 40)], [d[-1] for d in dims], rows)
        return a, keep

    info = capi.ChainRows2RouteInfo()
    a, keep = args((G1, G2), (TOWER, TOWER), (100, 100))
    assert lib.amar_chain_rows2_route(*a, ctypes.byref(info)) == 0 and not info.one_launch
    assert lib.amar_chain_rows2_f32(*a, None) == -2
    a, keep = args((G1, G1), (TOWER, TOWER), (100, 0))
    assert lib.amar_chain_rows2_route(*a, ctypes.byref(info)) == 0 and not info.one_launch and lib.amar_chain_rows2_f32(*a, None) == -2
    for bad in (args((G1, G1), (TOWER, TOWER), (100, 100), lda=[20, 24]), args((G1, G1), (TOWER, TOWER), (100, 100), misalign=8),
                args((G1, G1), (TOWER, TOWER), (100, -1))):
        assert lib.amar_chain_rows2_route(*bad[0], ctypes.byref(info)) == -1 and lib.amar_chain_rows2_f32(*bad[0], None) == -1
    a, keep = args((G1, G1), (TOWER, TOWER), (100, 100))
    assert lib.amar_chain_rows2_route(*a, None) == -1
    for k in (0, 1, 2, 3, 4, 6, 7, 8):
        b = list(a)
        b[k] = None
        assert lib.amar_chain_rows2_route(*b, ctypes.byref(info)) == -1 and lib.amar_chain_rows2_f32(*b, None) == -1, k
