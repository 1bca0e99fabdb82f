"""amar_chain_route / amar_chain_segments_route and amar_chain_pack_f32 on the host (no GPU).

The route functions are asked with made-up device addresses — they look at alignment and NULL only; dims, acts and the segment arrays are
real host arrays.  The launchers start from the same function, so these are the launchers' thresholds; every refusal returns before any
HIP call (csrc/amar_chain.hip: chain_route makes none), so the refusals are checked on the launchers themselves too.  The pack functions
are compared with the numpy restatement of their layout in tests/chain_ref.py, and the reference of tests/test_chain_forms_gpu.py is
checked here against itself: the float32 numpy evaluation of every GPU case stays inside the case's bound."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd import capi
from tests import chain_ref as cr

BASE = 0x7F0000100000                                                  # 16-byte aligned
EINVAL, EUNSUPPORTED = -1, -2
CODE = {None: 0, 'relu': 1, 'sigmoid': 2}
GENERIC, PIPE, ROWS = capi.CHAIN_KERNEL_GENERIC, capi.CHAIN_KERNEL_PIPE, capi.CHAIN_KERNEL_ROWS
assert (GENERIC, PIPE, ROWS) == (cr.GENERIC, cr.PIPE, cr.ROWS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_ONLY = os.environ.get('AMAR_PAIR_MFMA') == 'f32'                    # the switch of the split products, as this process started


def _addr(i, off=0):
    return BASE + 0x10000000 * i + off


class Call:
    """The arguments of amar_chain_indexed_f32 at made-up addresses; `edit` changes them by name.  units / acts as capi.chain takes them."""

    def __init__(self, P, Da, Db, units, acts=None, sum_inputs=False, in_act=None, ids=False, out_index=False, **edit):
        dims = [Da if sum_inputs else Da + Db] + list(units)
        acts = acts if acts is not None else ['relu'] * len(units)
        self.v = dict(A=_addr(0), lda=Da + 4, Da=Da, ids_a=_addr(1, 4) if ids else None, base_a=0,
                      B=_addr(2) if Db else None, ldb=Db + 4 if Db else 0, Db=Db, ids_b=_addr(3, 4) if ids and Db else None, base_b=0,
                      sum_inputs=int(sum_inputs), in_act=CODE.get(in_act, in_act), wpack=_addr(4), dims=dims, acts=[CODE.get(a, a) for a in acts],
                      n_layers=len(units), out=_addr(5), ldo=(dims[-1] + 3) // 4 * 4 + 4, out_index=_addr(6, 4) if out_index else None, P=P)
        self.v.update(edit)

    def args(self):
        v = self.v
        arr = lambda t, x: None if x is None else (t * max(1, len(x)))(*x)                                  # noqa: E731
        self.keep = [arr(ctypes.c_int32, v['dims']), arr(ctypes.c_int32, v['acts'])]
        return [v['A'], v['lda'], v['Da'], v['ids_a'], v['base_a'], v['B'], v['ldb'], v['Db'], v['ids_b'], v['base_b'], v['sum_inputs'], v['in_act'],
                v['wpack'], self.keep[0], self.keep[1], v['n_layers'], v['out'], v['ldo'], v['out_index'], v['P']]

    def route(self, code=False):
        info = capi.ChainRouteInfo()
        rc = capi.load().amar_chain_route(*self.args(), ctypes.byref(info))
        if code:
            return rc
        assert rc == 0, rc
        return info.as_dict()

    def launch(self):
        return capi.load().amar_chain_indexed_f32(*self.args(), None)


class Seg:
    """The arguments of amar_chain_segments_f32 likewise."""

    def __init__(self, P, widths, units, acts=None, ids=False, **edit):
        acts = acts if acts is not None else ['relu'] * len(units)
        self.v = dict(seg=[_addr(10 + j) for j in range(len(widths))], seg_ld=[w + 4 * j for j, w in enumerate(widths)], seg_width=list(widths),
                      n_seg=len(widths), ids=_addr(1, 4) if ids else None, base=0, wpack=_addr(4), dims=[sum(widths)] + list(units),
                      acts=[CODE.get(a, a) for a in acts], n_layers=len(units), out=_addr(5), ldo=(units[-1] + 3) // 4 * 4 + 4, P=P)
        self.v.update(edit)

    def args(self):
        v = self.v
        arr = lambda t, x: None if x is None else (t * max(1, len(x)))(*x)                                  # noqa: E731
        self.keep = [arr(ctypes.c_void_p, v['seg']), arr(ctypes.c_int64, v['seg_ld']), arr(ctypes.c_int32, v['seg_width']), arr(ctypes.c_int32, v['dims']),
                     arr(ctypes.c_int32, v['acts'])]
        k = self.keep
        return [k[0], k[1], k[2], v['n_seg'], v['ids'], v['base'], v['wpack'], k[3], k[4], v['n_layers'], v['out'], v['ldo'], v['P']]

    def route(self, code=False):
        info = capi.ChainRouteInfo()
        rc = capi.load().amar_chain_segments_route(*self.args(), ctypes.byref(info))
        if code:
            return rc
        assert rc == 0, rc
        return info.as_dict()

    def launch(self):
        return capi.load().amar_chain_segments_f32(*self.args(), None)


def _both(case):
    """The route's code; the launcher is asked too where it cannot launch (a refusal, or no rows): the addresses are made up."""
    a = case.route(code=True)
    if a != 0 or case.v['P'] == 0:
        b = case.launch()
        assert a == b, (a, b)
    return a


def _edited(call, **edit):
    call.v.update(edit)
    return call


def _sub(route, **want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)
    return True


def pair(P, W, depth, dot=True, **kw):
    """A pair-stage call: relu(A[ida] + B[idb]) through `depth` square ReLU layers of W (and a sigmoid 1-unit layer)."""
    kw.setdefault('ids', True)
    kw.setdefault('sum_inputs', True)
    kw.setdefault('in_act', 'relu')
    units = [W] * depth + ([1] if dot else [])
    return Call(P, W, W, units, ['relu'] * depth + (['sigmoid'] if dot else []), **kw)


# ---- the pack -------------------------------------------------------------------------------------------------------------------------
PACK_DIMS = [[48, 48, 48, 1], [64, 64, 1], [20, 30, 44, 1], [24, 100, 128], [128, 128], [4, 20], [8, 1], [1, 1], [16, 1, 1], [24, 30, 22, 12],
             [100, 30, 1], [44, 128, 20, 1], [16] * 9]


@pytest.mark.parametrize('dims', PACK_DIMS, ids=lambda d: '-'.join(map(str, d)))
def test_pack_matches_the_restated_layout(dims):
    rng = np.random.default_rng(sum(dims))
    ks = [rng.standard_normal((k, n)).astype(np.float32) + np.float32(3) for k, n in zip(dims[:-1], dims[1:])]        # no zero among the weights:
    bs = [rng.standard_normal(n).astype(np.float32) + np.float32(3) for n in dims[1:]]                                # a zero in the blob is padding
    blob, pdims = capi.chain_pack(ks, bs)
    want = cr.pack(ks, bs)
    assert pdims == dims and blob.dtype == np.float32 and blob.shape == want.shape == (cr.pack_floats(dims),)
    assert capi.load().amar_chain_pack_floats((ctypes.c_int32 * len(dims))(*dims), len(dims) - 1) == cr.pack_floats(dims)
    assert np.array_equal(blob.view(np.uint32), want.view(np.uint32))                                                  # pads are +0.0 exactly
    n_values = sum(k.size + b.size for k, b in zip(ks, bs))
    assert int((blob != 0).sum()) == n_values and int((blob.view(np.uint32) == 0).sum()) == blob.size - n_values


def test_pack_layout_spelled_out():
    """The fragment formula element by element on one ragged layer, and the 1-unit layer's 16 KT + 4 floats, independent of cr.pack."""
    K, N = 20, 30
    w = (np.arange(K * N, dtype=np.float32) + 1).reshape(K, N)
    b = -(np.arange(N, dtype=np.float32) + 1)
    d = np.arange(N, dtype=np.float32)[:, None] + np.float32(0.5)
    blob, _ = capi.chain_pack([w, d], [b, np.array([9.0], np.float32)])
    KT, NT = 2, 2
    for m in range(NT):
        for t in range(KT):
            for lane in range(64):
                for r in range(4):
                    k, n = 16 * t + 4 * (lane >> 4) + r, 16 * m + (lane & 15)
                    assert blob[((m * KT + t) * 64 + lane) * 4 + r] == (w[k, n] if k < K and n < N else 0)
    off = NT * KT * 256
    assert np.array_equal(blob[off:off + 32], np.concatenate([b, np.zeros(2, np.float32)]))
    off += 32
    assert np.array_equal(blob[off:off + 32], np.concatenate([d[:, 0], np.zeros(2, np.float32)]))
    assert blob[off + 32:].tolist() == [9.0, 0.0, 0.0, 0.0] and blob.size == off + 36
    # a single 1-unit layer is an ordinary layer (one fragment tile), not a dot
    blob, _ = capi.chain_pack([np.full((8, 1), 2, np.float32)], [np.array([5.0], np.float32)])
    assert blob.size == 256 + 16 and blob[256] == 5.0 and float(blob.sum()) == 8 * 2 + 5


def test_pack_refusals():
    lib = capi.load()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                                     # noqa: E731
    assert lib.amar_chain_pack_floats(None, 1) == EINVAL
    assert lib.amar_chain_pack_floats(i32(8, 8), 0) == EINVAL and lib.amar_chain_pack_floats(i32(*[8] * 10), 9) == EINVAL
    assert lib.amar_chain_pack_floats(i32(8, 0), 1) == EINVAL and lib.amar_chain_pack_floats(i32(0, 8), 1) == EINVAL
    assert lib.amar_chain_pack_floats(i32(8, 8, -1), 2) == EINVAL
    assert lib.amar_chain_pack_floats(i32(*[8] * 9), 8) == 8 * (256 + 16)
    w, b, out = np.ones((8, 8), np.float32), np.ones(8, np.float32), np.full(272, np.nan, np.float32)
    kp, bp = (ctypes.c_void_p * 1)(w.ctypes.data), (ctypes.c_void_p * 1)(b.ctypes.data)
    assert lib.amar_chain_pack_f32(None, bp, i32(8, 8), 1, out.ctypes.data) == EINVAL
    assert lib.amar_chain_pack_f32(kp, None, i32(8, 8), 1, out.ctypes.data) == EINVAL
    assert lib.amar_chain_pack_f32(kp, bp, i32(8, 8), 1, None) == EINVAL
    assert lib.amar_chain_pack_f32(kp, bp, None, 1, out.ctypes.data) == EINVAL
    assert lib.amar_chain_pack_f32(kp, bp, i32(8, 0), 1, out.ctypes.data) == EINVAL
    assert np.isnan(out).all()                                                                                          # nothing was written
    assert lib.amar_chain_pack_f32(kp, bp, i32(8, 8), 1, out.ctypes.data) == 0 and not np.isnan(out).any()
    with pytest.raises(ValueError):
        capi.chain_pack([np.ones((8, 8), np.float32)], [np.ones(7, np.float32)])


# ---- maxt, full, am ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W,maxt', [(4, 3), (48, 3), (52, 4), (64, 4), (68, 8), (96, 8), (128, 8)])
def test_maxt_thresholds(W, maxt):
    for call in (Call(100, 8, 0, [W]), Call(100, W, 0, [8]), Call(100, 8, 0, [8, W - 3 if W > 4 else W, 8, 1]), Call(100, 8, 0, [8, W, 1])):
        assert call.route()['maxt'] == maxt and call.route()['kernel'] == GENERIC


def test_widths_above_128_are_unsupported():
    for call in (Call(100, 8, 0, [132]), Call(100, 132, 0, [8]), Call(100, 8, 0, [129, 1]), Call(100, 64, 68, [8])):
        assert _both(call) == EUNSUPPORTED
    assert Call(100, 64, 64, [128, 1]).route(code=True) == 0
    # ... and so is a blob above 150 KB: three 128 x 128 layers are 198 144 bytes, two are 132 096
    assert _both(Call(100, 128, 0, [128, 128, 128])) == EUNSUPPORTED
    assert Call(100, 128, 0, [128, 128]).route()['lds_bytes'] == 132096 == 4 * cr.pack_floats([128, 128, 128])


def test_full_needs_every_width_at_maxt_tiles():
    assert Call(100, 48, 0, [48, 48, 1]).route()['full'] and Call(100, 36, 0, [33, 48, 1]).route()['full']
    assert Call(100, 24, 24, [48]).route()['full'] and Call(100, 64, 64, [128, 116, 1]).route()['full']
    for dims in ([32, 48, 48, 1], [48, 32, 48, 1], [48, 48, 32, 1], [48, 32, 48], [48, 48, 32], [32, 48, 48], [48, 64, 48]):
        assert not Call(100, dims[0], 0, dims[1:]).route()['full'], dims
    assert not Call(100, 64, 64, [128, 112, 1]).route()['full'] and not Call(100, 64, 48, [128, 128, 1]).route()['full']
    assert Call(100, 64, 64, [64, 1], sum_inputs=True).route()['full'] and not Call(100, 64, 64, [64, 1]).route()['full']   # (the sum is 64 wide, not 128)


def test_activation_mode():
    am = lambda *a, **k: Call(100, *a, **k).route()['am']                                                              # noqa: E731
    assert am(24, 0, [24, 24]) == 1 and am(24, 24, [48, 48, 1], ['relu', 'relu', 'sigmoid']) == 1
    # the 1-unit layer's activation never counts
    assert [am(24, 24, [48, 1], ['relu', a]) for a in (None, 'relu', 'sigmoid')] == [1, 1, 1]
    # a linear last layer: am 2 without a 1-unit layer, 0 with one behind it
    assert am(24, 0, [24, 24], ['relu', None]) == 2 and am(24, 0, [24], [None]) == 2
    assert am(24, 0, [24, 24, 1], ['relu', None, 'sigmoid']) == 0
    # a linear or sigmoid layer anywhere else
    assert am(24, 0, [24, 24], [None, 'relu']) == 0 and am(24, 0, [24, 24], [None, None]) == 0 and am(24, 0, [24, 24, 24], ['relu', None, None]) == 0
    assert am(24, 0, [24, 24], ['sigmoid', 'relu']) == 0 and am(24, 0, [24, 24], ['relu', 'sigmoid']) == 0
    assert am(24, 0, [24, 24, 1], ['sigmoid', 'relu', 'sigmoid']) == 0
    # in_act counts with sum_inputs only
    for in_act, want in ((None, 0), ('sigmoid', 0), ('relu', 1)):
        assert am(24, 24, [24, 24], sum_inputs=True, in_act=in_act) == want
        assert am(24, 24, [24, 24], ['relu', None], sum_inputs=True, in_act=in_act) == (2 if want else 0)
        assert am(24, 24, [48, 24], in_act=in_act) == 1 and am(24, 0, [24, 24], in_act=in_act) == 1


# ---- the pair-stage kernel: each of its conditions, both sides ----------------------------------------------------------------------------
def test_pipe_conditions():
    r = pair(1000, 48, 2).route()
    assert _sub(r, kernel=PIPE, maxt=3, full=True, am=1, split=not F32_ONLY, scatter=False, has_dot=True, layers=2, threads=256, blocks=8)
    assert _sub(pair(1000, 64, 1, out_index=True).route(), kernel=PIPE, maxt=4, scatter=True, split=not F32_ONLY)
    assert pair(1000, 48, 2, dot=False).route()['kernel'] == PIPE
    # Da == 16 maxt
    assert pair(1000, 36, 2).route()['kernel'] == GENERIC and pair(1000, 44, 2).route()['kernel'] == GENERIC and pair(1000, 52, 1).route()['kernel'] == GENERIC
    # both id lists
    assert pair(1000, 48, 2, ids_a=None).route()['kernel'] == GENERIC and pair(1000, 48, 2, ids_b=None).route()['kernel'] == GENERIC
    assert pair(1000, 48, 2, ids=False).route()['kernel'] == GENERIC
    # the summed ReLU input
    assert pair(1000, 48, 2, in_act=None).route()['kernel'] == GENERIC and pair(1000, 48, 2, in_act='sigmoid').route()['kernel'] == GENERIC
    assert Call(1000, 24, 24, [48, 48, 1], ids=True).route()['kernel'] == GENERIC                                       # concatenated, not summed
    # ReLU layers, square
    assert Call(1000, 48, 48, [48, 48, 1], ['relu', 'sigmoid', 'sigmoid'], sum_inputs=True, in_act='relu', ids=True).route()['kernel'] == GENERIC
    assert Call(1000, 48, 48, [48, 48], ['relu', None], sum_inputs=True, in_act='relu', ids=True).route()['kernel'] == GENERIC
    assert Call(1000, 48, 48, [48, 32, 1], None, sum_inputs=True, in_act='relu', ids=True).route()['kernel'] == GENERIC
    # the 1-unit layer's activation is free
    for a in (None, 'relu', 'sigmoid'):
        assert Call(1000, 48, 48, [48, 1], ['relu', a], sum_inputs=True, in_act='relu', ids=True).route()['kernel'] == PIPE
    # maxt <= 4
    assert pair(1000, 64, 1).route()['kernel'] == PIPE and pair(1000, 128, 1).route()['kernel'] == GENERIC
    assert pair(1000, 80, 1).route()['kernel'] == GENERIC and pair(1000, 96, 1).route()['kernel'] == GENERIC
    # 32-bit row bytes and positions
    top = (1 << 30) - (4 << 20)
    assert pair(1000, 48, 2, lda=(1 << 30) - 4).route()['kernel'] == PIPE and pair(1000, 48, 2, lda=1 << 30).route()['kernel'] == GENERIC
    assert pair(1000, 48, 2, ldb=(1 << 30) - 4).route()['kernel'] == PIPE and pair(1000, 48, 2, ldb=1 << 30).route()['kernel'] == GENERIC
    assert _sub(pair(top - 1, 48, 2).route(), kernel=PIPE, blocks=1536) and _sub(pair(top, 48, 2).route(), kernel=GENERIC, blocks=4096)
    # more than 64 KB of packed weights: four square layers at 64 (66 832 bytes)
    assert pair(1000, 64, 3).route()['kernel'] == PIPE and pair(1000, 64, 4).route()['lds_bytes'] == 66832 and pair(1000, 64, 4).route()['kernel'] == GENERIC


def test_pair_stage_with_out_index_and_no_dot_runs_the_generic_kernel():
    """The pipe kernel scatters scores only; a [P, N] block with out_index is the generic kernel's."""
    for W, depth in ((48, 1), (48, 2), (48, 3), (64, 1), (64, 2)):
        call = pair(1000, W, depth, dot=False, out_index=True)
        assert _both(Call(0, W, W, [W] * depth, sum_inputs=True, in_act='relu', ids=True, out_index=True)) == 0
        assert _sub(call.route(), kernel=GENERIC, maxt=W // 16, full=True, am=1, has_dot=False, scatter=False, split=False,
                    lds_bytes=4 * cr.pack_floats([W] * (depth + 1)))
        assert pair(1000, W, depth, dot=False).route()['kernel'] == PIPE and pair(1000, W, depth, out_index=True).route()['kernel'] == PIPE


@pytest.mark.parametrize('W,depth,packed,frags,split', [(64, 1, 16912, 24576, True), (64, 2, 33552, 49152, False), (64, 3, 50192, 73728, False),
                                                        (48, 1, 9616, 18432, True), (48, 2, 19024, 36864, True), (48, 3, 28432, 55296, False),
                                                        (48, 4, 37840, 73728, False)])
def test_split_depth_thresholds(W, depth, packed, frags, split):
    """64-wide pair stages leave the split products at two square layers (33 552 + 49 152 = 82 704 bytes > 64 KB; one layer:
    16 912 + 24 576 = 41 488), 48-wide ones at three (28 432 + 55 296 = 83 728; two layers: 19 024 + 36 864 = 55 888).
    Exact byte counts from the pack layout: fragments are layers x maxt x ceil(maxt / 2) x 3 KB."""
    dims = [W] * (depth + 1) + [1]
    floats = cr.pack_floats(dims)
    maxt = W // 16
    assert 4 * floats == packed and depth * maxt * ((maxt + 1) // 2) * 3 * 1024 == frags
    r = pair(1000, W, depth).route()
    assert (packed + frags <= 65536) == split
    split = split and not F32_ONLY
    assert r['kernel'] == PIPE and r['split'] == split
    assert r['lds_bytes'] == (packed + frags if split else packed)
    r = pair(1000, W, depth, dot=False).route()                                                                         # without the 1-unit layer
    nd = 4 * cr.pack_floats([W] * (depth + 1))
    assert nd == packed - 4 * (W + 4) and r['split'] == split and r['lds_bytes'] == (nd + frags if split else nd)


def test_split_byte_counts_named_in_the_design():
    want = (41488, 55888) if not F32_ONLY else (16912, 19024)
    assert (pair(1000, 64, 1).route()['lds_bytes'], pair(1000, 48, 2).route()['lds_bytes']) == want
    assert 33552 + 49152 == 82704 and 28432 + 55296 == 83728


def test_pair_mfma_switch_is_read_once_in_a_fresh_process():
    """AMAR_PAIR_MFMA=f32 in a child: the route reports the f32 instruction for shapes that split here.  Host only: no GPU call."""
    script = ("import ctypes, sys; sys.path.insert(0, {!r})\n"
              "from tests.test_chain_route_cpu import pair\n"
              "print(*[int(pair(1000, W, d).route()['split']) for W, d in ((48, 2), (64, 1))], int(pair(1000, 48, 2).route()['lds_bytes']))\n").format(ROOT)
    env = dict(os.environ, AMAR_PAIR_MFMA='f32')
    out = subprocess.run([sys.executable, '-c', script], env=env, cwd=ROOT, check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ['0', '0', '19024']
    if not F32_ONLY:
        assert pair(1000, 48, 2).route()['split'] and pair(1000, 64, 1).route()['split']


# ---- the entity-tower kernel --------------------------------------------------------------------------------------------------------------
SHAPES = [([24, 24, 24, 48], (2, 2, 2, 3)), ([48, 48, 48, 64], (3, 3, 3, 4)), ([24, 24, 24], (2, 2, 2)), ([8, 24, 24, 48], (1, 2, 2, 3)),
          ([16, 48, 48, 64], (1, 3, 3, 4)), ([48, 48, 48], (3, 3, 3))]


@pytest.mark.parametrize('dims,tiles', SHAPES, ids=lambda v: '-'.join(map(str, v)))
def test_rows_shapes(dims, tiles):
    n = len(dims) - 1
    shape = capi.chain_shape(*tiles)
    assert shape == capi.chain_shape(*tiles) == n | sum(t << (3 * (j + 1)) for j, t in enumerate(tiles))
    for ids in (False, True):
        assert _sub(Call(1000, dims[0], 0, dims[1:], ids=ids).route(), kernel=ROWS, shape=shape, lastlin=False, seg=False, am=1, blocks=8, threads=256,
                    lds_bytes=4 * cr.pack_floats(dims))
        assert _sub(Call(1000, dims[0], 0, dims[1:], ['relu'] * (n - 1) + [None], ids=ids).route(), kernel=ROWS, shape=shape, lastlin=True, am=2)
    ragged = [16 * (t - 1) + 4 for t in tiles]                                                                         # same tile counts, barely
    assert [cr.tiles16(w) for w in ragged] == list(tiles) and Call(1000, ragged[0], 0, ragged[1:]).route()['shape'] == shape
    # near misses: an activation that is not ReLU, a second table, an output index, a tile more or less, a layer more or less
    assert Call(1000, dims[0], 0, dims[1:], [None] + ['relu'] * (n - 1)).route()['kernel'] == GENERIC
    assert Call(1000, dims[0], 0, dims[1:], ['relu'] * (n - 1) + ['sigmoid']).route()['kernel'] == GENERIC
    assert Call(1000, dims[0], 4, [dims[1] + 4] + dims[2:]).route()['kernel'] == GENERIC
    assert Call(1000, dims[0], 0, dims[1:], out_index=True).route()['kernel'] == GENERIC
    assert Call(1000, dims[0], 0, dims[1:] + [1], ['relu'] * n + ['sigmoid']).route()['kernel'] == GENERIC
    for j in range(n + 1):
        for delta in (-16, 16):
            near = [w + (delta if k == j else 0) for k, w in enumerate(dims)]
            if near[j] < 4 or (near in [d for d, _ in SHAPES]):
                continue
            r = Call(1000, near[0], 0, near[1:]).route()
            assert _sub(r, kernel=GENERIC, shape=0, lastlin=False, seg=False), near
    assert Call(1000, dims[0], 0, dims[1:] + [dims[-1]]).route()['kernel'] == GENERIC
    assert Call(1000, dims[0], 0, dims[1:-1]).route()['kernel'] == (ROWS if dims[:-1] in [d for d, _ in SHAPES] else GENERIC)
    # 32-bit row bytes and positions
    top = (1 << 30) - (4 << 20)
    assert Call(1000, dims[0], 0, dims[1:], lda=1 << 30).route()['kernel'] == GENERIC and Call(1000, dims[0], 0, dims[1:], lda=(1 << 30) - 4).route()['kernel'] == ROWS
    assert _sub(Call(top - 1, dims[0], 0, dims[1:]).route(), kernel=ROWS, blocks=1024) and _sub(Call(top, dims[0], 0, dims[1:]).route(), kernel=GENERIC, blocks=4096)


def test_rows_needs_at_most_three_layers():
    assert Call(1000, 24, 0, [24, 24, 24, 48]).route()['kernel'] == GENERIC and Call(1000, 48, 0, [48, 48, 48]).route()['kernel'] == GENERIC
    assert Call(1000, 24, 0, [24]).route()['kernel'] == GENERIC and Call(1000, 64, 0, [64, 64]).route()['kernel'] == GENERIC


def test_segments_route():
    shape = capi.chain_shape(2, 2, 2, 3)
    r = Seg(1000, [8, 8, 8], [24, 24, 48], ['relu', 'relu', None]).route()
    assert _sub(r, kernel=ROWS, shape=shape, lastlin=True, seg=True, am=2, blocks=8, lds_bytes=4 * cr.pack_floats([24, 24, 24, 48]))
    assert _sub(Seg(1000, [8, 12], [24, 24, 40], ids=True).route(), kernel=ROWS, shape=shape, lastlin=False, seg=True)
    assert _sub(Seg(1000, [24], [24, 24]).route(), kernel=ROWS, shape=capi.chain_shape(2, 2, 2), seg=True)
    assert _sub(Seg(200000, [16, 16, 16], [48, 48, 64]).route(), kernel=ROWS, shape=capi.chain_shape(3, 3, 3, 4), seg=True, blocks=1024)
    # no kernel for the shape: the caller assembles the table
    for case in (Seg(1000, [32, 32, 32], [96, 48, 64]), Seg(1000, [8, 8, 8], [24, 24, 24, 48]), Seg(1000, [8, 8, 8], [24, 24], [None, 'relu']),
                 Seg(1000, [8, 8, 8], [24, 24, 1], ['relu', 'relu', 'sigmoid']), Seg(1000, [64, 64], [64, 64]), Seg((1 << 30) - (4 << 20), [8, 8, 8], [24, 24])):
        assert _both(case) == EUNSUPPORTED
    assert _both(Seg(0, [32, 32, 32], [96, 48, 64])) == 0                                                              # (an empty batch is not refused)
    # the sum of the widths
    assert _both(Seg(1000, [64, 64, 4], [24, 24])) == EUNSUPPORTED and Seg(1000, [64, 64], [24, 24]).route(code=True) == EUNSUPPORTED
    assert Seg(1000, [4] * 8, [24, 24]).route()['kernel'] == ROWS and Seg(1000, [4] * 8, [24, 24]).route()['seg']
    # widths, leading dimensions, alignment, counts
    ok = Seg(0, [8, 8, 8], [24, 24])
    assert _both(ok) == 0 and ok.route()['blocks'] == 0
    assert _both(Seg(0, [8, 6, 10], [24, 24])) == EINVAL and _both(Seg(0, [8, 0, 16], [24, 24])) == EINVAL
    assert _both(Seg(0, [8, 8, 8], [24, 24], seg_ld=[8, 7, 8])) == EINVAL and _both(Seg(0, [8, 8, 8], [24, 24], seg_ld=[8, 10, 8])) == EINVAL
    assert _both(Seg(0, [8, 8, 8], [24, 24], seg_ld=[8, 4, 8])) == EINVAL and _both(Seg(0, [8, 8, 8], [24, 24], seg_ld=[8, 1 << 30, 8])) == EINVAL
    assert _both(Seg(0, [8, 8, 8], [24, 24], seg_ld=[8, (1 << 30) - 4, 8])) == 0
    assert _both(Seg(0, [8, 8, 8], [24, 24], seg=[_addr(10), _addr(11, 8), _addr(12)])) == EINVAL
    assert _both(Seg(0, [8, 8, 8], [24, 24], seg=[_addr(10), None, _addr(12)])) == EINVAL
    assert _both(Seg(0, [8, 8, 8], [24, 24], n_seg=0)) == EINVAL and _both(Seg(0, [4] * 9, [36, 24])) == EINVAL
    for name in ('seg', 'seg_ld', 'seg_width', 'wpack', 'dims', 'acts', 'out'):
        case = Seg(0, [8, 8, 8], [24, 24])
        case.v[name] = None
        assert _both(case) == EINVAL, name
    assert _both(Seg(0, [8, 8, 8], [20, 24])) == 0 and _both(Seg(0, [8, 8, 8], [24, 24], dims=[20, 24, 24])) == EINVAL   # dims[0] is the sum
    assert capi.load().amar_chain_segments_route(*ok.args(), None) == EINVAL


# ---- grid caps, LDS, no rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make,cap', [(lambda P: Call(P, 24, 24, [48, 48, 1], ids=True), 4096), (lambda P: pair(P, 48, 2), 1536),
                                      (lambda P: Call(P, 24, 0, [24, 24]), 1024)], ids=['generic', 'pipe', 'rows'])
def test_blocks_at_the_grid_caps(make, cap):
    for P, blocks in ((1, 1), (128, 1), (129, 2), (cap * 128 - 1, cap), (cap * 128, cap), (cap * 128 + 1, cap), (cap * 128 + 45, cap), (3 * cap * 128, cap)):
        r = make(P).route()
        assert r['blocks'] == blocks and r['threads'] == 256, (P, r)
    assert make(0).route()['blocks'] == 0 and make(0).launch() == 0


def test_lds_bytes_is_the_packed_blob():
    for Da, Db, units in ((24, 24, [48, 48, 1]), (16, 8, [30, 1]), (4, 0, [20]), (128, 0, [128, 64]), (96, 0, [96, 48]), (24, 0, [24, 24, 48])):
        assert Call(77, Da, Db, units).route()['lds_bytes'] == 4 * cr.pack_floats([Da + Db] + units)


# ---- every refusal, on the route and on the launcher ------------------------------------------------------------------------------------------
def test_einval_of_every_argument_check():
    ok = lambda **e: _edited(Call(100, 24, 24, [48, 48, 1], ['relu', 'relu', 'sigmoid'], ids=True), **e)              # noqa: E731
    assert _both(ok()) != EINVAL and ok().route(code=True) == 0
    for name in ('A', 'wpack', 'dims', 'acts', 'out'):
        case = ok()
        case.v[name] = None
        assert _both(case) == EINVAL, name
    assert _both(ok(P=-1)) == EINVAL
    assert _both(ok(Da=0, dims=[24, 48, 48, 1])) == EINVAL and _both(ok(Da=22, Db=26)) == EINVAL and _both(ok(Da=26, Db=22)) == EINVAL
    assert _both(ok(Db=-4, dims=[20, 48, 48, 1])) == EINVAL
    assert _both(ok(lda=26)) == EINVAL and _both(ok(lda=20)) == EINVAL and _both(ok(ldb=26)) == EINVAL and _both(ok(ldb=20)) == EINVAL
    assert _both(ok(A=_addr(0, 8))) == EINVAL and _both(ok(B=_addr(2, 4))) == EINVAL and _both(ok(wpack=_addr(4, 8))) == EINVAL
    assert _both(ok(B=None)) == EINVAL
    assert ok(ids_a=_addr(1, 4), ids_b=_addr(3, 12), out=_addr(5, 4)).route(code=True) == 0                            # ids and scores are 4-byte values
    assert _both(ok(in_act=3)) == EINVAL and _both(ok(in_act=-1)) == EINVAL
    assert _both(ok(n_layers=0)) == EINVAL and _both(Call(100, 16, 0, [16] * 9)) == EINVAL and Call(100, 16, 0, [16] * 8).route(code=True) == 0
    assert _both(ok(dims=[44, 48, 48, 1])) == EINVAL and _both(ok(dims=[48, 0, 48, 1])) == EINVAL and _both(ok(dims=[48, 48, -1, 1])) == EINVAL
    assert _both(ok(acts=[1, 3, 2])) == EINVAL and _both(ok(acts=[-1, 1, 2])) == EINVAL
    assert _both(ok(ldo=0)) == EINVAL and ok(ldo=1).route(code=True) == 0                                              # scores: any positive stride
    # sum_inputs: equal widths, a second table, dims[0] the common width
    s = lambda **e: _edited(Call(100, 24, 24, [48, 1], sum_inputs=True, in_act='relu'), **e)                          # noqa: E731
    assert s().route(code=True) == 0 and _both(s(Db=20)) == EINVAL and _both(s(B=None)) == EINVAL and _both(s(dims=[48, 48, 1])) == EINVAL
    # a vector output: 16-byte rows
    v = lambda **e: _edited(Call(100, 24, 0, [24, 24]), **e)                                                           # noqa: E731
    assert v().route(code=True) == 0
    assert _both(v(ldo=20)) == EINVAL and _both(v(ldo=26)) == EINVAL and _both(v(out=_addr(5, 8))) == EINVAL
    assert _both(Call(100, 24, 0, [24, 22])) == EINVAL and _both(Call(100, 24, 0, [24, 1, 1], ldo=4)) != EINVAL
    assert _both(Call(100, 24, 0, [1])) == EINVAL                                                                      # one 1-unit layer is a [P, 1] block: no multiple of 4
    assert capi.load().amar_chain_route(*ok().args(), None) == EINVAL


# ---- capi.chain_supported promises no more than the route gives ---------------------------------------------------------------------------------
def test_chain_supported_implies_a_route():
    widths = (4, 20, 30, 48, 64, 100, 128, 132)
    n = 0
    for in_a in (4, 6, 24, 64, 128):
        for in_b, summed in ((0, False), (8, False), (in_a, True), (64, False)):
            for hidden in ([], [30], [48, 128], [132], [64] * 7, [64] * 8):
                for last in (1,) + widths:
                    dims = [in_a if summed else in_a + in_b] + hidden + [last]
                    if capi.chain_supported(dims, in_a, in_b, summed):
                        code = Call(100, in_a, in_b, dims[1:], sum_inputs=summed, in_act='relu').route(code=True)
                        assert code == 0, dims
                        n += 1
    assert n > 100
    # the packed blob must fit 150 KB: three 128 x 128 layers (198 144 bytes) do not, two do
    assert not capi.chain_supported([128, 128, 128, 128], 128) and not capi.chain_supported([128, 128, 128, 128], 64, 64)
    assert capi.chain_supported([128, 128, 128], 128) and capi.chain_supported([128, 128, 128, 1], 128)
    assert not capi.chain_supported([128] + [64] * 7 + [128], 128) and capi.chain_supported([64] * 9, 64)
    assert capi.chain_supported([24, 30, 1], 16, 8) and not capi.chain_supported([24, 30, 2], 16, 8) and not capi.chain_supported([24, 1], 16, 8)
    assert not capi.chain_supported([132, 8], 132) and not capi.chain_supported([24, 24], 22, 2) and not capi.chain_supported([8] * 10, 8)


# ---- the GPU cases, as far as a CPU can check them -------------------------------------------------------------------------------------------
def _case_route(case, P):
    """The route of a tests/chain_ref.py case at made-up addresses (tables with padded leading dimensions where the case pads them)."""
    pad = 8 if case.padded else 0
    if case.seg:
        return Seg(P, case.seg, case.units, case.acts, ids=case.ids).route()
    return Call(P, case.Da, case.Db, case.units, case.acts, sum_inputs=case.sum_inputs, in_act=case.in_act, ids=case.ids, out_index=case.out_index,
                lda=case.Da + pad, ldb=case.Db + pad if case.Db else 0).route()


ALL_CASES = cr.all_cases()


def test_case_names_are_unique_and_cover_every_instantiation():
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
    generic = {(c.expect['maxt'], c.expect['full'], c.expect['am']) for c in ALL_CASES if c.expect['kernel'] == GENERIC}
    assert generic == {(m, f, a) for m in (3, 4, 8) for f in (True, False) for a in (0, 1, 2)}
    pipe = {(c.expect['maxt'], c.expect['scatter'], c.expect['split']) for c in ALL_CASES if c.expect['kernel'] == PIPE}
    assert pipe == {(m, s, p) for m in (3, 4) for s in (True, False) for p in (True, False)}
    rows = {(c.expect['shape'], c.expect['lastlin'], c.expect['seg']) for c in ALL_CASES if c.expect['kernel'] == ROWS}
    shapes = [capi.chain_shape(*t) for _, t in SHAPES]
    assert {(s, l, False) for s in shapes for l in (True, False)} <= rows
    assert {l for _, l, g in rows if g} == {True, False} and len({s for s, _, g in rows if g}) >= 2
    # each generic form: with and without a 1-unit layer (am 2 has none), with and without ids, one table and two
    for key in generic:
        mine = [c for c in ALL_CASES if c.expect['kernel'] == GENERIC and (c.expect['maxt'], c.expect['full'], c.expect['am']) == key]
        assert {c.ids for c in mine} == {True, False} and {c.Db > 0 for c in mine} == {True, False}, key
        assert {c.has_dot for c in mine} == ({False} if key[2] == 2 else {True, False}), key
    dots = {c.acts[-1] for c in ALL_CASES if c.has_dot and c.expect['kernel'] == GENERIC}
    assert dots == {'sigmoid', None, 'relu'}
    am0 = [c for c in ALL_CASES if c.expect['kernel'] == GENERIC and c.expect['am'] == 0]
    assert any('sigmoid' in c.acts[:-1] for c in am0) and any(None in c.acts[:-1] for c in am0)
    assert {c.in_act for c in am0 if c.sum_inputs} == {None, 'sigmoid'}


@pytest.mark.parametrize('case', ALL_CASES, ids=repr)
def test_gpu_case_routes_as_it_says(case):
    expect = dict(case.expect, split=False) if F32_ONLY and 'split' in case.expect else case.expect
    for P in case.Ps:
        r = _case_route(case, P)
        assert _sub(r, **expect), (case, P)
        assert r['blocks'] == min(-(-P // 128), {GENERIC: 4096, PIPE: 1536, ROWS: 1024}[r['kernel']])
    assert capi.chain_supported(case.dims, case.Da, case.Db, case.sum_inputs)


@pytest.mark.parametrize('case', ALL_CASES, ids=repr)
def test_reference_bound_holds_for_the_float32_numpy_evaluation(case):
    """The bound is satisfiable: numpy's float32 evaluation of the case stays inside it (with the f32 constant c_K = K + 2 also where the
    device runs the split products, whose bound is wider), and every sigmoid evaluation term is below 1e-6."""
    d = case.draw()
    P = min(max(case.Ps), 20000)
    terms = []
    want, bound = case.reference(d, P, split=False, terms=terms)
    got = case.reference_f32(d, P)
    cr.assert_within(got, want, bound, repr(case))
    assert want.shape == ((P,) if case.has_dot else (P, case.dims[-1])) and (bound >= 0).all()
    assert all(0 < t < cr.SIGMOID_LIMIT for t in terms) and len(terms) == (case.acts + [case.in_act if case.sum_inputs else None]).count('sigmoid')
    wide = case.reference(d, P, split=True)[1]
    assert (wide >= bound).all()


def test_sigmoid_terms_stay_below_the_limit():
    """The worst float32 numpy sigmoid error over the pre-activations of all cases (each at its smallest and its largest P below 20 000),
    times the margin, is below 1e-6 (8.73e-8 x 4 where this was written; the figure depends on numpy's exp, the limit does not)."""
    worst = 0.0
    for case in ALL_CASES:
        if 'sigmoid' in case.acts or (case.sum_inputs and case.in_act == 'sigmoid'):
            d = case.draw()
            for P in (min(case.Ps), min(max(case.Ps), 20000)):
                terms = []
                case.reference(d, P, terms=terms)
                worst = max(worst, max(terms) / cr.SIGMOID_MARGIN)
    print('worst float32 numpy sigmoid error: {:.3e}'.format(worst))
    assert 0 < cr.SIGMOID_MARGIN * worst < cr.SIGMOID_LIMIT
