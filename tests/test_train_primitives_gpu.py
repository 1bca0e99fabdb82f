"""The separate training kernels of csrc/amar_train.hip at the edges of their launchers (pytest -m gpu): amar_scatter_add_rows_f32,
amar_wgrad_f32 (both routes), amar_act_bwd_f32, amar_add_inplace_f32, amar_row_affine_f32, amar_l2norm_fwd_f32 / _bwd_f32 and
amar_transpose_f32.  Every case asserts the route it means to run (amar_wgrad_route / amar_scatter_add_rows_route: the launchers ask
the same functions), compares EVERY element with the float64 reference of tests/train_primitives_ref.py inside the bound derived there
(or to the bit, where the kernel promises bits), and writes into buffers that are wider than the result and pre-filled with a sentinel,
which must still be there afterwards."""
import numpy as np
import pytest
import torch

from tests import train_primitives_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = np.float32(-12345.625)
U = ref.U


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guard:
    """A [rows, cols] output inside a wider, taller buffer full of SENT: `view` is what the kernel gets, intact() says that nothing
    outside it was written.  flat=True: a contiguous [rows, cols] block with a margin before and after (outputs that must be contiguous)."""
    def __init__(self, rows, cols, flat=False, left=3, right=2, fill=None):
        if flat:
            self.full = torch.full((rows * cols + 64,), float(SENT), device=DEV)
            self.view = self.full[32:32 + rows * cols].view(rows, cols)
        else:
            self.full = torch.full((rows + 2, left + cols + right), float(SENT), device=DEV)
            self.view = self.full[1:1 + rows, left:left + cols]
        if fill is not None:
            self.view.copy_(_t(fill))

    def get(self):
        return self.view.cpu().numpy()

    def intact(self):
        self.view.fill_(float(SENT))
        return bool((self.full == float(SENT)).all())


def strided(a, left=1, right=2):
    """`a` on the device as a column slice of a wider matrix (leading dimension cols + left + right; left = 1: a base that is not
    16-byte aligned)."""
    wide = torch.full((a.shape[0], a.shape[1] + left + right), 7.5, device=DEV)
    wide[:, left:left + a.shape[1]] = _t(a)
    return wide[:, left:left + a.shape[1]]


# ---- scatter_add_rows ---------------------------------------------------------------------------------------------------------------
def _scatter_case(hip, ids, W, n_rows, seed, base=0, lds_extra=0, kernel='owner'):
    """One call on `ids` into a random non-zero destination [n_rows, W] that is a column slice; returns (got, src, dst0, guard)."""
    rng = np.random.default_rng(seed)
    M = len(ids)
    src = rng.standard_normal((M, W)).astype(np.float32)
    dst0 = rng.standard_normal((n_rows, W)).astype(np.float32)
    src_d = strided(src, left=1, right=lds_extra - 1) if lds_extra else _t(src)
    assert hip._ld(src_d, 'src') == W + lds_extra or M == 1
    route = hip.scatter_add_rows_route(M, W)
    assert route['kernel'] == kernel
    g = Guard(n_rows, W, fill=dst0)
    hip.scatter_add_rows(src_d, _t(ids), g.view, base=base)
    return g.get(), src, dst0, g, route


def _owner_checks(hip, ids, W, n_rows, seed, base=0, lds_extra=0):
    got, src, dst0, g, route = _scatter_case(hip, ids, W, n_rows, seed, base, lds_extra)
    assert np.array_equal(got, ref.scatter_sequential_f32(src, ids, base, dst0)), "owner kernel: the sequential float32 sum, bit for bit"
    want, bound = ref.scatter_ref(src, ids, base, dst0)
    assert np.all(np.abs(got - want) <= bound)
    assert g.intact()
    again = _scatter_case(hip, ids, W, n_rows, seed, base, lds_extra)[0]
    assert np.array_equal(got, again), "owner kernel: the same bits on a second call"
    return route


# every M at W = 12 and every W at M = 4 097 (a sparse cross).  M: one position; 63 / 64 / 65 around one ballot of 64 ids; 4 096 = the last
# list with one position per wavefront, 4 097 = the first with two (p += gridDim.x * 4); 8 192 = the longest list the owner kernel takes.
# W: one column; 64 / 65 around one trip of the column loop (c0 += 64); 130 = three trips, the last with two live lanes.
OWNER_SHAPES = [(M, 12) for M in (1, 63, 64, 65, 4096, 4097, 8192)] + [(4097, W) for W in (1, 64, 65, 130)]


@pytest.mark.parametrize('M,W', OWNER_SHAPES)
def test_scatter_owner_random_ids_strided_with_base(hip, M, W):
    """Random ids with many repeats (M / 8 + 3 destination rows), strided src (lds = W + 3), dst a column slice holding random values
    (the kernel adds), base = 5."""
    rng = np.random.default_rng(M * 131 + W)
    n_rows = M // 8 + 3
    ids = (rng.integers(0, n_rows, M) + 5).astype(np.int32)
    route = _owner_checks(hip, ids, W, n_rows, seed=M + W, base=5, lds_extra=3)
    assert route['positions_per_wave'] == (2 if M > 4096 else 1) and route['blocks'] == min(-(-M // 4), 1024) and route['lds_bytes'] == 4 * M


@pytest.mark.parametrize('M', [130, 200, 4097])
def test_scatter_owner_duplicates_across_ballot_boundaries(hip, M):
    """The ownership ballot walks 64 ids at a time and the walk over later positions starts at (p + 1) & ~63.  First list: one id at
    positions {0, 63, 64, 127, 128, M - 1} — later positions on both sides of two word boundaries, and positions 63 / 64 / 127 / 128 must
    each find an EARLIER one (63 and 127 in their own word, 64 and 128 only in a previous word).  Second list: an id that first appears at
    63 (its walk starts at word 64: every later position counts) and one that first appears at 64 (its walk starts in its own word, where
    only q > p may count; nothing earlier in any word)."""
    ids = np.arange(10, 10 + M, dtype=np.int32)                        # all distinct, then the constructed repeats
    ids[[0, 63, 64, 127, 128, M - 1]] = 3
    _owner_checks(hip, ids, 12, M + 10, seed=M)
    ids = np.arange(10, 10 + M, dtype=np.int32)
    ids[[63, 65, 128, M - 1]] = 4
    ids[[64, 66, 127]] = 5
    _owner_checks(hip, ids, 12, M + 10, seed=M + 1)


def test_scatter_owner_all_equal_and_all_distinct(hip):
    """All 8 192 ids equal: one owner (position 0) adds 8 191 rows in order, every other wavefront finds an earlier position in its first
    ballot.  All distinct: every position owns its row and no ballot finds anything."""
    _owner_checks(hip, np.full(8192, 2, np.int32), 12, 4, seed=1)
    _owner_checks(hip, np.random.default_rng(2).permutation(8192).astype(np.int32), 12, 8192, seed=2)
    _owner_checks(hip, np.random.default_rng(3).permutation(4097).astype(np.int32), 65, 4097, seed=3)


def test_scatter_atomic_same_data_as_owner(hip):
    """The 8 192 / 8 193 pair on literally the same rows: src[:8192] of the atomic call is the owner call's src, so outside the row the
    8 193rd position adds to, the two results are sums of the same terms and differ by at most the sum of their bounds."""
    rng = np.random.default_rng(77)
    W, n_rows = 12, 700
    ids = rng.integers(0, n_rows, 8193).astype(np.int32)
    src = rng.standard_normal((8193, W)).astype(np.float32)
    dst0 = rng.standard_normal((n_rows, W)).astype(np.float32)
    assert hip.scatter_add_rows_route(8192, W)['kernel'] == 'owner' and hip.scatter_add_rows_route(8193, W)['kernel'] == 'atomic'
    g_o, g_a = Guard(n_rows, W, fill=dst0), Guard(n_rows, W, fill=dst0)
    src_d = strided(src, left=1, right=2)
    hip.scatter_add_rows(src_d[:8192], _t(ids[:8192]), g_o.view)
    hip.scatter_add_rows(src_d, _t(ids), g_a.view)
    got_o, got_a = g_o.get(), g_a.get()
    want_o, bound_o = ref.scatter_ref(src[:8192], ids[:8192], 0, dst0)
    want_a, bound_a = ref.scatter_ref(src, ids, 0, dst0)
    assert np.array_equal(got_o, ref.scatter_sequential_f32(src[:8192], ids[:8192], 0, dst0))
    assert np.all(np.abs(got_a - want_a) <= bound_a)
    other = np.arange(n_rows) != ids[8192]
    assert np.all(np.abs(got_a[other] - got_o[other]) <= bound_a[other] + bound_o[other])
    assert np.all(np.abs(got_a[~other] - (want_o[~other] + src[8192].astype(np.float64))) <= bound_a[~other])
    assert g_o.intact() and g_a.intact()


def test_scatter_atomic_second_grid_trip(hip):
    """M = 262 145, W = 8: 2 097 160 elements for a grid capped at 8 192 x 256 = 2 097 152 threads — the first eight threads take a
    second trip of the grid-stride loop (the last row of src)."""
    rng = np.random.default_rng(5)
    M, W, n_rows = 262145, 8, 5000
    route = hip.scatter_add_rows_route(M, W)
    assert route['kernel'] == 'atomic' and route['blocks'] == 8192 and M * W > 8192 * 256
    ids = rng.integers(0, n_rows, M).astype(np.int32)
    ids[-1] = 4999
    src = rng.standard_normal((M, W)).astype(np.float32)
    src[-1] = 1000.0                                                   # the second trip's row cannot hide inside the bound
    dst0 = rng.standard_normal((n_rows, W)).astype(np.float32)
    g = Guard(n_rows, W, fill=dst0)
    hip.scatter_add_rows(_t(src), _t(ids), g.view)
    want, bound = ref.scatter_ref(src, ids, 0, dst0)
    assert np.all(bound[4999] < 1.0) and np.all(np.abs(g.get() - want) <= bound)
    assert g.intact()


def test_scatter_empty_list_writes_nothing(hip):
    """M = 0 with real addresses (the C entry point: a zero-row torch view has no address to hand over): OK, nothing launched."""
    g = Guard(7, 5, fill=np.ones((7, 5), np.float32))
    src, ids = torch.full((4, 5), 3.0, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    assert hip.scatter_add_rows_route(0, 5)['blocks'] == 0
    code = hip.load().amar_scatter_add_rows_f32(src.data_ptr(), 5, ids.data_ptr(), 0, g.view.data_ptr(), g.view.stride(0), 0, 5, hip._stream())
    torch.cuda.synchronize()
    assert code == 0 and np.array_equal(g.get(), np.ones((7, 5), np.float32)) and g.intact()


# ---- wgrad --------------------------------------------------------------------------------------------------------------------------
def _wgrad_outputs(hip, x_d, dz_d, K, N, want_dw, want_db):
    gw = Guard(K, N, flat=True) if want_dw else None
    gb = Guard(1, N, flat=True) if want_db else None
    hip.wgrad(x_d if want_dw else None, dz_d, gw.view if gw else None, gb.view.view(N) if gb else None)
    out = (gw.get() if gw else None, gb.get()[0] if gb else None)
    assert (gw is None or gw.intact()) and (gb is None or gb.intact())
    return out


# (1, 5, 3): one row in a 128-row chunk, one thread column of a tile.  (64, 17, 33): one full stage of 64 rows; 17 = a second K tile with
# one live column, 33 = a third N tile with one.  (65, 1, 24): a second stage with one row; K = 1.  (1300, 24, 1): N = 1, eleven chunks,
# the last with 20 rows.  (8256, 40, 24): the first M with 192-row chunks (43 chunks).  (28736, 16, 16): the first M with 512-row chunks
# (57 chunks, the last with 64 rows).  (16385, 128, 128): the first M past the matrix-instruction route on a wide layer (256-row chunks,
# 65 of them, 8 x 8 tiles).
PARTIAL_SHAPES = [(1, 5, 3, 128), (64, 17, 33, 128), (65, 1, 24, 128), (1300, 24, 1, 128), (8256, 40, 24, 192), (28736, 16, 16, 512),
                  (16385, 128, 128, 256)]


def _wgrad_partial_case(hip, M, K, N, rows, x_d, dz_d, x, dz):
    for dw_given, db_given in ((True, True), (True, False), (False, True)):
        r = hip.wgrad_route(x_d if dw_given else None, dz_d, torch.empty((K, N), device=DEV) if dw_given else None,
                            torch.empty(N, device=DEV) if db_given else None)
        assert r['kernel'] == 'partial' and r['wg_rows'] == rows and r['chunks'] == -(-M // rows)
        assert (r['grid_k'], r['grid_n']) == (-(-K // 16) if dw_given else 1, -(-N // 16))
    want_w, want_b, bound_w, bound_b = ref.wgrad_ref(x, dz)
    dw, db = _wgrad_outputs(hip, x_d, dz_d, K, N, True, True)
    assert np.all(np.abs(dw - want_w) <= bound_w), float((np.abs(dw - want_w) / bound_w).max())
    assert np.all(np.abs(db - want_b) <= bound_b), float((np.abs(db - want_b) / bound_b).max())
    dw_only = _wgrad_outputs(hip, x_d, dz_d, K, N, True, False)[0]
    db_only = _wgrad_outputs(hip, None, dz_d, K, N, False, True)[1]
    assert np.array_equal(dw, dw_only) and np.array_equal(db, db_only), "the three forms of the call: the same bits"
    dw2, db2 = _wgrad_outputs(hip, x_d, dz_d, K, N, True, True)
    assert np.array_equal(dw, dw2) and np.array_equal(db, db2), "two-stage reduction: the same bits on repetition"


@pytest.mark.parametrize('M,K,N,rows', PARTIAL_SHAPES)
def test_wgrad_partial_route(hip, M, K, N, rows):
    """Strided operands with unaligned bases: ldx = K + 3, ldz = N + 1."""
    rng = np.random.default_rng(M + 7 * K + 11 * N)
    x, dz = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    x_d, dz_d = strided(x, 1, 2), strided(dz, 1, 0)
    if M > 1:
        assert x_d.stride(0) == K + 3 and dz_d.stride(0) == N + 1
    _wgrad_partial_case(hip, M, K, N, rows, x_d, dz_d, x, dz)


def test_wgrad_partial_route_fifteen_tiles_aligned(hip):
    """(4097, 96, 160) with aligned operands and leading dimensions that are multiples of 4: everything the matrix-instruction route
    asks for except the tile count, 3 x 5 = 15 tiles of 32 x 32 — the partial route, 33 chunks of 128 rows, the last with one row."""
    M, K, N = 4097, 96, 160
    rng = np.random.default_rng(15)
    x, dz = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    x_d, dz_d = strided(x, 4, 4), strided(dz, 4, 0)
    assert x_d.data_ptr() % 16 == 0 and dz_d.data_ptr() % 16 == 0 and x_d.stride(0) == K + 8 and dz_d.stride(0) == N + 4
    _wgrad_partial_case(hip, M, K, N, 128, x_d, dz_d, x, dz)


def test_wgrad_column_x_as_linear_bwd_calls_it(hip):
    """training.py:_LinearReverse.linear_bwd(column_x=True): the [n] gradient of an attention vector as the [n, 1] product dz^T . x,
    wgrad(dz [M, n], x [M, 1], dw.view(n, 1), None) — K = n = 48, N = 1, ldz = 1."""
    M, n = 777, 48
    rng = np.random.default_rng(48)
    dz, x = rng.standard_normal((M, n)).astype(np.float32), rng.standard_normal((M, 1)).astype(np.float32)
    dz_d, x_d = strided(dz, 1, 2), _t(x).view(M).clone().view(M, 1)
    g = Guard(1, n, flat=True)
    dw = g.view.view(n)
    r = hip.wgrad_route(dz_d, x_d, dw.view(n, 1), None)
    assert r['kernel'] == 'partial' and (r['grid_k'], r['grid_n'], r['chunks']) == (3, 1, 7)
    hip.wgrad(dz_d, x_d, dw.view(n, 1), None)
    want, _, bound, _ = ref.wgrad_ref(dz, x)
    assert np.all(np.abs(g.get()[0] - want[:, 0]) <= bound[:, 0])
    assert g.intact()


# M = 1 / 255 / 256 / 257: a stage of 256 rows with one row, one row short, full, and a second stage with one row; 16 384: the last M of
# the route (64 stages).  (300, 132, 124): 5 x 4 tiles, the last in each direction partial (4 of 32 columns of X, 28 of 32 of dZ).
MFMA_SHAPES = [(1, 128, 128), (255, 128, 128), (256, 128, 128), (257, 128, 128), (16384, 128, 128), (300, 132, 124)]


@pytest.mark.parametrize('M,K,N', MFMA_SHAPES)
def test_wgrad_matrix_instruction_route(hip, M, K, N):
    """Strided aligned operands (ldx = K + 8, ldz = N + 4), with and without db, repeated with equal bits."""
    rng = np.random.default_rng(M + K + N)
    x, dz = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    x_d, dz_d = strided(x, 4, 4), strided(dz, 4, 0)
    for db_given in (True, False):
        r = hip.wgrad_route(x_d, dz_d, torch.empty((K, N), device=DEV), torch.empty(N, device=DEV) if db_given else None)
        assert r == dict(kernel='mfma', wg_rows=0, chunks=1, grid_k=-(-K // 32), grid_n=-(-N // 32), scratch_floats=0)
    want_w, want_b, bound_w, bound_b = ref.wgrad_ref(x, dz)
    dw, db = _wgrad_outputs(hip, x_d, dz_d, K, N, True, True)
    assert np.all(np.abs(dw - want_w) <= bound_w), float((np.abs(dw - want_w) / bound_w).max())
    assert np.all(np.abs(db - want_b) <= bound_b), float((np.abs(db - want_b) / bound_b).max())
    dw_only = _wgrad_outputs(hip, x_d, dz_d, K, N, True, False)[0]
    dw2, db2 = _wgrad_outputs(hip, x_d, dz_d, K, N, True, True)
    assert np.array_equal(dw, dw_only) and np.array_equal(dw, dw2) and np.array_equal(db, db2)


# ---- element-wise kernels -------------------------------------------------------------------------------------------------------------
# 65 537 x 32 = 2 097 184 elements for a grid capped at 8 192 x 256 = 2 097 152 threads: the first 32 threads take a second trip of
# the grid-stride loop, which is the last row.
BIG = (65537, 32)
SHAPES = [(1, 1), (300, 7), BIG]


@pytest.mark.parametrize('M,N', SHAPES)
def test_act_bwd(hip, M, N):
    assert (M * N > 8192 * 256) == ((M, N) == BIG)
    rng = np.random.default_rng(M + N)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    y = np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32)   # about half of it exactly +0
    y.flat[::7] = -0.0
    y.flat[1::7] = -1.5
    sig = (1 / (1 + np.exp(-rng.standard_normal((M, N)) * 4))).astype(np.float32)
    dy_d = strided(dy, 1, 2)
    for act, y_h in (('relu', y), ('sigmoid', sig), (None, y)):
        y_d = strided(y_h, 2, 1)
        g = Guard(M, N)
        hip.act_bwd(dy_d, y_d, g.view, act)
        got, want = g.get(), ref.act_bwd_ref(dy, y_h, act)
        if act == 'sigmoid':                                           # dy * y, 1 - y, their product: three roundings, < 4 u relative
            assert np.all(np.abs(got - want) <= 4 * U * np.abs(want))
        else:                                                          # relu: dy where y > 0 (not at +0, not at -0), else +0; none: a copy
            assert np.array_equal(got, want.astype(np.float32))
            assert act is None or not np.any(got[y_h <= 0])
        assert g.intact()
        # dZ aliasing dY (capi.act_bwd's contract; both pointers are __restrict__): the same bits
        alias = Guard(M, N, fill=dy)
        hip.act_bwd(alias.view, y_d, alias.view, act)
        assert np.array_equal(alias.get(), got) and alias.intact()


@pytest.mark.parametrize('M,W', SHAPES)
@pytest.mark.parametrize('scale', [1.0, 0.5, 0.3])
def test_add_inplace(hip, M, W, scale):
    """dst += scale * src is compiled to one fused multiply-add (v_fmac_f32 with the scale as its scalar operand; hipcc contracts by
    default and the kernel does not turn it off), so the expectation is fmaf(scale, src, dst): one rounding.  At scale 1 and 0.5 the
    product is exact and a separate multiply and add give the same bits; 0.3 tells the two apart."""
    rng = np.random.default_rng(M + W)
    dst0, src = rng.standard_normal((M, W)).astype(np.float32), rng.standard_normal((M, W)).astype(np.float32)
    g = Guard(M, W, fill=dst0)
    hip.add_inplace(g.view, strided(src, 1, 2), scale)
    want = ref.fma_f32(np.float32(scale), src, dst0)
    if scale != 0.3:
        assert np.array_equal(want, dst0 + np.float32(scale) * src)
    assert np.array_equal(g.get(), want)
    assert g.intact()


@pytest.mark.parametrize('M,W', SHAPES)
def test_row_affine(hip, M, W):
    """out = (a + b) * scale[row]: one addition and one multiplication, each within u / (1 + u) of its exact result — within 2 u of
    the float64 value, relative, per element (an exact zero where a + b cancels)."""
    rng = np.random.default_rng(M + W)
    a, b = rng.standard_normal((M, W)).astype(np.float32), rng.standard_normal((M, W)).astype(np.float32)
    b.flat[::5] = -a.flat[::5]
    sc = rng.uniform(0.1, 1, M).astype(np.float32)
    a_d, b_d, sc_d = strided(a, 1, 2), strided(b, 2, 3), _t(sc)
    for b_h, b_dev in ((b, b_d), (None, None)):
        want = ref.row_affine_ref(a, sc, b_h)
        g = Guard(M, W)
        hip.row_affine(a_d, sc_d, g.view, b=b_dev)
        got = g.get()
        assert np.all(np.abs(got - want) <= 2 * U * np.abs(want))
        assert g.intact()
        # out aliasing a (layers/graphsage_conv.py: the aggregate is scaled where it stands; both pointers are __restrict__)
        alias = Guard(M, W, fill=a)
        hip.row_affine(alias.view, sc_d, alias.view, b=b_dev)
        assert np.array_equal(alias.get(), got) and alias.intact()


# rsqrtf is an approximation, so these three bounds cannot be derived; they are TWICE the worst error measured with these inputs on an
# MI355X with the kernels as they were before this file existed (all of L2_CASES, both activations), each capped at what
# test_sage_training_kernels already held as a whole-array ratio:
#   inv  worst |got - ref| / ref                      measured 1.917e-7 (C = 64)               -> bound 3.834e-7  (cap 1e-6)
#   nrm  worst |got - ref| / |ref|                    measured 2.417e-7 (C = 64)               -> bound 4.834e-7  (cap 1e-6)
#   dz   worst |got - ref| / scale (l2norm_bwd_ref)   measured 4.871e-7 (C = 2, relu, 2 M rows) -> bound 9.742e-7  (cap 1e-5)
# (u = 2**-24 = 5.96e-8: the worst inv is 3.2 u, of which the 64-term sum of squares and the rsqrt approximation share.)
MEASURED_INV, MEASURED_NRM, MEASURED_DZ = 1.917e-7, 2.417e-7, 4.871e-7
L2_INV_BOUND, L2_NRM_BOUND, L2_DZ_BOUND = min(2 * MEASURED_INV, 1e-6), min(2 * MEASURED_NRM, 1e-6), min(2 * MEASURED_DZ, 1e-5)
# 2 097 153 rows for a grid capped at 2 097 152 threads (one row per thread): thread 0 takes a second trip, the last row
L2_CASES = [(300, 1), (300, 12), (300, 64), (2097153, 2)]


def l2_inputs(M, C):
    rng = np.random.default_rng(M + C)
    z, dy = rng.standard_normal((M, C)).astype(np.float32), rng.standard_normal((M, C)).astype(np.float32)
    z[5] = 0                                                           # zero rows: clamped, inv = 1e6, nrm = 0
    z[6] *= np.float32(1e-8)                                           # clamped and not zero: nrm = 1e6 z, linear
    if C > 1:
        z[7, C // 2] = 0                                               # one exact zero among non-zeros: the n > 0 mask at n = 0
        z[8, 0] = -0.0
    z[-1] = np.abs(z[-1]) + 1                                          # (the row of a second grid trip: nothing about it is small)
    return z, dy


def l2_run(hip, M, C, act):
    """(errors, guards intact, y == act(nrm)): the worst per-element errors of one forward + reverse pass on l2_inputs(M, C)."""
    z, dy = l2_inputs(M, C)
    z_d, dy_d = strided(z, 1, 0), strided(dy, 1, 1)
    g_n, g_y, g_i, g_z = Guard(M, C, left=1, right=0), Guard(M, C, left=0, right=1), Guard(1, M, flat=True), Guard(M, C, left=1, right=0)
    hip.l2norm_fwd(z_d, g_n.view, g_i.view.view(M), g_y.view, act=act)
    hip.l2norm_bwd(dy_d, g_n.view, g_i.view.view(M), g_z.view, act=act)
    inv, nrm, y, dz = g_i.get()[0], g_n.get(), g_y.get(), g_z.get()
    want_inv, want_nrm, _ = ref.l2norm_ref(z, act)
    want_dz, scale = ref.l2norm_bwd_ref(dy, z, act)
    assert np.all((want_nrm == 0) <= (nrm == 0)) and np.all((scale == 0) <= (dz == 0))       # exact zeros stay exact
    errs = (float((np.abs(inv - want_inv) / want_inv).max()),
            float((np.abs(nrm - want_nrm) / np.where(want_nrm == 0, 1, np.abs(want_nrm))).max()),
            float((np.abs(dz - want_dz) / np.where(scale == 0, 1, scale)).max()))
    y_ok = np.array_equal(y, np.maximum(nrm, 0) if act == 'relu' else nrm)
    return errs, all(g.intact() for g in (g_n, g_y, g_i, g_z)), y_ok


@pytest.mark.parametrize('M,C', L2_CASES)
@pytest.mark.parametrize('act', ['relu', None])
def test_l2norm_fwd_bwd(hip, M, C, act):
    assert (M > 8192 * 256) == (C == 2)
    errs, intact, exact_ok = l2_run(hip, M, C, act)
    print('l2norm M={} C={} act={}: worst inv {:.3e} nrm {:.3e} dz {:.3e}'.format(M, C, act, *errs))
    assert exact_ok, "y = act(nrm) bit for bit"
    assert errs[0] <= L2_INV_BOUND and errs[1] <= L2_NRM_BOUND and errs[2] <= L2_DZ_BOUND, errs
    assert intact


@pytest.mark.parametrize('K,N', [(1, 1), (1, 300), (300, 1), (1500, 1400)])
def test_transpose(hip, K, N):
    """(1500, 1400): 2 100 000 elements, 2 848 past the capped grid — a second trip."""
    assert (K * N > 8192 * 256) == (K == 1500)
    src = np.random.default_rng(K + N).standard_normal((K, N)).astype(np.float32)
    got = hip.transpose(_t(src))
    assert tuple(got.shape) == (N, K) and np.array_equal(got.cpu().numpy(), src.T)
