"""amar_dense_route on the host (no GPU): which of its eight kernels amar_dense_f32 takes for a call, asked with made-up addresses — the
function looks at alignment and NULL only, nothing is dereferenced.  The launcher calls the same function, so these are the launcher's
thresholds.  And the float64 reference and bounds of tests/dense_ref.py against torch float64."""
import ctypes

import numpy as np
import pytest
import torch

from deep_cbrs_amar_renaissance_amd import capi
from tests import dense_ref as ref

BASE = 0x7F0000100000                                                  # 16-byte aligned; + 8: half way between two boundaries
EINVAL, EUNSUPPORTED = -1, -2
WT = capi.DENSE_WT


def droute(M, K, N, act=0, ldx=None, ldy=None, x_off=0, w_off=0, y_off=0, bias_off=0, ids=True, bias=True, code=False):
    """The route of a dense call on row-major operands at made-up addresses (X, W, Y, bias 16-byte aligned plus the byte offsets given),
    ldx = K and ldy = N unless given."""
    addr = {name: BASE + 0x10000000 * i for i, name in enumerate(('X', 'ids', 'W', 'bias', 'Y'))}
    info = capi.DenseRouteInfo()
    rc = capi.load().amar_dense_route(addr['X'] + x_off, K if ldx is None else ldx, addr['ids'] if ids else None, addr['W'] + w_off,
                                      addr['bias'] + bias_off if bias else None, addr['Y'] + y_off, N if ldy is None else ldy, M, K, N, act,
                                      ctypes.byref(info))
    if code:
        return rc
    assert rc == 0, rc
    return info.as_dict()


def ceil8(n):
    return -(-n // 8) * 8


def kernel_of(*args, **kwargs):
    r = droute(*args, **kwargs)
    return r['kernel'] if r['kernel'] != 'guarded' else 'guarded_' + 'ft'[r['vec_x']] + 'ft'[r['vec_w']]


def test_small_kernel_thresholds():
    assert droute(4096, 32, 64) == dict(kernel='small', vec_x=True, vec_w=True, w_trans=False, grid_x=64, grid_y=1, n_col_blocks=1, launches=1)
    assert droute(4097, 32, 64) == dict(kernel='full', vec_x=True, vec_w=True, w_trans=False, grid_x=40, grid_y=1, n_col_blocks=1, launches=1)
    assert kernel_of(1, 32, 64) == 'small' and kernel_of(4096, 768, 256) == 'small'
    for M in (1, 64, 4096):
        assert kernel_of(M, 48, 64) == 'full'                          # K % 32: never small
        assert kernel_of(M, 16, 64) == 'full'
        assert kernel_of(M, 32, 96) == 'guarded_tt'                    # N % 64
    # where small's and tile128's conditions both hold, small is asked first
    assert ceil8(4096 // 128) * (1024 // 128) >= 256
    assert droute(4096, 32, 1024) == dict(kernel='small', vec_x=True, vec_w=True, w_trans=False, grid_x=64, grid_y=16, n_col_blocks=16, launches=1)
    assert kernel_of(4097, 32, 1024) == 'tile128'


@pytest.mark.parametrize('M,N', [(3073, 1024), (15361, 256), (31745, 128)])
def test_tile128_only_where_it_fills_the_chip(M, N):
    """ceil8(ceil(M / 128)) * N / 128 >= 256: first taken at M, not one row (= one row tile) earlier."""
    ncb = N // 128
    r = droute(M, 16, N)
    assert r == dict(kernel='tile128', vec_x=True, vec_w=True, w_trans=False, grid_x=256, grid_y=1, n_col_blocks=ncb, launches=1)
    assert ceil8(-(-M // 128)) * ncb == 256 and ceil8(-(-(M - 1) // 128)) * ncb == 256 - 8 * ncb
    r = droute(M - 1, 16, N)
    assert r == dict(kernel='full', vec_x=True, vec_w=True, w_trans=False, grid_x=(256 - 8 * ncb) * 2, grid_y=1, n_col_blocks=2 * ncb, launches=1)
    assert kernel_of(M, 48, N) == 'tile128' and kernel_of(M, 8, N) == 'guarded_tt' and kernel_of(M, 24, N) == 'guarded_tt'     # K % 16
    assert kernel_of(M, 16, N + 64) == 'full'                          # N % 128
    assert kernel_of(M, 16, N + 4) == 'guarded_tt'                     # N % 64


def test_tails_go_to_the_guarded_kernel():
    for M in (1, 130, 5000):
        for K, N in ((24, 64), (17, 64), (1, 64), (16, 24), (16, 68), (48, 132), (33, 100)):
            assert kernel_of(M, K, N, ldx=(K + 3) // 4 * 4) == 'guarded_tt', (M, K, N)


@pytest.mark.parametrize('what,kwargs,want', [
    ('X + 8 bytes', dict(x_off=8), 'guarded_ft'), ('X + 4 bytes', dict(x_off=4), 'guarded_ft'), ('ldx % 4', dict(ldx=50), 'guarded_ft'),
    ('W + 8 bytes', dict(w_off=8), 'guarded_tf'), ('W + 4 bytes', dict(w_off=4), 'guarded_tf'), ('N % 4', dict(N=66), 'guarded_tf'),
    ('AMAR_DENSE_WT', dict(act=WT), 'guarded_tt'),
    ('X + 8 bytes and W + 8 bytes', dict(x_off=8, w_off=8), 'guarded_ff'), ('ldx % 4 and N % 4', dict(ldx=49, N=62), 'guarded_ff'),
    ('AMAR_DENSE_WT and X + 8 bytes', dict(act=WT | 1, x_off=8), 'guarded_ft'), ('AMAR_DENSE_WT and N % 4', dict(act=WT | 2, N=66), 'guarded_tf'),
    ('AMAR_DENSE_WT, ldx % 4 and W + 8 bytes', dict(act=WT, ldx=51, w_off=8), 'guarded_ff')])
@pytest.mark.parametrize('base', [dict(M=333, K=48, N=192), dict(M=100, K=32, N=64), dict(M=3073, K=16, N=1024)])
def test_every_alignment_fallback_from_a_guard_free_call(what, kwargs, want, base):
    """One at a time from a call that routes to full (and to small and to tile128): each gives the matching guarded variant on full's grid."""
    assert kernel_of(**base) == {333: 'full', 100: 'small', 3073: 'tile128'}[base['M']]
    if 'N' in kwargs:
        kwargs = dict(kwargs, N=base['N'] + kwargs['N'] - 64)
    if 'ldx' in kwargs:
        kwargs = dict(kwargs, ldx=base['K'] + kwargs['ldx'] - 48)
    kw = dict(base, **kwargs)
    r = droute(**kw)
    ncb = -(-kw['N'] // 64)
    assert kernel_of(**kw) == want, what
    assert r['w_trans'] == bool(kw.get('act', 0) & WT)
    assert (r['grid_x'], r['grid_y'], r['n_col_blocks'], r['launches']) == (ceil8(-(-kw['M'] // 128)) * ncb, 1, ncb, 1), what


def test_outputs_alignment_ids_and_bias_are_not_looked_at():
    for base in (dict(M=333, K=48, N=192), dict(M=100, K=32, N=64), dict(M=3073, K=16, N=1024), dict(M=64, K=17, N=65)):
        want = droute(**base)
        for kw in (dict(y_off=4), dict(y_off=8), dict(bias_off=4), dict(bias_off=8), dict(ldy=base['N'] + 5), dict(ids=False), dict(bias=False),
                   dict(act=1), dict(act=2), dict(ldx=base['K'] + 4) if base['K'] % 4 == 0 else dict()):
            assert droute(**dict(base, **kw)) == want, kw


@pytest.mark.parametrize('M', [1, 64, 65, 128, 129, 1024, 1025, 4096, 4097, 100000])
def test_grid_is_the_workgroups_the_form_needs(M):
    for K, N in ((32, 64), (64, 192), (16, 64), (48, 256), (16, 1024), (32, 2048), (24, 24), (17, 65), (48, 1), (16, 4100)):
        r = droute(M, K, N, ldx=(K + 3) // 4 * 4)
        row_tiles = -(-M // 128)
        if r['kernel'] == 'small':
            assert M <= 4096 and (r['grid_x'], r['grid_y'], r['n_col_blocks']) == (-(-M // 64), N // 64, N // 64)
        elif r['kernel'] == 'tile128':
            assert (r['grid_x'], r['grid_y'], r['n_col_blocks']) == (ceil8(row_tiles) * (N // 128), 1, N // 128) and r['grid_x'] >= 256
        else:
            assert (r['grid_x'], r['grid_y'], r['n_col_blocks']) == (ceil8(row_tiles) * -(-N // 64), 1, -(-N // 64))
        assert r['grid_x'] * r['grid_y'] >= (-(-M // 64) * (N // 64) if r['kernel'] == 'small' else row_tiles * r['n_col_blocks'])


def test_route_argument_checks_equal_the_launchers():
    """The codes of amar_dense_f32's own argument checks, for the same arguments, from the query and from the launcher (which returns
    them before it touches the device)."""
    lib, info, a = capi.load(), capi.DenseRouteInfo(), BASE
    # (X, ldx, ids, W, bias, Y, ldy, M, K, N, act)
    refused = [
        (a, 7, None, a, a, a, 8, 10, 8, 8, 0),                         # ldx < K
        (a, 8, None, a, a, a, 7, 10, 8, 8, 0),                         # ldy < N
        (a, 8, None, a, a, a, 8, 10, 8, 8, 3), (a, 8, None, a, a, a, 8, 10, 8, 8, WT | 3), (a, 8, None, a, a, a, 8, 10, 8, 8, -1),
        (a, 8, None, a, a, a, 8, 10, 8, 8, 0x200), (a, 8, None, a, a, a, 8, 0, 8, 8, 3),               # a bad act, with M == 0 too
        (None, 8, None, a, a, a, 8, 10, 8, 8, 0), (a, 8, None, None, a, a, 8, 10, 8, 8, 0), (a, 8, None, a, a, None, 8, 10, 8, 8, 0),
        (a, 8, None, a, a, a, 8, -1, 8, 8, 0), (a, 8, None, a, a, a, 8, 10, 0, 8, 0), (a, 8, None, a, a, a, 8, 10, 8, 0, 0),
        (a, 8, None, a, a, None, 8, 0, 8, 8, 0),                       # NULL is refused before M == 0 is accepted
    ]
    for args in refused:
        info.kernel = 7
        assert lib.amar_dense_route(*args, ctypes.byref(info)) == EINVAL, args
        assert info.kernel == -1
        assert lib.amar_dense_f32(*args, None) == EINVAL, args
    assert lib.amar_dense_route(a, 8, None, a, a, a, 8, 10, 8, 8, 0, None) == EINVAL
    # M == 0: nothing to do, nothing launched
    for act in (0, 1, 2, WT, WT | 2):
        assert lib.amar_dense_route(a, 8, None, a, None, a, 8, 0, 8, 8, act, ctypes.byref(info)) == 0
        assert info.as_dict() == dict(kernel=None, vec_x=False, vec_w=False, w_trans=bool(act & WT), grid_x=0, grid_y=0, n_col_blocks=0, launches=0)
        assert lib.amar_dense_f32(a, 8, None, a, None, a, 8, 0, 8, 8, act, None) == 0
    # bias and ids may be NULL
    assert droute(10, 8, 8, ids=False, bias=False, code=True) == 0
    # the XCD-affine grid must fit 2^31 - 1 workgroups
    M = 128 * (0x7fffffff // 8 * 8)
    assert droute(M, 16, 64, code=True) == 0 and droute(M + 1, 16, 64, code=True) == EUNSUPPORTED
    assert lib.amar_dense_f32(a, 16, None, a, None, a, 64, M + 1, 16, 64, 0, None) == EUNSUPPORTED
    assert droute(128 * 0x7fffffff + 1, 16, 64, code=True) == EUNSUPPORTED                         # the row tiles alone


def case_addresses(c):
    """Made-up operands laid out as the GPU test lays out the live ones: X contiguous (ldx = K) or, shifted, one float into a buffer with
    ldx = K + 4; W contiguous at an aligned address or one float in; Y at column 3 of a buffer 5 columns wider than N."""
    return dict(M=c.M, K=c.K, N=c.N, act=WT if c.w_trans else 0, ldx=c.K + 4 if c.x_shift else c.K, x_off=4 if c.x_shift else 0,
                w_off=4 if c.w_shift else 0, ldy=c.N + 5, y_off=12)


@pytest.mark.parametrize('name', [c.name for c in ref.CASES])
def test_every_case_of_the_table_routes_as_the_table_says(name):
    c = ref.CASE_BY_NAME[name]
    gx, gy, ncb = ref.expected_grid(c)
    want = dict(kernel=c.kernel, vec_x=c.vec_x, vec_w=c.vec_w, w_trans=c.w_trans, grid_x=gx, grid_y=gy, n_col_blocks=ncb, launches=1)
    for ids in (False, True):
        for bias in (False, True):
            assert droute(ids=ids, bias=bias, **case_addresses(c)) == want


def test_the_table_names_all_eight_forms_and_the_transposed_variants():
    forms = {(c.kernel, c.vec_x, c.vec_w) for c in ref.CASES if not c.w_trans}
    assert forms == {('small', True, True), ('tile128', True, True), ('full', True, True)} | {('guarded', x, w) for x in (False, True) for w in (False, True)}
    assert {(c.vec_x, c.vec_w) for c in ref.CASES if c.w_trans} == {(x, w) for x in (False, True) for w in (False, True)}
    assert all(c.kernel == 'guarded' for c in ref.CASES if c.w_trans)
    assert max(c.M * c.N * 4 for c in ref.CASES) <= 16 * 2 ** 20 + 2 ** 18            # the largest output: 16 MB


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w_transposed', [False, True])
@pytest.mark.parametrize('with_bias,with_ids', ref.VARIANTS)
def test_float64_reference_matches_torch(w_transposed, with_bias, with_ids):
    rng = np.random.default_rng(3)
    table = rng.standard_normal((50, 19)).astype(np.float32)
    w = rng.uniform(-0.3, 0.3, (23, 19) if w_transposed else (19, 23)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, 23).astype(np.float32) if with_bias else None
    ids = rng.integers(0, 50, 31).astype(np.int32) if with_ids else None
    xt = torch.tensor(table, dtype=torch.float64)
    if with_ids:
        xt = xt[torch.tensor(ids, dtype=torch.int64)]
    wt = torch.tensor(w, dtype=torch.float64)
    zt = xt @ (wt.t() if w_transposed else wt)
    st = xt.abs() @ (wt.t() if w_transposed else wt).abs()
    if with_bias:
        zt, st = zt + torch.tensor(b, dtype=torch.float64), st + torch.tensor(b, dtype=torch.float64).abs()
    for act, fn in (('none', lambda t: t), ('relu', torch.relu), ('sigmoid', torch.sigmoid)):
        want, s = ref.dense_ref(table, w, b, act, ids, w_transposed)
        assert want.dtype == np.float64 and want.shape == (31 if with_ids else 50, 23)
        np.testing.assert_allclose(want, fn(zt).numpy(), rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(s, st.numpy(), rtol=1e-14, atol=0)
        assert np.all(np.abs(want) <= s * (1 + 1e-15) + (act == 'sigmoid'))


def test_bounds_are_the_derived_figures_and_hold_for_float32_sums():
    s = np.array([[0.5, 2.0]])
    assert np.array_equal(ref.linear_bound(16, s), 19 * 2.0 ** -24 * s) and np.array_equal(ref.bound(16, s, 'relu'), ref.bound(16, s, 'none'))
    assert np.array_equal(ref.bound(16, s, 'sigmoid'), 19 * 2.0 ** -24 * s / 4 + ref.SIGMOID_F32_EVAL)
    # a float32 fma-free sum in k order, and numpy's pairwise float32 matmul, stay inside the bound; the bound is not vacuous: dropping
    # the smallest term of one element, or one k-tile, leaves it
    rng = np.random.default_rng(5)
    x, w, b = rng.standard_normal((40, 48)).astype(np.float32), rng.uniform(-0.3, 0.3, (48, 9)).astype(np.float32), rng.uniform(-0.2, 0.2, 9).astype(np.float32)
    z, sc = ref.pre_activation(x, w, b)
    seq = np.zeros((40, 9), np.float32)
    for k in range(48):
        seq = seq + x[:, k:k + 1] * w[k:k + 1, :]
    seq = seq + b
    for got in (seq, x @ w + b):
        assert got.dtype == np.float32
        for act in ref.ACTS:
            got_a = ref.activation(got, act) if act != 'sigmoid' else (np.float32(1) / (np.float32(1) + np.exp(-got)))
            assert np.all(np.abs(got_a.astype(np.float64) - ref.activation(z, act)) <= ref.bound(48, sc, act)), act
    assert not np.all(np.abs((x[:, :32] @ w[:32] + b).astype(np.float64) - z) <= ref.linear_bound(48, sc))
    terms = np.abs(x[:, :, None].astype(np.float64) * w[None, :, :])
    terms[terms < 1e-3] = np.inf                                       # (a term below the bound itself cannot be missed by any test)
    k_min = terms.argmin(1)
    dropped = seq.astype(np.float64) - np.take_along_axis(x[:, :, None].astype(np.float64) * w[None], k_min[:, None, :], 1)[:, 0, :]
    assert np.all(np.abs(dropped - z) > ref.linear_bound(48, sc))


def test_sigmoid_term_is_measured_not_chosen():
    """SIGMOID_F32_EVAL = SIGMOID_FACTOR x what numpy float32 leaves on the z of every case of the table, re-measured here."""
    measured = ref.measure_sigmoid_term()
    print('sigmoid float32 evaluation error over the case table:', measured)
    assert abs(measured - ref.SIGMOID_F32_MEASURED) <= 0.05 * measured
    assert ref.SIGMOID_FACTOR == 2.0 and ref.SIGMOID_F32_EVAL == 2.0 * ref.SIGMOID_F32_MEASURED
    assert measured < 2 * 2.0 ** -23                                   # a few float32 roundings of a value below 1
    assert ref.SIGMOID_F32_EVAL <= 1e-6                                # the suite's own figure for sigmoid outputs
