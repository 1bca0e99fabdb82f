"""Every kernel form of amar_dense_f32 on the device: the 64 x 64 small kernel, the 128 x 128 tile, the guard-free 128 x 64 tile, the four
guarded variants, and a transposed W in every vec pair — at the smallest shapes at which each can go wrong (tests/dense_ref.py: CASES).

Every case asserts its route on the live tensors (capi.dense_route: the launcher asks the same host function) and only then launches.
Each runs with all three activations, with and without bias, with and without a row gather (ids out of order, with repeats, over a table
taller than M), into a column window at offset 3 of a wider buffer: the window is NaN before the call and must hold no NaN after it, every
element must lie within the derived bound of its float64 value — (K + 3) 2^-24 (sum_k |x_k||w_k| + |b|) per element, a quarter of it plus
the measured float32 evaluation term for the sigmoid — and every sentinel around the window (three columns left, two right, one row below)
must keep its bits.  Then the forms against each other, bit for bit, on one product."""
import numpy as np
import pytest
import torch

from tests import dense_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 1234.5
LEFT, RIGHT = 3, 2                                                     # sentinel columns left and right of the window (offset 3: not a multiple of 4)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)          # (a copy: the shared inputs are read-only)


def shifted_rows(a, pad=4):
    """`a` [R, K] as a view one float into an aligned device buffer, leading dimension K + pad."""
    R, K = a.shape
    buf = torch.zeros(R * (K + pad) + 4, device=DEV)
    view = buf[1:1 + R * (K + pad)].view(R, K + pad)[:, :K]
    view.copy_(_t(a))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == K + pad
    return view


def shifted_flat(a):
    """`a` as a contiguous view one float into a flat device buffer."""
    buf = torch.zeros(a.size + 1, device=DEV)
    view = buf[1:].view(*a.shape)
    view.copy_(_t(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def window(M, N):
    """(buffer, Y): Y = the [M, N] window at column LEFT of a buffer of M + 1 rows; NaN inside, SENTINEL outside."""
    buf = torch.full((M + 1, LEFT + N + RIGHT), SENTINEL, device=DEV)
    y = buf[:M, LEFT:LEFT + N]
    y.fill_(float('nan'))
    return buf, y


def sentinels_untouched(buf, M, N):
    rest = buf.clone()
    rest[:M, LEFT:LEFT + N] = SENTINEL
    return torch.equal(rest.view(torch.int32), torch.full_like(buf, SENTINEL).view(torch.int32))


def expected_route(c):
    gx, gy, ncb = ref.expected_grid(c)
    return dict(kernel=c.kernel, vec_x=c.vec_x, vec_w=c.vec_w, w_trans=c.w_trans, grid_x=gx, grid_y=gy, n_col_blocks=ncb, launches=1)


_OPERANDS = {}


def device_operands(name):
    """The case's operands on the device, laid out as the case asks (kept for the case's four variants, then dropped)."""
    if name not in _OPERANDS:
        _OPERANDS.clear()
        c = ref.CASE_BY_NAME[name]
        table, w, b, ids = ref.case_inputs(name)
        _OPERANDS[name] = (shifted_rows(table) if c.x_shift else _t(table), shifted_flat(w) if c.w_shift else _t(w), _t(b), _t(ids))
    return _OPERANDS[name]


@pytest.mark.parametrize('with_bias,with_ids', ref.VARIANTS)
@pytest.mark.parametrize('name', [c.name for c in ref.CASES])
def test_dense_form(hip, name, with_bias, with_ids):
    c = ref.CASE_BY_NAME[name]
    table_d, w_d, b_d, ids_d = device_operands(name)
    x_d = table_d if with_ids else table_d[:c.M]
    z, s = ref.case_reference(name, with_bias, with_ids)
    buf, y = window(c.M, c.N)
    for act in ref.ACTS:
        kw = dict(act=ref.capi_act(act), ids=ids_d if with_ids else None, w_transposed=c.w_trans)
        assert hip.dense_route(x_d, w_d, y, **kw) == expected_route(c)
        y.fill_(float('nan'))
        hip.dense(x_d, w_d, b_d if with_bias else None, y, **kw)
        torch.cuda.synchronize()
        got = y.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any(), act
        err, lim = np.abs(got - ref.activation(z, act)), ref.bound(c.K, s, act)
        print('{} bias={} ids={} {}: worst error / bound = {:.3f}'.format(name, with_bias, with_ids, act, float((err / lim).max())))
        assert np.all(err <= lim), (act, float((err / lim).max()), np.argwhere(err > lim)[:4].tolist())
        assert sentinels_untouched(buf, c.M, c.N), act


def test_the_cases_name_each_of_the_eight_forms(hip):
    """What test_dense_form asserts as routes covers the eight kernels (and the four transposed variants)."""
    routes = {(c.kernel, c.vec_x, c.vec_w, c.w_trans) for c in ref.CASES}
    for kernel in ('small', 'tile128', 'full'):
        assert (kernel, True, True, False) in routes
    for vx in (False, True):
        for vw in (False, True):
            assert ('guarded', vx, vw, False) in routes and ('guarded', vx, vw, True) in routes


def test_forms_agree_bit_for_bit(hip):
    """One product (K = 64, N = 1024); its first 64 rows through small, through full (inside a 4 097-row call, N cut into column ranges
    that are no multiple of 128), through tile128 (the 4 097-row call on all of N: with K % 32 == 0 a call of up to 4 096 rows is small's,
    so the 128 x 128 tile needs one row more), through the guarded kernel by a misaligned X, by a misaligned W, and through a transposed
    W: the same instruction in the same k order everywhere, zero padding in the guarded ones."""
    rng = np.random.default_rng(64)
    K, N, R = 64, 1024, 64
    x = rng.standard_normal((4097, K)).astype(np.float32)
    w = rng.uniform(-0.3, 0.3, (K, N)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, N).astype(np.float32)
    x_d, w_d, b_d = _t(x), _t(w), _t(b)
    x_shift, w_shift, wt_d = shifted_rows(x[:R]), shifted_flat(w), _t(w.T)
    cuts = [(0, 192), (192, 384), (384, 576), (576, 768), (768, 960), (960, 1024)]
    w_cut = [_t(w[:, lo:hi]) for lo, hi in cuts]
    for act in ref.ACTS:
        a = ref.capi_act(act)
        out = {}

        def run(key, X, W, Y, bias, kernel, vec=(True, True), wt=False):
            r = hip.dense_route(X, W, Y, act=a, w_transposed=wt)
            assert (r['kernel'], r['vec_x'], r['vec_w'], r['w_trans']) == (kernel, vec[0], vec[1], wt), (key, r)
            hip.dense(X, W, bias, Y, act=a, w_transposed=wt)

        out['small'] = torch.full((R, N), float('nan'), device=DEV)
        run('small', x_d[:R], w_d, out['small'], b_d, 'small')
        full = torch.full((4097, N), float('nan'), device=DEV)
        for (lo, hi), wc in zip(cuts, w_cut):
            run('full', x_d, wc, full[:, lo:hi], b_d[lo:hi], 'full')
        out['full'] = full[:R]
        t128 = torch.full((4097, N), float('nan'), device=DEV)
        run('tile128', x_d, w_d, t128, b_d, 'tile128')
        out['tile128'] = t128[:R]
        out['guarded_x'] = torch.full((R, N), float('nan'), device=DEV)
        run('guarded_x', x_shift, w_d, out['guarded_x'], b_d, 'guarded', (False, True))
        out['guarded_w'] = torch.full((R, N), float('nan'), device=DEV)
        run('guarded_w', x_d[:R], w_shift, out['guarded_w'], b_d, 'guarded', (True, False))
        out['transposed'] = torch.full((R, N), float('nan'), device=DEV)
        run('transposed', x_d[:R], wt_d, out['transposed'], b_d, 'guarded', (True, True), wt=True)
        torch.cuda.synchronize()
        assert not torch.isnan(out['small']).any()
        for key, y in out.items():
            assert torch.equal(y, out['small']), (act, key, int((y != out['small']).sum()))
        # every row the two big calls share, not only the first 64
        assert torch.equal(full, t128), act
    # and the float64 value, so that agreeing is not agreeing on something else
    z, s = ref.pre_activation(x[:R], w, b)
    assert np.all(np.abs(out['small'].cpu().numpy().astype(np.float64) - ref.activation(z, 'sigmoid')) <= ref.bound(K, s, 'sigmoid'))


def test_full_and_tile128_agree_across_the_threshold(hip):
    """(3 072, 16, 1 024) runs the guard-free 128 x 64 tile, (3 073, 16, 1 024) the 128 x 128 tile: the shared rows, bit for bit."""
    name = 'tile128-3073x16x1024'
    table_d, w_d, b_d, _ = device_operands(name)
    y_full, y_128 = torch.full((3072, 1024), float('nan'), device=DEV), torch.full((3073, 1024), float('nan'), device=DEV)
    assert hip.dense_route(table_d[:3072], w_d, y_full, act='relu')['kernel'] == 'full'
    assert hip.dense_route(table_d[:3073], w_d, y_128, act='relu')['kernel'] == 'tile128'
    hip.dense(table_d[:3072], w_d, b_d, y_full, act='relu')
    hip.dense(table_d[:3073], w_d, b_d, y_128, act='relu')
    assert not torch.isnan(y_128).any()
    assert torch.equal(y_128[:3072], y_full)
    _OPERANDS.clear()
