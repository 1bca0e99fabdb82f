"""Direct tests of the C-ABI entry points that the rest of the suite reaches only through whole models: the two-branch head
(amar_dual_chain_f32 / _indexed_f32), the element-wise head kernels (attention mix, add3, locality scale, with reverses), the optimizer
kernels (adam_advance / adam_dev / adam_multi / sum_into), amar_bce_grad_f32 and amar_colmax_f32 (pytest -m gpu).

Reference: tests/entry_point_ref.py (numpy float64; pinned to oracle.* and autograd by tests/test_entry_points_cpu.py).  Errors are measured
per element against the element's own scale (the sum of the magnitudes of its terms), never against the largest value of the array; every
output starts as NaN or a sentinel, every strided output has guard columns on both sides that must keep it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dual_chain_worker as dw
from tests import entry_point_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
_t = dw._t


# ---- two-branch head ------------------------------------------------------------------------------------------------------------------
# Which kernel a case reaches, by the dispatcher (amar_dual_chain_indexed_f32): `full` = D == W == 64, ReLU everywhere, n_branch >= 1 and all
# four id lists.  full and the split image (3 KB per fragment triple: 8 per branch layer, 16 + 8 per further trunk layer, plus the tail)
# <= 160 KB -> dual_chain_split_kernel<1, 768>; full otherwise, or with AMAR_PAIR_MFMA=f32 -> dual_chain_full_kernel; everything else ->
# dual_chain_kernel<1> (1 024 threads = 16 waves of 16 pairs, at most 1 024 workgroups: one grid pass covers 262 144 pairs).

def _check_scores(got, want, scale, last_act):
    assert np.isfinite(got).all()
    if last_act == 'sigmoid':
        err = float(np.abs(got - want).max())
        print('max |score - float64| = {:.3g}'.format(err))
        assert err < 1e-6
    else:
        err = ref.scaled_error(got, want, scale)
        print('max |out - float64| / scale = {:.3g}'.format(err))
        assert err < 5e-6                                             # test_chain_fused_stack's bound, per element


def _rows(rng, n_rows, P):
    return [rng.integers(0, n_rows, P) for _ in range(2)], [rng.integers(0, n_rows, P) for _ in range(2)]


GENERIC_SHAPES = [(D, W) for D in (16, 32, 48, 64) for W in (4, 20, 48, 64)]


@pytest.mark.parametrize('k', range(len(GENERIC_SHAPES)), ids=['D{}-W{}'.format(*s) for s in GENERIC_SHAPES])
def test_dual_chain_generic_kernel_shapes(hip, k):
    """dual_chain_kernel<1> (none of these is `full`: 64 x 64 comes with n_branch = 0) over every D x W, with n_branch, the activations,
    the trunk depth and the last activation rotating; P around the 16-pair tile and the 256-pair workgroup; alternately on contiguous tables
    and on column slices of NaN-padded wider buffers (lda = D + 12) with `out` one column of a [P, 3] buffer; bases 3 / 5 / 7 / 11 on views
    that start that many rows into their buffers."""
    D, W = GENERIC_SHAPES[k]
    n_branch, n_trunk = k % 3, 2 + k % 2
    in_act = ('relu', 'none', 'sigmoid')[(k // 3) % 3]
    branch_acts = (['relu', 'none'], ['none', 'relu'])[k % 2][:n_branch]
    last = ('sigmoid', 'none')[(k // 2) % 2]
    trunk_acts = ['relu'] * (n_trunk - 1) + [last]
    assert not (D == 64 and W == 64 and n_branch >= 1 and in_act == 'relu')
    h = ref.draw_dual_head(np.random.default_rng(100 + k), D, W, n_branch, n_trunk, 400)
    wpack = dw.pack(hip, h)
    for n, P in enumerate((1, 15, 16, 17, 255, 257)):
        rows_a, rows_b = _rows(np.random.default_rng(1000 * k + P), 380, P)
        layout = n % 2 == 1
        got, buf = dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, in_act, branch_acts, trunk_acts, sliced=layout, strided_out=layout)
        want, scale = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], in_act, branch_acts, trunk_acts)
        _check_scores(got, want, scale, last)
        if layout:
            assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, 2]).all()


@pytest.mark.parametrize('missing', range(4))
@pytest.mark.parametrize('D,W', [(64, 64), (32, 20)])
def test_dual_chain_table_read_without_ids(hip, missing, D, W):
    """Each of the four id lists absent in turn: pair p reads row p of that table in place (the 64 x 64 ReLU head leaves the guard-free
    kernels for dual_chain_kernel<1> with it); the other three keep their lists and non-zero bases."""
    P = 300
    h = ref.draw_dual_head(np.random.default_rng(200 + missing), D, W, 1, 3, 400)
    rows_a, rows_b = _rows(np.random.default_rng(201 + missing), 380, P)
    rows_dev_a, rows_dev_b = list(rows_a), list(rows_b)
    (rows_dev_a if missing < 2 else rows_dev_b)[missing % 2] = None
    (rows_a if missing < 2 else rows_b)[missing % 2] = np.arange(P)
    acts = ['relu', 'relu', 'sigmoid']
    for sliced in (False, True):
        got, _ = dw.run(hip, h, dw.pack(hip, h), rows_dev_a, rows_dev_b, [3, 5], [7, 11], P, 'relu', ['relu'], acts, sliced=sliced)
        want, scale = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], 'relu', ['relu'], acts)
        _check_scores(got, want, scale, 'sigmoid')


def _indexed_equals_scattered(hip, h, wpack, rows_a, rows_b, P, in_act, branch_acts, trunk_acts, plain):
    perm = np.random.default_rng(P).permutation(P).astype(np.int32)
    got, _ = dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, in_act, branch_acts, trunk_acts, out_index=_t(perm))
    scattered = np.empty_like(plain)
    scattered[perm] = plain
    assert np.array_equal(got.view(np.int32), scattered.view(np.int32))          # bit for bit


def test_dual_chain_generic_kernel_second_grid_pass(hip):
    """P = 262 144 + 333: the 1 024 workgroups of dual_chain_kernel<1> (in_act = none keeps the case off the guard-free kernels) start a
    second grid-stride pass that ends inside a tile; also through out_index (a random permutation) against the plain call scattered on the host."""
    P = 1024 * 256 + 333
    for D, W, n_branch, in_act, last in ((32, 20, 1, 'relu', 'none'), (64, 64, 1, 'none', 'sigmoid')):
        h = ref.draw_dual_head(np.random.default_rng(300 + D), D, W, n_branch, 3, 3000)
        rows_a, rows_b = _rows(np.random.default_rng(301), 2900, P)
        acts = ['relu', 'relu', last]
        wpack = dw.pack(hip, h)
        got, _ = dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, in_act, ['relu'] * n_branch, acts)
        want, scale = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], in_act, ['relu'] * n_branch, acts)
        _check_scores(got, want, scale, last)
        _indexed_equals_scattered(hip, h, wpack, rows_a, rows_b, P, in_act, ['relu'] * n_branch, acts, got)


def _f32_layer_by_layer(hip, h, rows_a, rows_b, n_branch, trunk_acts):
    """The f32 evaluation: amar_chain_f32's generic kernel (f32 matrix instruction) layer by layer on pre-gathered, pre-summed rows, as
    test_pair_stage_split_products_against_f32_and_f64 takes it."""
    xs = []
    for br in range(2):
        x = torch.relu(_t(h['A'][br])[_t(rows_a[br])] + _t(h['B'][br])[_t(rows_b[br])]).contiguous()
        for w, b in h['branch'][br]:
            blob, dims = hip.chain_pack([w], [b])
            y = torch.empty((x.shape[0], dims[-1]), device=DEV)
            hip.chain(x, _t(blob), dims, ['relu'], y)
            x = y
        xs.append(x)
    blob, dims = hip.chain_pack([w for w, _ in h['trunk']], [b for _, b in h['trunk']])
    out = torch.empty((xs[0].shape[0], 1), device=DEV)
    hip.chain(torch.cat(xs, dim=1).contiguous(), _t(blob), dims, [None if a == 'none' else a for a in trunk_acts], out)
    torch.cuda.synchronize()
    return out[:, 0].cpu().numpy()


@pytest.mark.parametrize('n_branch,n_trunk', [(1, 2), (1, 3), (2, 2)])
def test_dual_chain_split_kernel(hip, n_branch, n_trunk):
    """dual_chain_split_kernel<1, 768> (D = W = 64, ReLU throughout, all id lists; 8 n_branch * 2 + 16 + 8 (n_trunk - 2) fragment triples =
    32 / 40 / 48 -> 96 / 120 / 144 KB + tail <= 160 KB): 12 waves of 16 pairs per workgroup, so P around 192 and one P above the 1 024 x 192
    of a grid pass.  Scores within 1e-6 of float64, on average no less accurate than the f32 instruction, out_index bit for bit."""
    assert os.environ.get('AMAR_PAIR_MFMA') != 'f32'
    h = ref.draw_dual_head(np.random.default_rng(400 + 10 * n_branch + n_trunk), 64, 64, n_branch, n_trunk, 3000)
    wpack = dw.pack(hip, h)
    acts, bacts = ['relu'] * (n_trunk - 1) + ['sigmoid'], ['relu'] * n_branch
    for P in (1, 191, 192, 193, 1024 * 192 + 500):
        rows_a, rows_b = _rows(np.random.default_rng(401 + P), 2900, P)
        got, _ = dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, 'relu', bacts, acts, sliced=P == 193, strided_out=P == 193)
        want, scale = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], 'relu', bacts, acts)
        _check_scores(got, want, scale, 'sigmoid')
        if P > 1000:
            assert want.min() < 0.3 and want.max() > 0.7                                          # scores spread over (0, 1)
            f32 = _f32_layer_by_layer(hip, h, rows_a, rows_b, n_branch, acts)
            e_split, e_f32 = np.abs(got - want), np.abs(f32 - want)
            print('mean error: split {:.3g}, f32 {:.3g}; max {:.3g} / {:.3g}'.format(e_split.mean(), e_f32.mean(), e_split.max(), e_f32.max()))
            assert e_f32.max() < 1e-6
            assert e_split.mean() < 1.5 * e_f32.mean() + 1e-9
            _indexed_equals_scattered(hip, h, wpack, rows_a, rows_b, P, 'relu', bacts, acts, got)


@pytest.mark.parametrize('P', [17, 4099])
def test_dual_chain_full_kernel_when_the_split_image_exceeds_the_lds(hip, P):
    """D = W = 64, n_branch = 2, a three-layer trunk: 32 + 16 + 8 = 56 fragment triples = 168 KB > 160 KB, so the guard-free f32 kernel
    dual_chain_full_kernel runs in this process (its f32 blob is 114 KB)."""
    h = ref.draw_dual_head(np.random.default_rng(500), 64, 64, 2, 3, 3000)
    wpack = dw.pack(hip, h)
    acts, bacts = ['relu', 'relu', 'sigmoid'], ['relu', 'relu']
    rows_a, rows_b = _rows(np.random.default_rng(501 + P), 2900, P)
    got, buf = dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, 'relu', bacts, acts, sliced=True, strided_out=True)
    want, scale = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], 'relu', bacts, acts)
    _check_scores(got, want, scale, 'sigmoid')
    assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, 2]).all()
    _indexed_equals_scattered(hip, h, wpack, rows_a, rows_b, P, 'relu', bacts, acts,
                              dw.run(hip, h, wpack, rows_a, rows_b, [3, 5], [7, 11], P, 'relu', bacts, acts)[0])


def _raw_dual(hip, D, trunk_dims, lda=None, P=8, n_branch=1, out=None, indexed=False):
    """amar_dual_chain_f32 called with explicit arguments (the wrapper derives lda from the tensors); returns the status code."""
    lda = lda if lda is not None else [D, D]
    tabs = [torch.zeros((16, max(D, 68) + 4), device=DEV) for _ in range(4)]
    ids = [torch.zeros(max(P, 1), dtype=torch.int32, device=DEV) for _ in range(4)]
    wpack = torch.zeros(40_000, device=DEV)
    out = out if out is not None else torch.zeros((max(P, 1), 1), device=DEV)
    arr = lambda vals, ctype: (ctype * len(vals))(*vals)                                                   # noqa: E731
    args = [arr([t.data_ptr() for t in tabs[:2]], ctypes.c_void_p), arr(lda, ctypes.c_int64), arr([t.data_ptr() for t in ids[:2]], ctypes.c_void_p),
            arr([0, 0], ctypes.c_int32), arr([t.data_ptr() for t in tabs[2:]], ctypes.c_void_p), arr(lda, ctypes.c_int64),
            arr([t.data_ptr() for t in ids[2:]], ctypes.c_void_p), arr([0, 0], ctypes.c_int32), D, 1, n_branch, arr([1] * max(1, n_branch), ctypes.c_int32),
            arr(trunk_dims, ctypes.c_int32), arr([1] * (len(trunk_dims) - 2) + [2], ctypes.c_int32), len(trunk_dims) - 1, wpack.data_ptr(),
            out.data_ptr(), 1]
    lib = hip.load()
    code = lib.amar_dual_chain_indexed_f32(*args, None, P, None) if indexed else lib.amar_dual_chain_f32(*args, P, None)
    torch.cuda.synchronize()
    return code


def test_dual_chain_refusals_are_part_of_the_contract(hip):
    assert _raw_dual(hip, 16, [32, 16, 1]) == OK and _raw_dual(hip, 16, [32, 16, 1], indexed=True) == OK      # the helper's own arguments are valid
    assert _raw_dual(hip, 20, [40, 20, 1]) == EUNSUPPORTED                                                    # D % 16 != 0
    assert _raw_dual(hip, 68, [136, 64, 1]) == EUNSUPPORTED                                                   # D > 64
    assert _raw_dual(hip, 32, [64, 32, 16, 1]) == EUNSUPPORTED                                                # unequal trunk hidden widths
    assert _raw_dual(hip, 32, [48, 32, 1]) == EINVAL                                                          # trunk_dims[0] != 2 D
    assert _raw_dual(hip, 32, [64, 32, 2]) == EINVAL                                                          # last width != 1
    assert _raw_dual(hip, 32, [64, 32, 1], lda=[28, 32]) == EINVAL                                            # lda < D
    assert _raw_dual(hip, 32, [64, 32, 1], lda=[32, 34]) == EINVAL                                            # lda % 4 != 0
    out = torch.full((4, 1), -7.0, device=DEV)
    assert _raw_dual(hip, 32, [64, 32, 1], P=0, out=out) == OK                                                # P = 0: nothing launched
    assert bool((out == -7.0).all())
    h = ref.draw_dual_head(np.random.default_rng(1), 20, 20, 0, 2, 40)                                        # and through the wrapper: an error, no fallback
    wpack, (rows_a, rows_b) = dw.pack(hip, h), _rows(np.random.default_rng(2), 30, 8)
    with pytest.raises(hip.AmarError, match=r'amar_dual_chain_f32 failed.*code -2'):
        dw.run(hip, h, wpack, rows_a, rows_b, [0, 0], [0, 0], 8, 'relu', [], ['relu', 'sigmoid'])


def test_dual_chain_f32_switch_in_a_child_process(hip, tmp_path):
    """AMAR_PAIR_MFMA=f32 is read once per process, so ONE fresh child (tests/dual_chain_worker.py) scores the common head with it:
    dual_chain_full_kernel on a shape whose default is the split kernel.  f32 form within 1e-6 of float64 and within 5e-7 of this
    process's split-form scores."""
    assert os.environ.get('AMAR_PAIR_MFMA') != 'f32'
    path = str(tmp_path / 'f32_scores.npy')
    env = dict(os.environ, AMAR_PAIR_MFMA='f32')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'dual_chain_worker.py'), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    f32 = np.load(path)
    split = dw.score_common_case(hip)
    h, rows_a, rows_b, P = dw.common_case()
    want, _ = ref.dual_head(h['A'], h['B'], rows_a, rows_b, h['branch'], h['trunk'], 'relu', ['relu'], ['relu', 'relu', 'sigmoid'])
    print('f32 form: max error {:.3g}; split form: {:.3g}; f32 - split: {:.3g}'.format(np.abs(f32 - want).max(), np.abs(split - want).max(),
                                                                                     np.abs(f32 - split).max()))
    assert f32.shape == (P,) and np.isfinite(f32).all()
    assert np.abs(f32 - want).max() < 1e-6 and np.abs(split - want).max() < 1e-6
    assert np.abs(f32 - split).max() < 5e-7


# ---- element-wise head kernels --------------------------------------------------------------------------------------------------------------
# grid1d caps a launch at 8 192 blocks of 256: M x width = 40 000 x 64 > 2 097 152 makes every thread take a second grid-stride step.
ELEMENTWISE_SHAPES = [(M, W) for M in (1, 257, 5000) for W in (1, 5, 8, 64, 100)] + [(40_000, 64)]
SENTINEL = -12345.0


def _slice_of(a, ld_extra, offset=1):
    """A float32 [M, W] array as a column slice (starting at column `offset`) of a sentinel-filled [M, W + ld_extra] device buffer: its own,
    possibly odd, leading dimension and guard columns on both sides."""
    M, W = a.shape
    buf = torch.full((M, W + ld_extra), SENTINEL, device=DEV)
    view = buf[:, offset:offset + W]
    view.copy_(_t(a))
    return view, buf


def _out_slice(M, W, ld_extra, offset=1):
    buf = torch.full((M, W + ld_extra), float('nan'), device=DEV)
    buf[:, :offset] = SENTINEL
    buf[:, offset + W:] = SENTINEL
    return buf[:, offset:offset + W], buf


def _guards_kept(buf, W, offset=1):
    return bool((buf[:, :offset] == SENTINEL).all()) and bool((buf[:, offset + W:] == SENTINEL).all())


def _bound(key):
    """KERNEL_FACTOR x what numpy float32 leaves on the reference inputs, measured when first asked (on the CPU)."""
    return ref.KERNEL_FACTOR * ref.f32_numpy_figures()[key]


@pytest.mark.parametrize('M,W', ELEMENTWISE_SHAPES)
def test_attention_mix_and_reverse(hip, M, W):
    """amar_attention_mix_f32 / _bwd_f32 on column slices with leading dimensions W + 3, W + 2, W + 5, W + 4, W + 7 (odd ones included),
    saturated tanh and a == b planted.  Error per element against max(|a|, |b|) (forward), |dOut| (dA, dB) and |dOut| |a - b| (dTA, dTB).
    numpy float32 leaves 2.197e-7 forward and 1.367e-7 in reverse on the reference inputs (ref.f32_numpy_figures); the kernels are held to
    4 x that: 8.8e-7 and 5.5e-7."""
    dout, a, b, ta, tb = ref.draw_attention_inputs(np.random.default_rng(M + W), M, W)
    (dd, _), (ad, _), (bd, _), (tad, _), (tbd, _) = (_slice_of(t, e) for t, e in zip((dout, a, b, ta, tb), (3, 2, 5, 4, 7)))
    out, obuf = _out_slice(M, W, 3)
    hip.attention_mix(ad, bd, tad, tbd, out)
    f64 = [t.astype(np.float64) for t in (dout, a, b, ta, tb)]
    fwd_scale, bwd_scales = ref.attention_scales(dout, a, b)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and _guards_kept(obuf, W)
    err = ref.scaled_error(got, ref.attention_mix(*f64[1:]), fwd_scale)
    print('forward: {:.3g} (bound {:.3g})'.format(err, _bound('attention_mix')))
    assert err < _bound('attention_mix')
    same = a == b
    assert np.array_equal(got[same], a[same]) or np.abs(got[same] - a[same]).max() <= 2 ** -23 * np.abs(a[same]).max()   # a == b: out = a
    grads = [g.cpu().numpy() for g in hip.attention_mix_bwd(dd, ad, bd, tad, tbd)]
    want = ref.attention_mix_bwd(*f64)
    for name, g, w, s in zip(('dA', 'dB', 'dTA', 'dTB'), grads, want, bwd_scales):
        assert np.isfinite(g).all()
        err = ref.scaled_error(g, w, s)
        print('{}: {:.3g} (bound {:.3g})'.format(name, err, _bound('attention_mix_bwd')))
        assert err < _bound('attention_mix_bwd')
    # dA + dB = dOut to rounding: wa and 1 - wa are complementary
    assert np.abs(grads[0].astype(np.float64) + grads[1] - dout).max() <= 3 * ref.F32_EPS * max(1e-30, np.abs(dout).max())
    assert ref.scaled_error(grads[0].astype(np.float64) + grads[1], dout.astype(np.float64), np.abs(dout.astype(np.float64))) <= 4 * ref.F32_EPS


@pytest.mark.parametrize('act', ['none', 'relu', 'sigmoid'])
@pytest.mark.parametrize('M,W', ELEMENTWISE_SHAPES)
def test_add3_act(hip, M, W, act):
    """amar_add3_act_f32 on slices with leading dimensions W + 3 / W + 2 / W + 5, out W + 4.  Scale |a| + |b| + |c| (through the sigmoid:
    times s (1 - s), plus s).  numpy float32: 1.121e-7 / 1.131e-7 / 1.372e-7 (none / relu / sigmoid) -> bounds 4.5e-7 / 4.5e-7 / 5.5e-7.
    Planted: sums of +-100 under the sigmoid (1 and ~0, never NaN), exact-zero sums under ReLU."""
    a, b, c = ref.draw_add3_inputs(np.random.default_rng(7 * M + W), M, W, act)
    (ad, _), (bd, _), (cd, _) = (_slice_of(t, e) for t, e in zip((a, b, c), (3, 2, 5)))
    out, obuf = _out_slice(M, W, 4, offset=2)
    hip.add3_act(ad, bd, cd, out, act=None if act == 'none' else act)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and _guards_kept(obuf, W, offset=2)
    with np.errstate(over='ignore'):
        want = ref.add3_act(*(t.astype(np.float64) for t in (a, b, c)), act)
    err = ref.scaled_error(got, want, ref.add3_scale(a, b, c, act))
    print('{}: {:.3g} (bound {:.3g})'.format(act, err, _bound('add3_' + act)))
    assert err < _bound('add3_' + act)
    flat, n = got.reshape(-1), min(M * W, 6)
    if act == 'sigmoid':
        assert all(flat[j] == (1.0 if j % 2 == 0 else flat[j]) and (j % 2 == 0 or 0 <= flat[j] < 1e-37) for j in range(n))
    if act == 'relu' and n == 6:
        assert flat[0] == 0 and flat[1] == 0 and flat[2] == 0 and flat[3] == 0 and flat[4] == 0 and flat[5] == 0


@pytest.mark.parametrize('M,W', ELEMENTWISE_SHAPES)
def test_locality_scale_and_reverse(hip, M, W):
    """amar_locality_scale_f32 / _bwd_f32 on slices (leading dimensions W + 3, W + 2; out / dX W + 5).  Scales |x| (forward), |dOut| (dX,
    plus |previous dX| when accumulating) and sum |dOut x| per row (dw).  numpy float32: 1.124e-7 forward, 1.313e-7 reverse -> bounds 4.5e-7,
    5.3e-7.  w = +-100 planted: sigmoid' = 0, dw = 0 and never NaN.  accumulate = 1 adds the previous dX exactly once."""
    dout, x, w = ref.draw_locality_inputs(np.random.default_rng(3 * M + W), M, W)
    (dd, _), (xd, _) = (_slice_of(t, e) for t, e in zip((dout, x), (3, 2)))
    wd = _t(w)
    out, obuf = _out_slice(M, W, 5, offset=2)
    hip.locality_scale(xd, wd, out)
    d64, x64, w64 = (t.astype(np.float64) for t in (dout, x, w))
    fwd_scale, (dx_scale, dw_scale) = ref.locality_scales(dout, x)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and _guards_kept(obuf, W, offset=2)
    err = ref.scaled_error(got, ref.locality_scale(x64, w64), fwd_scale)
    print('forward: {:.3g} (bound {:.3g})'.format(err, _bound('locality_scale')))
    assert err < _bound('locality_scale')
    want_dx, want_dw = ref.locality_scale_bwd(d64, x64, w64)
    prev = np.random.default_rng(5).standard_normal((M, W)).astype(np.float32)
    for accumulate in (False, True):
        dx, dxbuf = _out_slice(M, W, 5, offset=2)
        if accumulate:
            dx.copy_(_t(prev))
        dwd = torch.full((M,), float('nan'), device=DEV)
        hip.locality_scale_bwd(dd, xd, wd, dx, dwd, accumulate=accumulate)
        gdx, gdw = dx.cpu().numpy(), dwd.cpu().numpy()
        assert np.isfinite(gdx).all() and np.isfinite(gdw).all() and _guards_kept(dxbuf, W, offset=2)
        e_dx = ref.scaled_error(gdx, want_dx + (prev if accumulate else 0), dx_scale + (np.abs(prev) if accumulate else 0))
        e_dw = ref.scaled_error(gdw, want_dw, dw_scale)
        print('accumulate={}: dX {:.3g}, dw {:.3g} (bound {:.3g})'.format(accumulate, e_dx, e_dw, _bound('locality_scale_bwd')))
        assert e_dx < _bound('locality_scale_bwd') and e_dw < _bound('locality_scale_bwd')
        assert (gdw[:min(M, 4)] == 0).all()


# ---- optimizer kernels ----------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


def _ulps(got, want64):
    want32 = np.float32(want64)
    return abs(float(got) - float(want32)) / float(np.spacing(want32))


@pytest.mark.parametrize('start', [0, 9999])
def test_adam_advance_counts_and_corrects(hip, start):
    state = torch.tensor([float(start), 0.0], device=DEV)
    for k in range(1, 11):
        hip.adam_advance(state, LR, B1, B2)
        t, lr_t = state.cpu().numpy()
        assert t == start + k
        assert _ulps(lr_t, ref.adam_lr_t(start + k, np.float32(LR), np.float32(B1), np.float32(B2))) <= 1


def _adam_arrays(rng, n):
    w, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m, v = (rng.standard_normal(n) * 0.1).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    z = slice(0, min(n, 3))
    g[z], v[z], m[z] = 0, 0, 0                                        # v = 0, g = 0 (and l2 = 0 below for these): the update is 0, never NaN
    return w, g, m, v


def _adam_check64(got, before, parts, lr_t, l2):
    """w, m, v against float64 at the 1e-6 of test_training_kernels, per element against ref.adam_scales (the magnitudes of the element's own
    terms), not against the largest value of the array."""
    b1, b2, eps, l2 = (float(np.float32(x)) for x in (B1, B2, EPS, l2))
    parts = np.asarray(parts, dtype=np.float64).reshape(-1, before[0].size)
    want = ref.adam_step(before[0], parts.sum(0), before[1], before[2], lr_t, b1, b2, eps, l2)
    scales = ref.adam_scales(before[0], parts, before[1], before[2], lr_t, b1, b2, eps, l2)
    for name, a, b, sc in zip('wmv', got, want, scales):
        assert np.isfinite(a).all()
        err = ref.scaled_error(a, b, sc)
        assert err < 1e-6, (name, err)
    # the update itself, w' - w: to 1e-6 of the update its terms' magnitudes would give, plus the rounding of the stored w' (half an ulp)
    upd_scale = scales[0] - np.abs(before[0].astype(np.float64))
    upd_err = np.abs((got[0].astype(np.float64) - before[0]) - (want[0] - before[0]))
    assert (upd_err <= 1e-6 * upd_scale + ref.F32_EPS * np.abs(want[0])).all()


@pytest.mark.parametrize('n', [1, 1000, 2_100_003])                   # the last: above one grid pass of 8 192 x 256 elements
@pytest.mark.parametrize('l2', [0.0, 1e-3])
def test_adam_dev_reads_the_step_from_the_device(hip, n, l2):
    w, g, m, v = _adam_arrays(np.random.default_rng(n), n)
    state = torch.zeros(2, device=DEV)
    for _ in range(3):
        hip.adam_advance(state, LR, B1, B2)
    lr_t = float(state[1])
    dev = [_t(w), _t(m), _t(v)]
    hip.adam_dev(dev[0], _t(g), dev[1], dev[2], state, B1, B2, EPS, l2=l2)
    host = [_t(w), _t(m), _t(v)]
    hip.adam(host[0], _t(g), host[1], host[2], lr_t, B1, B2, EPS, l2=l2)       # the host-step form with the same lr_t: the same arithmetic
    for a, b in zip(dev, host):
        assert torch.equal(a, b)
    got = [t.cpu().numpy() for t in dev]
    _adam_check64(got, (w, m, v), g, lr_t, l2)
    assert n <= 3 or np.abs(got[0][3:] - w[3:]).max() > 0                                # (the update is not zero elsewhere)
    if l2 == 0.0:
        assert np.array_equal(got[0][:min(n, 3)], w[:min(n, 3)])


def _multi_layout():
    """Slots (n, vector path?, g_groups, l2) cut from ONE sentinel-filled buffer with gaps between them; every array of a vector slot is
    16-byte aligned with n % 4 == 0, the scalar slots have n % 4 != 0 or a w offset by one float."""
    spec = [(1, False, 0, 0.0), (1023, False, 0, 1e-3), (1024, True, 0, 1e-3), (1025, False, 1, 0.0), (4100, True, 0, 0.0), (4099, False, 0, 1e-3),
            (2048, 'offset', 0, 1e-3)]
    for groups in (1, 4, 5, 16, 17, 33):
        spec += [(1028, True, groups, 1e-3 if groups % 2 else 0.0), (1027, False, groups, 0.0 if groups % 2 else 1e-3)]
    return spec


def test_adam_multi_every_path(hip):
    """optim_multi_kernel<V_ADAM> over amar_adam_slot: vector and scalar path (by n % 4 and by alignment), block boundaries, deferred partial gradients in groups of 16
    (vector) and 4 (scalar) with their tails, slot lookup by block number, the per-block atomic into loss_acc.  Every slot equals adam_dev on
    the partial gradients summed in order 0 .. G-1 in float32 bit for bit, and float64 within 1e-6; the memory between slots is untouched."""
    rng = np.random.default_rng(11)
    spec = _multi_layout()
    GAP = 8                                                                              # floats (a multiple of 4: alignment survives)
    total = sum(4 * (n + 4 + GAP) + (max(g, 1)) * (n + 4) + GAP for n, _, g, _ in spec) + 64
    host = np.full(total, SENTINEL, dtype=np.float32)
    pos, slots = GAP, []

    def take(count, offset_one):
        nonlocal pos
        start = pos + (1 if offset_one else 0)
        pos = (start + count + GAP + 3) // 4 * 4
        return slice(start, start + count)
    for n, kind, groups, l2 in spec:
        w, g, m, v = _adam_arrays(rng, n)
        parts = np.stack([g] + [rng.standard_normal(n).astype(np.float32) for _ in range(max(groups, 1) - 1)])
        sw, sm, sv, sg = take(n, kind == 'offset'), take(n, False), take(n, False), take(max(groups, 1) * n, False)
        host[sw], host[sm], host[sv], host[sg] = w, m, v, parts.reshape(-1)
        slots.append({'n': n, 'kind': kind, 'groups': groups, 'l2': l2, 'w': sw, 'm': sm, 'v': sv, 'g': sg, 'parts': parts})
    assert pos <= total
    owned = np.zeros(total, dtype=bool)
    for s in slots:
        for key in 'wmvg':
            owned[s[key]] = True
    state = torch.zeros(2, device=DEV)
    for _ in range(5):
        hip.adam_advance(state, LR, B1, B2)
    lr_t = float(state[1])
    reg_scale = 0.5
    results = {}
    for with_loss in (False, True):
        buf = _t(host)
        entries = []
        for s in slots:
            g = buf[s['g']]
            entries.append((buf[s['w']], hip.DeferredGradient(g, s['groups'], (s['n'],)) if s['groups'] else g, buf[s['m']], buf[s['v']], s['l2']))
            vec = s['n'] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (entries[-1][0], g, entries[-1][2], entries[-1][3]))
            assert vec == (s['kind'] is True), (s['n'], s['kind'])                       # the path the slot was laid out for
        table, blocks = hip.adam_slot_table(entries)
        assert blocks == sum((s['n'] + 1023) // 1024 for s in slots)
        loss = torch.full((1,), 2.5, device=DEV) if with_loss else None
        hip.adam_multi(table.to(DEV), len(slots), blocks, state, B1, B2, EPS, reg_scale=reg_scale, loss_acc=loss)
        torch.cuda.synchronize()
        results[with_loss] = buf.cpu().numpy()
    after = results[True]
    assert np.array_equal(results[True].view(np.int32), results[False].view(np.int32))   # loss_acc = NULL changes nothing else
    assert np.array_equal(after[~owned], host[~owned])                                   # gaps and the floats before an offset w keep the sentinel
    reg64, n_blocks = 0.0, 0
    for s in slots:
        g32 = ref.sum_groups_f32(s['parts'])
        assert np.array_equal(after[s['g']], host[s['g']])                               # gradients are read only
        single = [_t(host[s[key]].copy()) for key in 'wmv']
        hip.adam_dev(single[0], _t(g32), single[1], single[2], state, B1, B2, EPS, l2=s['l2'])
        for key, t in zip('wmv', single):
            assert np.array_equal(after[s[key]].view(np.int32), t.cpu().numpy().view(np.int32)), (s['n'], s['kind'], s['groups'], key)
        _adam_check64([after[s[key]] for key in 'wmv'], tuple(host[s[key]] for key in 'wmv'), s['parts'], lr_t, s['l2'])
        if s['l2']:
            reg64 += float(np.float32(s['l2'])) * float(np.sum(host[s['w']].astype(np.float64) ** 2))
            n_blocks += (s['n'] + 1023) // 1024
    want_loss = 2.5 + reg_scale * reg64
    # n_blocks float atomics onto a growing positive sum; per block 4 fused products per lane, 6 + 3 additions of the tree, 2 products behind it
    bound = (n_blocks * 2.0 ** -24 + (4 + 6 + 3 + 2) * 2.0 ** -24) * want_loss
    got_loss = float(loss[0])
    print('loss_acc {:.9g}, float64 {:.9g}, bound {:.3g}'.format(got_loss, want_loss, bound))
    assert abs(got_loss - want_loss) <= bound


GOLDEN_ADAM = os.path.join(ROOT, 'tests', 'golden', 'adam_multi_bits.npz')


def _run_golden_adam_case(hip):
    """One amar_adam_multi_f32 launch after seven advances on seeded slots (vector / scalar path, l2, 16 and 5 deferred groups; gradients
    and second moments spread over eight decades); returns the concatenated w, m, v."""
    rng = np.random.default_rng(2025)
    state = torch.zeros(2, device=DEV)
    for _ in range(7):
        hip.adam_advance(state, LR, B1, B2)
    entries = []
    for n, l2, G in ((4096, 1e-3, 0), (1023, 1e-4, 0), (2048, 1e-3, 16), (777, 0.0, 5)):
        w = _t(rng.standard_normal(n).astype(np.float32))
        g = _t((rng.standard_normal(max(G, 1) * n) * 10.0 ** rng.uniform(-6, 0, max(G, 1) * n)).astype(np.float32))
        m = _t((rng.standard_normal(n) * 0.1).astype(np.float32))
        v = _t((rng.uniform(0, 1, n) * 10.0 ** rng.uniform(-8, 0, n)).astype(np.float32))
        entries.append((w, hip.DeferredGradient(g, G, (n,)) if G else g, m, v, l2))
    table, blocks = hip.adam_slot_table(entries)
    hip.adam_multi(table.to(DEV), len(entries), blocks, state, B1, B2, EPS)
    torch.cuda.synchronize()
    return {key: np.concatenate([e[k].cpu().numpy() for e in entries]) for key, k in (('w', 0), ('m', 2), ('v', 3))}


def test_adam_multi_keeps_the_recorded_bits(hip):
    """The Adam kernels share one update (optim_step, csrc/amar_optim.hip) whose fused products are those adam_multi_kernel — the kernel
    every fit() ran — had before the three were unified: its results equal, bit for bit, the ones recorded from the library before that
    change (tests/golden/adam_multi_bits.npz), so trained weights did not move."""
    got, want = _run_golden_adam_case(hip), np.load(GOLDEN_ADAM)
    for key in 'wmv':
        assert np.array_equal(got[key].view(np.int32), want[key].view(np.int32)), key


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 100_003])
def test_sum_into(hip, n):
    x = (np.random.default_rng(n).standard_normal(n) * 3).astype(np.float32)
    acc = torch.full((1,), 1.25, device=DEV)
    hip.sum_into(_t(x) if n else torch.empty(0, device=DEV), acc, scale=0.375)
    want = 1.25 + 0.375 * float(x.astype(np.float64).sum())
    bound = n * ref.F32_EPS * float(np.abs(x.astype(np.float64)).sum()) + 2 * ref.F32_EPS * abs(want)      # + the final product and sum
    print('n = {}: error {:.3g}, bound {:.3g}'.format(n, abs(float(acc[0]) - want), bound))
    assert abs(float(acc[0]) - want) <= bound
    if n == 0:
        assert float(acc[0]) == 1.25


@pytest.mark.parametrize('B', [1, 2, 1023, 4096, 100_001])
@pytest.mark.parametrize('strided', [False, True])
def test_bce_grad_clip_points(hip, B, strided):
    """Every clip case for both labels: p = 0, 1, 1e-7, 1 - 1.19e-7, one ulp on either side of both clip points, 0.5."""
    rng = np.random.default_rng(B)
    p = rng.uniform(0, 1, B).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    e32 = np.float32(1e-7)
    special = [np.float32(0), np.float32(1), *ref.ulp_neighbours(e32), *ref.ulp_neighbours(np.float32(1) - e32), np.float32(0.5)]
    planted = [(v, lab) for lab in (0.0, 1.0) for v in special][:B] if B > 2 else [(np.float32(0), 1.0), (np.float32(1), 0.0)][:B]
    for j, (v, lab) in enumerate(planted):
        p[j], y[j] = v, lab
    if strided:
        buf = torch.full((B, 3), SENTINEL, device=DEV)
        buf[:, 1] = _t(p)
        pd = buf[:, 1:2]
    else:
        pd = _t(p)
    dz, terms = torch.full((B, 1), float('nan'), device=DEV), torch.full((B,), float('nan'), device=DEV)
    hip.bce_grad(pd, _t(y), dz, terms)
    want_terms, want_dz = ref.bce_terms_f32(p, y)
    gt, gd = terms.cpu().numpy(), dz.cpu().numpy()[:, 0]
    assert np.isfinite(gt).all() and np.isfinite(gd).all()
    rel = lambda got, want: float(np.abs(got.astype(np.float64) - want).max() / max(1e-30, np.abs(want).max()))   # noqa: E731
    assert rel(gt, want_terms.astype(np.float64)) < 1e-5 and rel(gd, want_dz.astype(np.float64)) < 1e-5
    # ... and element by element on the planted ones, whose terms range from 6e-8 to 16
    k = len(planted)
    assert (np.abs(gt[:k].astype(np.float64) - want_terms[:k]) <= 1e-5 * np.maximum(np.abs(want_terms[:k]), 1e-2)).all()
    outside = (p < e32) | (p > np.float32(1) - e32)
    assert (gd[outside] == 0).all()
    mean64 = ref.bce_mean_loss(p, y)
    assert abs(float(gt.astype(np.float64).sum()) / B - mean64) <= 1e-6 * max(mean64, 1e-30)


COLMAX_SIZES = [0, 1, 255, 256, 257, 24_577, 590_000]                 # 24 577 > 96 blocks of 256: a second grid-stride step


def _colmax_vectors(n, rng):
    base = rng.uniform(0.5, 9.0, n).astype(np.float32)
    out = {'positive': base.copy(), 'negative': -base, 'mixed': (base - 4.0).astype(np.float32), 'all -0': np.full(n, -0.0, dtype=np.float32)}
    if n:
        first, last = -base, -base
        first, last = first.copy(), last.copy()
        first[0], last[-1] = 11.0, 11.0
        neg0, pos0 = -base, -base
        neg0, pos0 = neg0.copy(), pos0.copy()
        neg0[n // 2], pos0[n // 2] = -0.0, 0.0
        out.update({'max first': first, 'max last': last, 'negatives, one -0': neg0, 'negatives, one +0': pos0})
    return out


@pytest.mark.parametrize('n', COLMAX_SIZES)
def test_colmax_is_the_maximum(hip, n):
    """amar_colmax_f32 is the bound amar_gat_lt_f32 subtracts: >= every element and == the float maximum (IEEE comparison, so either zero
    stands for the other).  A maximum of -0.0 used to be lost (its int image is INT_MIN, which an atomicMax never stores): the result was
    -inf, or a negative below the maximum."""
    out = torch.full((1,), 123.0, device=DEV)
    for name, x in _colmax_vectors(n, np.random.default_rng(n)).items():
        hip.colmax(_t(x) if n else torch.empty(0, device=DEV), out)               # the same word every time: each call resets it in-stream
        got = float(out[0])
        want = float(x.max()) if n else -np.inf
        print('n = {}, {}: {} (max {})'.format(n, name, got, want))
        assert got == want, name
        assert n == 0 or (got >= x).all()


def test_colmax_on_another_stream_and_after_a_larger_result(hip):
    big, small = _t(np.array([5.0, 7.0, 3.0], dtype=np.float32)), _t(np.array([-3.0, -2.0, -9.0], dtype=np.float32))
    out = torch.zeros(1, device=DEV)
    hip.colmax(big, out)
    hip.colmax(small, out)                                                        # must not remember the 7
    assert float(out[0]) == -2.0
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        x = torch.full((70_001,), -1.5, device=DEV)
        x[-1] = -0.25
        hip.colmax(x, out)
    stream.synchronize()
    assert float(out[0]) == -0.25


@pytest.mark.parametrize('C', [8, 32])
def test_gat_lds_tiled_with_a_bound_of_negative_zero(hip, C):
    """test_gat_lds_tiled's case with a_neigh = +0 and H < 0: every s_neigh is -0.0, so the bound is -0.0.  The output must be finite and
    equal to the row kernel's (with the bound lost as -inf, M_i = -inf and every weight exp(+inf))."""
    from scipy import sparse
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, _unit_entries
    n = 300
    rng = np.random.default_rng(C)
    rows = np.repeat(np.arange(n), 9)
    key = np.unique(rows * n + rng.integers(0, n, len(rows)))
    a = DeviceCSR.from_scipy(sparse.coo_matrix((np.ones(len(key), np.float32), (key // n, key % n)), shape=(n, n)), with_values=False)
    r, c, diag, off = _unit_entries(a, False)
    rw = lds_tiled.GAT_ROWS_PER_WAVE[C]
    lt = lds_tiled.LdsTiled.build(r, c, n, n, C, diag, torch.ones(n, device=DEV), None, off, n_cu=3, split=64, rw=rw, split_growth=1.25)
    h = -rng.uniform(0.5, 2.0, (n, C)).astype(np.float32)
    sn = np.full(n, -0.0, dtype=np.float32)                                       # H . a_neigh with a_neigh = +0 and H < 0: a sum of negative zeros
    assert np.array_equal(np.signbit((h * np.float32(0.0))[:, 0]), np.ones(n, dtype=bool))
    assert np.signbit(sn).all() and (sn == 0).all()
    ss = rng.standard_normal(n).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, C).astype(np.float32)
    y_row, y_lt = torch.empty((n, C), device=DEV), torch.full((n, C), float('nan'), device=DEV)
    hip.gat_layer(a.rowptr, a.colidx, _t(h), _t(ss), _t(sn), _t(b), y_row, self_loop=True)
    hip.gat_lt(lt, a, _t(h), _t(ss), _t(sn), _t(b), y_lt, self_loop=True)
    got, want = y_lt.cpu().numpy(), y_row.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max())        # test_gat_lds_tiled's tolerance
