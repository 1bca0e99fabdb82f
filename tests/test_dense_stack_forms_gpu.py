"""The 16-row and 64-row forms of the one-launch Dense-stack kernels (amar_dense_stack_f32, amar_dense_stack_bwd_f32 and their pair
launchers) against float64 (tests/dense_stack_ref.py), at the smallest shapes that select each form (pytest -m gpu).

Each case first ASKS the launcher's own route function (capi.dense_stack_route / capi.dense_stack_bwd_route) and asserts the row form,
the workgroup count and the 16-byte-load flags it claims to test.  Every matrix operand and output is a column slice of a wider buffer
with PAD more rows whose slack is NaN, kernels and biases lie inside NaN-filled flat buffers, the workspace is NaN with NaN behind it:
a read outside an operand shows up in a result, a store outside an output shows up in the slack.

Bounds (dense_stack_ref; U = 2^-24), all derived from float32 summation or taken from the older stack tests, none measured here:
  forward, per layer and element, against float64 of the device's OWN previous layer:  (K + 2) U (|x| . |W| + |b|)  (none / relu),
                                                                                      3e-6  (sigmoid: __expf)
  reverse  dX0 per element; every workgroup's partial of every dW_l / db_l per element (this locates a bad tile); the error of dZ is
           carried down the chain (dense_stack_ref.reverse); reduced dW / db also helpers.rel_err < 5e-6
  against amar_dense_bwd_f32 layer by layer (the tile kernel: a second implementation): within the sum of the two bounds
  pairs    bit for bit against two single launches (the header's contract)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dense_stack_ref as ref
from tests import helpers
from tests.test_dense_bwd_routes_gpu import _host, _np, _slack_untouched, _slice, _within

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
N_SRC = 500                                                            # rows of the table a gathering case reads from


def _flat(data, misaligned):
    """(buffer, view): a contiguous array (a kernel, a bias) inside a NaN-filled flat buffer: 16 bytes in, or 8 bytes (misaligned)."""
    off = 2 if misaligned else 4
    buf = torch.full((data.size + 8,), NAN, dtype=torch.float32, device=DEV)
    view = buf[off:off + data.size].view(data.shape)
    view.copy_(_host(data))
    assert (view.data_ptr() % 16 == 0) != misaligned
    return buf, view


def _nan_slice(M, C, misaligned):
    return _slice(np.full((M, C), np.nan, np.float32), misaligned)


def _no_store_outside(pairs, what):
    for k, (buf, view) in enumerate(pairs):
        assert _slack_untouched(buf, view, NAN), '{}: a store outside output {}'.format(what, k)


# ---- forward -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def fwd_case(M, dims, acts, gather):
    rng = np.random.default_rng(7919 * M + sum(dims) + len(dims))
    L = len(acts)
    x = rng.standard_normal((N_SRC if gather else M, dims[0])).astype(np.float32)
    ids = rng.integers(0, N_SRC, M).astype(np.int32) if gather else None
    ws = [(rng.standard_normal((dims[l], dims[l + 1])) * 0.3).astype(np.float32) for l in range(L)]
    bs = [(rng.standard_normal(dims[l + 1]) * 0.1).astype(np.float32) for l in range(L)]
    for a in [x] + ws + bs:
        a.setflags(write=False)
    return dict(x=x, ids=ids, ws=ws, bs=bs, x0=x[ids] if gather else x)


class Forward:
    """The device operands of one forward case and fresh NaN outputs per call."""

    def __init__(self, M, dims, acts, gather=False, misaligned=False, xcopy=False, no_bias=(), zero_bias=()):
        self.M, self.dims, self.acts, self.misaligned = M, list(dims), list(acts), misaligned
        self.case = case = fwd_case(M, tuple(dims), tuple(acts), gather)
        self.bs = [None if l in no_bias else np.zeros_like(b) if l in zero_bias else b for l, b in enumerate(case['bs'])]
        self.x_buf, self.X = _slice(case['x'], misaligned)
        self.ids = torch.from_numpy(case['ids']).to(DEV) if gather else None
        self.W = [_flat(w, misaligned)[1] for w in case['ws']]
        self.B = [None if b is None else _flat(b, misaligned)[1] for b in self.bs]
        self.want_xcopy = xcopy

    def spec(self):
        self.outs = [_nan_slice(self.M, d, self.misaligned) for d in self.dims[1:]]
        self.xcopy = _nan_slice(self.M, self.dims[0], self.misaligned) if self.want_xcopy else None
        return dict(X=self.X, weights=self.W, biases=self.B, acts=self.acts, outs=[v for _, v in self.outs], ids=self.ids,
                    xcopy=self.xcopy[1] if self.xcopy else None)

    def verify(self, what):
        """Every layer against float64 of the device's own previous layer; Xcopy exact; nothing stored outside the outputs."""
        cur = self.case['x0']
        if self.xcopy:
            assert np.array_equal(self.xcopy[1].cpu().numpy(), cur), what + ': Xcopy is the gathered rows'
            _no_store_outside([self.xcopy], what + ' Xcopy')
        for l, act in enumerate(self.acts):
            got = self.outs[l][1].cpu().numpy()
            want, bound = ref.forward_layer(cur, self.case['ws'][l], self.bs[l], act)
            _within('{} layer {}'.format(what, l), got.astype(np.float64), want, bound)
            cur = got
        _no_store_outside(self.outs, what)

    def bits(self):
        return [v.clone() for _, v in self.outs] + ([self.xcopy[1].clone()] if self.xcopy else [])


def check_forward(hip, fwd, expect):
    spec = fwd.spec()
    route = hip.dense_stack_route(**spec)
    print('route', route)
    assert {k: route[k] for k in expect} == expect, route
    hip.dense_stack(**spec)
    fwd.verify('first')
    first = fwd.bits()
    hip.dense_stack(**fwd.spec())
    assert all(torch.equal(a, b) for a, b in zip(first, fwd.bits())), 'called twice: identical bits'
    return first


LDS_128 = 4 * (2 * 64 * 130 + 128 * 130)                               # four layers of 128 columns: the largest request


@pytest.mark.parametrize('M,dims,acts,kwargs,expect', [
    (4097, [24, 24, 24], ['relu', 'relu'], dict(gather=True, xcopy=True), dict(rows=64, groups=65, vec_x=True, vec_w=[True, True])),
    (4097, [5, 7, 3], ['sigmoid', None], dict(), dict(rows=64, groups=65, vec_x=False, vec_w=[False, False])),
    (4097, [24, 24, 24], ['relu', 'relu'], dict(gather=True, xcopy=True, misaligned=True), dict(rows=64, groups=65, vec_x=False, vec_w=[False, False])),
    (4097, [128] * 5, ['relu', 'relu', 'relu', None], dict(), dict(rows=64, groups=65, vec_x=True, vec_w=[True] * 4, lds_bytes=LDS_128)),
    (4096, [96, 64, 64, 1], ['relu', 'relu', 'sigmoid'], dict(), dict(rows=16, groups=256, vec_x=True, vec_w=[True, True, False])),
    (17, [48, 48], ['relu'], dict(), dict(rows=16, groups=2, vec_x=True, vec_w=[True])),
    (4097, [48, 48], [None], dict(), dict(rows=64, groups=65, vec_x=True, vec_w=[True]))],
    ids=['64rows-gather-xcopy', '64rows-scalar-hidden-sigmoid', '64rows-misaligned', '64rows-4x128', '16rows-4096', '16rows-one-layer', '64rows-one-layer'])
def test_forward_forms(hip, M, dims, acts, kwargs, expect):
    """(M = 4 097: 65 workgroups of 64 rows, the last with ONE live row; M = 4 096: the other side of the threshold.)"""
    check_forward(hip, Forward(M, dims, acts, **kwargs), expect)


def test_forward_null_bias_is_a_zero_bias(hip):
    """bias[1] == NULL (include/amar_hip.h: a zero bias): the same bits as a vector of zeros, both within the bounds."""
    expect = dict(rows=16, groups=5, vec_x=True, vec_w=[True, True])
    null = check_forward(hip, Forward(65, [16, 48, 48], ['relu', 'relu'], no_bias=(1,)), expect)
    zero = check_forward(hip, Forward(65, [16, 48, 48], ['relu', 'relu'], zero_bias=(1,)), expect)
    assert all(torch.equal(a, b) for a, b in zip(null, zero))


# ---- reverse -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def bwd_case(M, dims, acts):
    """Float32 operands (read-only): kernels, the saved activations of a float32 forward pass with edge values planted, a top gradient.
    The top gradient is drawn around 0.5, not around 0: helpers.rel_err measures a reduced gradient against the size of the RESULT, and
    with top_is_dz the bias gradient of a one-column last layer is the plain sum of the top gradient.  Zero-mean draws made that a
    cancelling sum (M = 2 048: sum 0.375 against sum of magnitudes 1 611.5 in float64), where float32 arithmetic that is correct to
    4e-9 of the magnitudes is 1.8e-5 of the result and 5e-6 cannot hold; the per-element bounds, taken against the magnitudes, do not
    depend on this."""
    rng = np.random.default_rng(104729 * M + sum(dims) + len(dims))
    L = len(acts)
    ws = [(rng.standard_normal((dims[l], dims[l + 1])) * 0.3).astype(np.float32) for l in range(L)]
    xs = [rng.standard_normal((M, dims[0])).astype(np.float32)]
    for l, act in enumerate(acts):
        y = ref.activate(xs[-1].astype(np.float64) @ ws[l] + rng.standard_normal(dims[l + 1]) * 0.1, act).astype(np.float32)
        if act == 'relu':                                              # an exact zero, a negative zero (no gradient through either), a plain value
            y.flat[0], y.flat[-1] = -0.0, 0.0
            assert np.signbit(y.flat[0]) and (y == 0).sum() >= 2
            if y.size > 2:
                y.flat[1] = 0.75
        elif act == 'sigmoid':                                         # saturated: sigmoid' is exactly 0 at both
            y.flat[0], y.flat[-1] = 1.0, 0.0
        xs.append(y)
    top = (rng.standard_normal((M, dims[-1])) + 0.5).astype(np.float32)
    for a in ws + xs + [top]:
        a.setflags(write=False)
    return dict(ws=ws, xs=xs, top=top)


@functools.lru_cache(maxsize=2)
def bwd_want(M, dims, acts, top_is_dz, rows):
    """The float64 reverse pass with its bounds, and per layer the partials of `rows`-row workgroups and of the tile kernel's 64."""
    case = bwd_case(M, dims, acts)
    want = ref.reverse(case['xs'], case['ws'], list(acts), case['top'], top_is_dz)
    want['parts'] = [ref.partials(case['xs'][l], want['dz'][l], want['err'][l], rows) for l in range(len(acts))]
    want['parts64'] = want['parts'] if rows == 64 else [ref.partials(case['xs'][l], want['dz'][l], want['err'][l], 64) for l in range(len(acts))]
    return want


class Reverse:
    def __init__(self, M, dims, acts, top_is_dz, misaligned=False):
        self.M, self.dims, self.acts, self.top_is_dz, self.misaligned = M, list(dims), list(acts), top_is_dz, misaligned
        self.L = len(acts)
        self.case = case = bwd_case(M, tuple(dims), tuple(acts))
        self.ins = [_slice(x, misaligned)[1] for x in case['xs'][:-1]]
        self.ytop = None if top_is_dz else _slice(case['xs'][-1], misaligned)[1]
        self.top = _slice(case['top'], misaligned)[1]
        self.W = [_flat(w, misaligned)[1] for w in case['ws']]

    def spec(self, hip, dx0=True, defer=False):
        """Fresh NaN outputs and a NaN workspace with NaN behind it."""
        floats = hip.dense_stack_bwd_workspace(self.M, self.dims, DEV).numel()
        self.wk_buf = torch.full((floats + 64,), NAN, dtype=torch.float32, device=DEV)
        self.dx0 = _nan_slice(self.M, self.dims[0], self.misaligned) if dx0 else None
        return dict(dYtop=self.top, Ytop=self.ytop, inputs=self.ins, weights=self.W, acts=self.acts, workspace=self.wk_buf[:floats],
                    dWs=[torch.full((self.dims[l], self.dims[l + 1]), NAN, device=DEV) for l in range(self.L)],
                    dbs=[torch.full((self.dims[l + 1],), NAN, device=DEV) for l in range(self.L)], dX0=self.dx0[1] if dx0 else None, defer=defer)

    def workspace_kept(self, spec):
        """Every partial written, nothing behind the workspace."""
        floats = spec['workspace'].numel()
        return bool(torch.isnan(self.wk_buf[floats:]).all()) and not bool(torch.isnan(self.wk_buf[4:floats]).any())


def check_reverse(hip, M, dims, acts, top_is_dz, expect, misaligned=False):
    rv = Reverse(M, dims, acts, top_is_dz, misaligned)
    L = rv.L
    # the route, asserted
    eager = rv.spec(hip)
    route = hip.dense_stack_bwd_route(**eager)
    print('route', route)
    assert {k: route[k] for k in expect} == expect, route
    rows, G = route['rows'], route['groups']
    assert G == -(-M // rows) == int(hip.load().amar_dense_stack_bwd_groups(M))
    want = bwd_want(M, tuple(dims), tuple(acts), top_is_dz, rows)
    # eager: dX0 per element, reduced gradients
    assert hip.dense_stack_bwd(**eager) is None
    dx0_first = rv.dx0
    _within('dX0', _np(dx0_first[1]), want['dx0'], want['dx0_bound'])
    _no_store_outside([dx0_first], 'dX0')
    assert rv.workspace_kept(eager), 'eager: the workspace'
    for l in range(L):
        dw, dw_b, db, db_b, dw_mag, db_mag = want['parts'][l]
        for name, got, parts in (('dW', eager['dWs'][l], dw), ('db', eager['dbs'][l], db)):
            assert not bool(torch.isnan(got).any()), (name, l)
            e = helpers.rel_err(_np(got), parts.sum(0))
            print('layer {} reduced {}: rel_err {:.3e}'.format(l, name, e))
            assert e < ref.REDUCED_TOL, (name, l)
    # deferred: every workgroup's partial of every layer, per element; added in group order they are the reduced gradients, bit for bit
    lazy_spec = rv.spec(hip, defer=True)
    lazy = hip.dense_stack_bwd(**lazy_spec)
    assert rv.workspace_kept(lazy_spec), 'deferred: the workspace'
    assert torch.equal(rv.dx0[1], dx0_first[1])
    _no_store_outside([rv.dx0], 'deferred dX0')
    assert len(lazy) == L
    for l in range(L):
        dw, dw_b, db, db_b, dw_mag, db_mag = want['parts'][l]
        lw, lb = lazy[l]
        assert lw.groups == lb.groups == G
        _within('layer {} dW partials'.format(l), _np(lw.partials).reshape(dw.shape), dw, dw_b)
        _within('layer {} db partials'.format(l), _np(lb.partials).reshape(db.shape), db, db_b)
        assert torch.equal(lw.materialize(), eager['dWs'][l]) and torch.equal(lb.materialize(), eager['dbs'][l]), l
        assert bool(torch.isnan(lazy_spec['dWs'][l]).all()) and bool(torch.isnan(lazy_spec['dbs'][l]).all()), 'defer: dW / db themselves are not written'
    # a second call: identical bits
    again = rv.spec(hip)
    hip.dense_stack_bwd(**again)
    assert torch.equal(rv.dx0[1], dx0_first[1])
    assert all(torch.equal(a, b) for a, b in zip(again['dWs'] + again['dbs'], eager['dWs'] + eager['dbs'])), 'called twice: identical bits'
    # without dX0 (W_0 is not even staged): the same partials, bit for bit
    nodx_spec = rv.spec(hip, dx0=False, defer=True)
    nodx = hip.dense_stack_bwd(**nodx_spec)
    assert rv.workspace_kept(nodx_spec), 'no dX0: the workspace'
    for l in range(L):
        assert torch.equal(nodx[l][0].partials, lazy[l][0].partials) and torch.equal(nodx[l][1].partials, lazy[l][1].partials), l
    # the same stack layer by layer through amar_dense_bwd_f32 (the 64-row tile kernel): within the sum of the two bounds
    g = rv.top
    G64 = -(-M // 64)
    for l in range(L - 1, -1, -1):
        K, N = dims[l], dims[l + 1]
        act = None if (top_is_dz and l == L - 1) else acts[l]
        y = (rv.ytop if l == L - 1 else rv.ins[l + 1]) if act is not None else None
        dx, dw2, db2 = torch.empty((M, K), device=DEV), torch.empty((K, N), device=DEV), torch.empty(N, device=DEV)
        ws1 = hip.dense_bwd_workspace(M, K, N, DEV)
        assert hip.dense_bwd_route(rv.ins[l], y, g, rv.W[l], act, ws1, dX=dx, dW=dw2, db=db2)['kernel'] == 'tile'
        hip.dense_bwd(rv.ins[l], y, g, rv.W[l], act, ws1, dX=dx, dW=dw2, db=db2)
        dw, dw_b, db, db_b, dw_mag, db_mag = want['parts'][l]
        t = want['parts64'][l]
        _within('layer {} dW against the tile kernel'.format(l), _np(eager['dWs'][l]), _np(dw2),
                ref.reduced_bound(dw_b, dw_mag, G) + ref.reduced_bound(t[1], t[4], G64))
        _within('layer {} db against the tile kernel'.format(l), _np(eager['dbs'][l]), _np(db2),
                ref.reduced_bound(db_b, db_mag, G) + ref.reduced_bound(t[3], t[5], G64))
        g = dx
    _within('dX0 against the tile kernel', _np(dx0_first[1]), _np(g), 2 * want['dx0_bound'])


def ALL(n, v=True):
    return [v] * n


REVERSE_CASES = [
    (1025, [24, 24, 24], ['relu', 'relu'], False, dict(rows=64, groups=17, vec_top=True, vec_x=ALL(2), vec_w=ALL(2))),
    (1025, [5, 7, 3], ['sigmoid', None], False, dict(rows=64, groups=17, vec_top=False, vec_x=ALL(2, False), vec_w=ALL(2, False))),
    (1025, [24, 24, 24], ['relu', 'relu'], True, dict(rows=64, groups=17, vec_top=False, vec_x=ALL(2, False), vec_w=ALL(2, False))),
    (4096, [128] * 5, ['relu', 'relu', 'relu', None], False, dict(rows=64, groups=64, vec_top=True, vec_x=ALL(4), vec_w=ALL(4), lds_bytes=LDS_128)),
    (2048, [96, 64, 64, 1], ['relu', 'relu', 'sigmoid'], False, dict(rows=64, groups=32, vec_top=False, vec_x=ALL(3), vec_w=[True, True, False])),
    (1024, [48, 48, 48, 48, 1], ['relu', 'relu', 'relu', 'sigmoid'], False, dict(rows=16, groups=64, vec_top=False, vec_x=ALL(4), vec_w=[True, True, True, False])),
    (17, [48, 48], ['relu'], False, dict(rows=16, groups=2, vec_top=True, vec_x=ALL(1), vec_w=ALL(1))),
    (1025, [48, 48], ['relu'], False, dict(rows=64, groups=17, vec_top=True, vec_x=ALL(1), vec_w=ALL(1)))]


@pytest.mark.parametrize('top_is_dz', [False, True], ids=['ytop', 'top-is-dz'])
@pytest.mark.parametrize('M,dims,acts,misaligned,expect', REVERSE_CASES,
                         ids=['64rows-last-group-one-row', '64rows-scalar-hidden-sigmoid', '64rows-misaligned', '64rows-4x128-8-dxa-tiles', '64rows-mixed-vec_w',
                              '16rows-1024', '16rows-one-layer', '64rows-one-layer'])
def test_reverse_forms(hip, M, dims, acts, misaligned, expect, top_is_dz):
    """(M = 1 025: 17 workgroups of 64 rows, the last with ONE live row; M = 1 024: the other side of the threshold; each with a strided
    dX0 and with dX0 = None, with Ytop and with the top gradient already taken w.r.t. the pre-activation.)"""
    check_reverse(hip, M, dims, acts, top_is_dz, expect, misaligned=misaligned)


# ---- pairs: bit for bit against two single launches -----------------------------------------------------------------------------
def _forward_pair(hip, a, b, rows_single, rows_pair):
    """Two Forward cases as two launches and as one; the pair's row form from the two single routes by the header's rule."""
    sa, sb = a.spec(), b.spec()
    ra, rb = hip.dense_stack_route(**sa)['rows'], hip.dense_stack_route(**sb)['rows']
    assert (ra, rb) == rows_single and (16 if ra == rb == 16 else 64) == rows_pair
    hip.dense_stack(**sa)
    hip.dense_stack(**sb)
    a.verify('single 0')
    b.verify('single 1')
    singles = a.bits() + b.bits()
    hip.dense_stack_pair(a.spec(), b.spec())
    a.verify('pair 0')
    b.verify('pair 1')
    assert all(torch.equal(x, y) for x, y in zip(singles, a.bits() + b.bits())), 'the pair equals two launches, bit for bit'


def test_forward_pair_both_64_rows(hip):
    _forward_pair(hip, Forward(4097, [24, 24, 24], ['relu', 'relu'], gather=True, xcopy=True),
                  Forward(4097, [16, 48, 48], ['relu', None], gather=True, xcopy=True), (64, 64), 64)


def test_forward_pair_mixed_rows_runs_64(hip):
    """M = 300 alone runs 16-row workgroups, in a pair with M = 4 097 64-row ones: a sum's order (ascending k) does not depend on the row
    form, so the bits must not either."""
    _forward_pair(hip, Forward(300, [96, 64, 32, 48], ['relu', 'relu', None]),
                  Forward(4097, [24, 24, 24], ['relu', 'relu'], gather=True, xcopy=True), (16, 64), 64)


def test_forward_pair_with_an_empty_first_stack(hip):
    """M = 0 with M = 17 (split = 0: every workgroup belongs to the second stack).  Through the C entry: an empty tensor has no address."""
    lib = hip.load()
    a, b = Forward(17, [24, 24, 24], ['relu', 'relu']), Forward(17, [48, 48], ['relu'])
    sb = b.spec()
    hip.dense_stack(**sb)
    b.verify('single')
    single = b.bits()
    args_a, args_b = hip._dense_stack_args(**a.spec()), hip._dense_stack_args(**b.spec())
    args_a[-1] = 0                                                     # the first stack: real operands, no rows
    info = hip.DenseStackRouteInfo()
    assert lib.amar_dense_stack_route(*args_a, ctypes.byref(info)) == 0 and info.groups == 0
    d0, d1 = hip.DenseStackDesc(*[hip._as_pointer(v) for v in args_a]), hip.DenseStackDesc(*[hip._as_pointer(v) for v in args_b])
    assert lib.amar_dense_stack_pair_f32(ctypes.byref(d0), ctypes.byref(d1), None) == 0
    b.verify('pair')
    assert all(torch.equal(x, y) for x, y in zip(single, b.bits()))
    assert all(bool(torch.isnan(buf).all()) for buf, _ in a.outs), 'a stack without rows stores nothing'
    assert lib.amar_dense_stack_f32(*args_a, None) == 0


@pytest.mark.parametrize('M,first,second', [(1025, ([24, 24, 24], ['relu', 'relu']), ([5, 7, 3], ['sigmoid', None])),
                                            (2048, ([16, 48, 48], ['relu', 'relu']), ([96, 64, 32, 48], ['relu', 'relu', None]))])
@pytest.mark.parametrize('defer', [False, True], ids=['eager', 'deferred'])
def test_reverse_pair_64_rows(hip, M, first, second, defer):
    a, b = Reverse(M, first[0], first[1], False), Reverse(M, second[0], second[1], False)
    sa, sb = a.spec(hip, defer=defer), b.spec(hip, defer=defer)
    assert hip.dense_stack_bwd_route(**sa)['rows'] == hip.dense_stack_bwd_route(**sb)['rows'] == 64
    la, lb = hip.dense_stack_bwd(**sa), hip.dense_stack_bwd(**sb)
    dxa, dxb = a.dx0, b.dx0
    pa, pb = a.spec(hip, defer=defer), b.spec(hip, defer=defer)
    qa, qb = hip.dense_stack_bwd_pair(pa, pb)
    assert a.workspace_kept(pa) and b.workspace_kept(pb)
    _no_store_outside([a.dx0, b.dx0], 'pair dX0')
    assert not bool(torch.isnan(dxa[1]).any()) and torch.equal(dxa[1], a.dx0[1]) and torch.equal(dxb[1], b.dx0[1])
    if defer:
        for single, pair in ((la, qa), (lb, qb)):
            for (w1, b1), (w2, b2) in zip(single, pair):
                assert w1.groups == w2.groups == -(-M // 64) and torch.equal(w1.partials, w2.partials) and torch.equal(b1.partials, b2.partials)
    else:
        assert qa is None and qb is None
        for s, p in ((sa, pa), (sb, pb)):
            for x, y in zip(s['dWs'] + s['dbs'], p['dWs'] + p['dbs']):
                assert not bool(torch.isnan(x).any()) and torch.equal(x, y)
