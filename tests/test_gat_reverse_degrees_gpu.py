"""GPU: the one-head GAT forward with attention dropout and the reverse pass (gat_bwd_target_kernel / gat_bwd_source_kernel through their
four entry points) on tests/gat_reverse_ref.py:degree_graph, whose row and column lengths sit one below, on and one above every stride of
the walks (64 for the softmax statistics, 64 / LPN for the edge walk), with a 300-entry row whose 260 parallel entries wrap the dropout
ordinal, empty rows and a short last workgroup (pytest -m gpu).

Every element is compared with float64 autograd by tests/entry_point_ref.py:scaled_error under the scales of gat_reverse_ref's
docstring.  The bound is min(FACTOR times the error the float32 torch restatement leaves on the same inputs, the project's whole-array
cap); FACTOR = entry_point_ref.KERNEL_FACTOR = 4.  The whole-array criteria of the older GAT tests are asserted as well.

MEASURED on an MI355X, worst scaled error over the 56 cases and the class of the row it fell on (gat_reverse_ref.row_class: 'hub row' is
the 300-entry row, 'hub column' node 20, which its 260 parallel entries point at): y 1.03e-06 (hub row), dH 8.17e-07 (hub column),
ds 8.14e-08 (hub column), dt 1.54e-07 (ladder); the float32 restatement's worst figures on the same cases: gat_reverse_ref.F32_FIGURES.
No case needed more than FACTOR = 4."""
import numpy as np
import pytest
import torch

from tests import gat_reverse_ref as ref
from tests.entry_point_ref import scaled_error
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -12345.625
PAD = 4                                                               # guard columns on either side: 16 bytes, leading dimension C + 8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sliced(a=None, shape=None, fill=float('nan')):
    """(view [n, C] at column PAD of a [n, C + 2 PAD] buffer full of SENT, the buffer): `a` copied in, or `fill`."""
    n, C = a.shape if a is not None else shape
    buf = torch.full((n, C + 2 * PAD), SENT, device=DEV)
    view = buf[:, PAD:PAD + C]
    if a is not None:
        view.copy_(_t(a))
    else:
        view.fill_(fill)
    return view, buf


def _guards_intact(view, buf):
    C = view.shape[1]
    return bool((buf[:, :PAD] == SENT).all() and (buf[:, PAD + C:] == SENT).all())


@pytest.fixture(scope='module')
def graphs():
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    out = {}
    for directed in (False, True):
        m, tgt, src = ref.degree_graph(directed)
        a = DeviceCSR.from_scipy(m, with_values=False, drop_diagonal=True)
        assert np.array_equal(a.colidx.cpu().numpy(), src) and a.nnz == len(tgt)
        at = a.transposed()
        assert (at is a) == (not directed)
        out[directed] = (a, at)
    return out


def _reverse(hip, a, transposed, H, ss, sn, Y, dY, bias, a_s, a_n, self_loop, drop):
    """One call of the entry point the arguments select, into outputs that start as NaN; dH is a column slice (lddh = C + 8).
    Returns ({'dout', 'ds', 'dt', 'dH'} as device tensors, dH's buffer)."""
    n, C = H.shape
    nan = float('nan')
    dout, scratch = torch.full((n, C), nan, device=DEV), torch.full((3 * n,), nan, device=DEV)
    ds, dt = torch.full((n,), nan, device=DEV), torch.full((n,), nan, device=DEV)
    dH, dh_buf = _sliced(shape=(n, C))
    name = 'amar_gat_bwd' + ('_directed' if transposed is not None else '') + ('_dropout' if drop is not None else '') + '_f32'
    f32, i32 = torch.float32, torch.int32
    t_ptrs = () if transposed is None else (hip._ptr(transposed.rowptr, i32, 't_rowptr'), hip._ptr_entries(transposed.colidx, i32, 't_colidx'))
    assert transposed is None or (transposed.rowptr.numel() == n + 1 and transposed.colidx.numel() == a.colidx.numel())
    assert a.rowptr.numel() == n + 1 and all(tuple(v.shape) == (n, C) for v in (Y, dY)) and min(ss.numel(), sn.numel()) >= n
    assert all(v.numel() == C and v.is_contiguous() for v in (bias, a_s, a_n))
    code = getattr(hip.load(), name)(
        hip._ptr(a.rowptr, i32, 'rowptr'), hip._ptr_entries(a.colidx, i32, 'colidx'), *t_ptrs, hip._ptr(H, f32, 'H'), hip._ld(H, 'H'), C,
        hip._ptr(ss, f32, 's_self'), hip._ptr(sn, f32, 's_neigh'), hip._ptr(Y, f32, 'Y'), hip._ld(Y, 'Y'), hip._ptr(dY, f32, 'dY'), hip._ld(dY, 'dY'),
        hip._ptr(bias, f32, 'bias'), hip._ptr(a_s, f32, 'a_self'), hip._ptr(a_n, f32, 'a_neigh'), hip._ptr(dout), hip._ptr(scratch), hip._ptr(ds),
        hip._ptr(dt), hip._ptr(dH), hip._ld(dH, 'dH'), 1 if self_loop else 0, n, *(drop._args() if drop is not None else ()), hip._stream())
    hip._check(code, name)
    return {'dout': dout, 'ds': ds, 'dt': dt, 'dH': dH}, dh_buf


def _worst(got, want, scale, classes):
    """(scaled_error, class of the row of the worst live element)."""
    rel = np.abs(np.asarray(got, dtype=np.float64) - want) / np.where(scale > 0, scale, np.inf)
    return scaled_error(got, want, scale), classes[np.unravel_index(rel.argmax(), rel.shape)[0]]


@pytest.mark.parametrize('C', ref.WIDTHS)
@pytest.mark.parametrize('self_loop', [True, False])
@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('rate', [None, ref.DROP_RATE])
def test_forward_and_reverse_on_the_degree_ladder(hip, graphs, C, self_loop, directed, rate):
    a, at = graphs[directed]
    n = ref.N
    case = ref.case(C, self_loop, directed, rate)
    h, a_s, a_n, bias, dy = case['inputs']
    want, classes = case['want'], ref.row_class(directed)
    bound = {q: min(case['bound'][q], ref.CAP_FORWARD if q == 'y' else ref.CAP_GRADIENT) for q in ref.QUANTITIES}
    ss, sn = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.rowwise_xw(_t(h), torch.eye(C, device=DEV).contiguous(), torch.empty((n, C), device=DEV), a_self=_t(a_s), a_neigh=_t(a_n), s_self=ss, s_neigh=sn)
    (H, h_buf), (Y, y_buf), (dY, dy_buf) = _sliced(h), _sliced(shape=(n, C)), _sliced(dy)
    b_d, as_d, an_d = _t(bias), _t(a_s), _t(a_n)
    step = torch.full((1,), ref.DROP_STEP, dtype=torch.int64, device=DEV)
    drop = None if rate is None else hip.Dropout(ref.DROP_SEED, step, ref.DROP_SITE, rate)
    # ---- forward
    if drop is None:
        hip.gat_layer(a.rowptr, a.colidx, H, ss, sn, b_d, Y, self_loop=self_loop)
    else:
        hip.gat_layer_dropout(a.rowptr, a.colidx, H, ss, sn, b_d, Y, drop, self_loop=self_loop)
    y = Y.cpu().numpy()
    err_y, where_y = _worst(y, want['y'], want['scale_y'], classes)
    print('C', C, 'self_loop', self_loop, 'directed', directed, 'rate', rate, '| y', '%.2e' % err_y, where_y, 'bound %.2e' % bound['y'])
    assert err_y <= bound['y'] and rel_err(y, want['y']) < 1e-5
    assert _guards_intact(Y, y_buf) and _guards_intact(H, h_buf)
    if not self_loop:
        empty = np.diff(a.rowptr.cpu().numpy()) == 0
        assert empty.sum() >= 10 and np.array_equal(y[empty], np.broadcast_to(np.maximum(bias, 0), y[empty].shape))
    # ---- reverse
    run = lambda d=drop, tr=(at if directed else None): _reverse(hip, a, tr, H, ss, sn, Y, dY, b_d, as_d, an_d, self_loop, d)      # noqa: E731
    got, dh_buf = run()
    assert _guards_intact(got['dH'], dh_buf) and _guards_intact(dY, dy_buf) and _guards_intact(Y, y_buf)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(host['dout'], dy * (y > 0))
    for q in ('dH', 'ds', 'dt'):
        err, where = _worst(host[q], want[q], want['scale_' + q], classes)
        print('   ', q, '%.2e' % err, where, 'bound %.2e' % bound[q], 'float32 restatement %.2e' % case['f32'][q])
        assert err <= bound[q], (q, err, where)
    assert np.abs(host['dH'] - want['dH']).max() <= 2e-4 * np.abs(want['dH']).max()
    whole = max(np.abs(want['ds']).max(), np.abs(want['dt']).max())
    assert np.abs(host['ds'] - want['ds']).max() <= 2e-4 * whole and np.abs(host['dt'] - want['dt']).max() <= 2e-4 * whole
    again, _ = run()
    assert all(torch.equal(got[k], again[k]) for k in got)                                                   # no float atomics
    if not directed:
        twice, _ = run(tr=a)                                        # one structure through the directed entry point: the same bits
        assert all(torch.equal(got[k], twice[k]) for k in got)
    if rate is None:
        # rate 0 through the dropout entry point: the criterion of test_dropout_gpu.py:test_gat_bwd_with_attention_dropout
        zero, _ = run(d=hip.Dropout(ref.DROP_SEED, step, ref.DROP_SITE, 0.0))
        for k in got:
            assert float((got[k] - zero[k]).abs().max()) <= 1e-5 * float(got[k].abs().max()) + 1e-12, k
        # a second implementation: the multi-head kernels with one head share no code with these below the entry point
        S = torch.stack([ss, sn], dim=1).contiguous()
        dout2, dS2, dH2 = hip.gat_heads_bwd(a.rowptr, a.colidx, H, 1, S, Y, dY, b_d, as_d.view(C, 1, 1), an_d.view(C, 1, 1), concat=True,
                                            self_loop=self_loop, transposed=(at.rowptr, at.colidx) if directed else None)
        assert torch.equal(dout2, got['dout'])
        for q, other in (('dH', dH2), ('ds', dS2[:, 0]), ('dt', dS2[:, 1])):
            assert scaled_error(other.cpu().numpy(), host[q].astype(np.float64), want['scale_' + q]) <= 2 * bound[q], q
    assert int(step.item()) == ref.DROP_STEP


@pytest.mark.parametrize('C', [8, 64])
def test_single_node_and_graphs_without_entries(hip, C):
    """n = 1 and n = 5 with an empty colidx through all four entry points; n = 0 returns without a launch.  The bound is FACTOR times the
    float32 restatement's error as elsewhere, with a floor of FACTOR unit roundoffs (4 * 2^-24) of the element's scale: on a graph of one
    term per row the restatement can come out exact, and a kernel may still round each of its few operations once.  With the self loop
    every softmax has one term and ds = dt = 0 up to the rounding of d alpha_ii and c_i, which cancel: held to that floor-or-bound times
    their scale directly, besides the comparison with the reference (whose own values are the denominator's 1e-9 of d alpha)."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    rng = np.random.default_rng(C)
    a_s, a_n = ((rng.standard_normal(C) * 0.7 / np.sqrt(C)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.1, 0.3, C).astype(np.float32)
    step = torch.full((1,), ref.DROP_STEP, dtype=torch.int64, device=DEV)
    for n in (1, 5):
        a = DeviceCSR(torch.zeros(n + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, (n, n))
        h = (rng.standard_normal((n, C)) * 0.7 + 0.2).astype(np.float32)
        dy = rng.standard_normal((n, C)).astype(np.float32)
        ss, sn = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        hip.rowwise_xw(_t(h), torch.eye(C, device=DEV).contiguous(), torch.empty((n, C), device=DEV), a_self=_t(a_s), a_neigh=_t(a_n), s_self=ss, s_neigh=sn)
        (H, _), (dY, _) = _sliced(h), _sliced(dy)
        none = np.zeros(0, dtype=np.int64)
        for self_loop in (True, False):
            T, S, _ = ref.with_self_loops(none, none, n, self_loop)
            for rate in (None, 0.0, ref.DROP_RATE):
                ks = ref.edge_masks(none, none, n, self_loop, rate) if rate else None
                want = ref.gat_reverse64(h, a_s, a_n, bias, dy, T, S, n, ks)
                f32 = ref.errors(ref.gat_reverse32(h, a_s, a_n, bias, dy, T, S, n, ks), want)
                drop = None if rate is None else hip.Dropout(ref.DROP_SEED, step, ref.DROP_SITE, rate)
                Y, y_buf = _sliced(shape=(n, C))
                if drop is None:
                    hip.gat_layer(a.rowptr, a.colidx, H, ss, sn, _t(bias), Y, self_loop=self_loop)
                else:
                    hip.gat_layer_dropout(a.rowptr, a.colidx, H, ss, sn, _t(bias), Y, drop, self_loop=self_loop)
                y = Y.cpu().numpy()
                # (a graph of one term per row leaves the restatement next to no error: FACTOR unit roundoffs as the floor)
                assert scaled_error(y, want['y'], want['scale_y']) <= max(ref.FACTOR * f32['y'], 4 * 2.0 ** -24) and _guards_intact(Y, y_buf)
                for tr in (None, a):
                    got, dh_buf = _reverse(hip, a, tr, H, ss, sn, Y, dY, _t(bias), _t(a_s), _t(a_n), self_loop, drop)
                    host = {k: v.cpu().numpy() for k, v in got.items()}
                    assert _guards_intact(got['dH'], dh_buf) and np.array_equal(host['dout'], dy * (y > 0))
                    if not self_loop:
                        assert not host['dH'].any() and not host['ds'].any() and not host['dt'].any()
                        continue
                    # one term per softmax: ds = dt = 0 up to the rounding of the two numbers that cancel; dH = g + ds a_s + dt a_n
                    for q in ('dH', 'ds', 'dt'):
                        assert scaled_error(host[q], want[q], want['scale_' + q]) <= max(ref.FACTOR * f32[q], 4 * 2.0 ** -24), (q, n, rate)
                    assert np.abs(want['ds']).max() < 1e-7 and np.abs(want['dt']).max() < 1e-7
                    for q in ('ds', 'dt'):
                        limit = max(ref.FACTOR * f32[q], 4 * 2.0 ** -24) * want['scale_' + q] + np.abs(want[q])
                        assert (np.abs(host[q]) <= limit).all(), (q, n, rate)
    # n = 0: no launch, nothing written
    a = DeviceCSR(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, (0, 0))
    lib, f32t, i32 = hip.load(), torch.float32, torch.int32
    buf = {k: torch.full((4, C), float('nan'), device=DEV) for k in ('H', 'Y', 'dY', 'dout', 'dH', 'scratch')}
    vec = {k: torch.full((C,), float('nan'), device=DEV) for k in ('ss', 'sn', 'bias', 'a_s', 'a_n', 'ds', 'dt')}
    code = lib.amar_gat_bwd_f32(hip._ptr(a.rowptr, i32), hip._ptr_entries(a.colidx, i32, 'colidx'), hip._ptr(buf['H'], f32t), C, C, hip._ptr(vec['ss']),
                                hip._ptr(vec['sn']), hip._ptr(buf['Y']), C, hip._ptr(buf['dY']), C, hip._ptr(vec['bias']), hip._ptr(vec['a_s']),
                                hip._ptr(vec['a_n']), hip._ptr(buf['dout']), hip._ptr(buf['scratch']), hip._ptr(vec['ds']), hip._ptr(vec['dt']),
                                hip._ptr(buf['dH']), C, 1, 0, hip._stream())
    assert code == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in list(buf.values()) + list(vec.values()))
