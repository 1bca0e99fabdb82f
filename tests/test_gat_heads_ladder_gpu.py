"""GPU: the multi-head GAT kernels (amar_rowwise_xw_heads_f32, amar_gat_heads_f32, amar_gat_heads_bwd_f32) on
tests/gat_heads_ladder_ref.py:ladder_graph, whose row and column lengths sit one below, on and one above every stride of the walks (64 / LPN
entries per trip of the edge walk, NS * CQ of pass 1, 24 of the heads of 3 and 6 quads among them), per element and per head, and with
every head's maximum planted at a position of its own (pytest -m gpu).

Every element of S, y, dHd, ds and dt is compared with float64 autograd by tests/entry_point_ref.py:scaled_error under the per-head scales
of the reference's docstring.  The bound is min(FACTOR times the error the float32 torch restatement leaves on the same inputs, the
project's whole-array cap), FACTOR = entry_point_ref.KERNEL_FACTOR = 4; the whole-array criteria of tests/test_gat_heads_gpu.py are
asserted as well.  tests/test_gat_heads_ladder_cpu.py shows that a cut walk, a head read from another head's slot and a missed maximum
each miss these bounds.

MEASURED on an MI355X, worst scaled error, the class of the row it fell on (gat_heads_ladder_ref.row_class), its head and shape, with the
float32 restatement's figure on the same case beside it.  Ladder (88 cases): y 1.31e-06 (hub column, head 3 of (16, 4); restatement
5.00e-06), dH 1.31e-06 (hub column, head 1 of (4, 16); 3.97e-06), ds 5.27e-07 (hub row, head 13 of (16, 4); 1.59e-06), dt 7.21e-07 (hub row,
head 4 of (16, 4); 3.73e-06).  Planted maxima (110 cases): y 1.31e-06 (hub row, (2, 24); 4.83e-06), dH 1.06e-06 (hub column, (2, 32);
3.47e-06), ds 4.26e-07 (hub column, (16, 4); 2.25e-06), dt 9.99e-07 (hub row, (16, 4); 3.87e-06).  The largest ratio of a kernel's error to
the restatement's on the same case was 1.41 (ladder, dt of (2, 32)) and 2.37 (planted, ds of (2, 32)): no case needed more than FACTOR = 4,
and no kernel was changed.  The restatement's worst figures over the ladder cases are gat_heads_ladder_ref.F32_FIGURES.  Not measured:
attention dropout (the multi-head layers refuse it), graphs beyond 515 nodes, and heads * C above 64 (refused by the entry points)."""
import numpy as np
import pytest
import torch

from tests import gat_heads_ladder_ref as ref
from tests import gat_reverse_ref as one
from tests.entry_point_ref import F32_EPS, scaled_error
from tests.helpers import rel_err
from tests.test_gat_reverse_degrees_gpu import _guards_intact, _sliced, _t

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def graphs():
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    out = {}
    for directed in (False, True):
        m, tgt, src, _ = ref.ladder_graph(directed)
        a = DeviceCSR.from_scipy(m, with_values=False, drop_diagonal=True)
        assert np.array_equal(a.colidx.cpu().numpy(), src) and a.nnz == len(tgt)
        at = a.transposed()
        assert (at is a) == (not directed)
        out[directed] = (a, at)
    return out


def _reverse(hip, a, transposed, Hd, heads, S, Y, dY, bias, a_s, a_n, tape, concat, self_loop):
    """amar_gat_heads_bwd_f32 itself, into outputs that start as NaN; dHd is a column slice (lddh = heads * C + 8).
    Returns ({'dout', 'dS', 'dH'} as device tensors, dHd's buffer)."""
    n, HC = Hd.shape
    C, nan = HC // heads, float('nan')
    dout, scratch = torch.full(tuple(Y.shape), nan, device=DEV), torch.full((3 * heads * n,), nan, device=DEV)
    dS = torch.full((n, 2 * heads), nan, device=DEV)
    dH, dh_buf = _sliced(shape=(n, HC))
    f32, i32 = torch.float32, torch.int32
    tr = a if transposed is None else transposed
    assert a.rowptr.numel() == tr.rowptr.numel() == n + 1 and tr.colidx.numel() == a.colidx.numel() and tuple(S.shape) == (n, 2 * heads)
    assert tuple(Y.shape) == tuple(dY.shape) == (n, HC if concat else C) and bias.numel() == Y.shape[1] and S.is_contiguous()
    assert all(v.numel() == HC and v.is_contiguous() for v in (a_s, a_n)) and (concat or (tuple(tape.shape) == (n, HC) and tape.is_contiguous()))
    code = hip.load().amar_gat_heads_bwd_f32(
        hip._ptr(a.rowptr, i32, 'rowptr'), hip._ptr_entries(a.colidx, i32, 'colidx'), hip._ptr(tr.rowptr, i32, 't_rowptr'),
        hip._ptr_entries(tr.colidx, i32, 't_colidx'), hip._ptr(Hd, f32, 'Hd'), hip._ld(Hd, 'Hd'), heads, C, hip._ptr(S, f32, 'S'),
        hip._ptr(Y, f32, 'Y'), hip._ld(Y, 'Y'), hip._ptr(dY, f32, 'dY'), hip._ld(dY, 'dY'), hip._ptr(bias, f32, 'bias'), hip._ptr(a_s, f32, 'a_self'),
        hip._ptr(a_n, f32, 'a_neigh'), hip._ptr(None if concat else tape, f32, 'out_tape'), hip._ptr(dout), hip._ptr(scratch), hip._ptr(dS),
        hip._ptr(dH), hip._ld(dH, 'dH'), 1 if concat else 0, 1 if self_loop else 0, n, hip._stream())
    hip._check(code, 'amar_gat_heads_bwd_f32')
    return {'dout': dout, 'dS': dS, 'dH': dH}, dh_buf


def _worst(got, want, scale, classes, width):
    """(scaled_error, class of the row of the worst live element, its head)."""
    rel = np.abs(np.asarray(got, dtype=np.float64) - want) / np.where(scale > 0, scale, np.inf)
    row, col = np.unravel_index(rel.argmax(), rel.shape)
    return scaled_error(got, want, scale), classes[row], int(col // width)


def _run_case(hip, graphs, case, heads, C, concat, self_loop, directed, S_host=None, label=''):
    """Forward with its tape, then the reverse, on `case` (ref.case or ref.planted_case); S from rowwise_xw_heads unless given."""
    a, at = graphs[directed]
    n, hc = ref.N, heads * C
    width = hc if concat else C
    hd, a_s, a_n, bias, dy = case['inputs']
    want, bound, classes = case['want'], case['bound'], ref.row_class(directed)
    (Hd, h_buf), (Y, y_buf), (dY, dy_buf) = _sliced(shape=(n, hc)), _sliced(shape=(n, width)), _sliced(dy)
    as_d, an_d, b_d = _t(a_s), _t(a_n), _t(bias)
    if S_host is None:
        S = torch.full((n, 2 * heads), float('nan'), device=DEV)
        hip.rowwise_xw_heads(_t(hd.reshape(n, hc)), torch.eye(hc, device=DEV).view(hc, heads, C).contiguous(), Hd, as_d, an_d, S)
        assert torch.equal(Hd, _t(hd.reshape(n, hc))) and _guards_intact(Hd, h_buf)
        s_host = S.cpu().numpy()
        for k, q in enumerate(('s', 't')):                          # the scalars per element: scale sum_c |hd a|
            err = scaled_error(s_host[:, k * heads:(k + 1) * heads], want[q], want['scale_s'][k])
            assert err <= (C + 1) * F32_EPS, (q, err)               # (C terms added one after the other: gamma_C = C u / (1 - C u) of their magnitudes)
    else:
        Hd.copy_(_t(hd.reshape(n, hc)))
        S = _t(np.concatenate(S_host, axis=1))
    tape = torch.full((n, hc), float('nan'), device=DEV)
    hip.gat_heads(a.rowptr, a.colidx, Hd, heads, S, b_d, Y, concat=concat, self_loop=self_loop, out_tape=tape)
    y = Y.cpu().numpy()
    assert np.isfinite(y).all()
    err_y, where_y, head_y = _worst(y, want['y'], want['scale_y'], classes, C if concat else width)
    print(label, (heads, C), 'concat', concat, 'self_loop', self_loop, 'directed', directed, '| y %.2e' % err_y, where_y, 'head', head_y if concat else '-',
          'bound %.2e' % bound['y'], 'float32 restatement %.2e' % case['f32']['y'])
    assert err_y <= bound['y'] and rel_err(y, want['y']) < 1e-5
    assert _guards_intact(Y, y_buf) and _guards_intact(Hd, h_buf)
    out = tape.cpu().numpy().astype(np.float64).reshape(n, heads, C)  # the tape: the heads' outputs before joining and bias
    assert np.abs(np.maximum((out.reshape(n, hc) if concat else out.mean(1)) + bias, 0) - y).max() < 1e-6
    empty = np.diff(a.rowptr.cpu().numpy()) == 0
    if not self_loop:
        assert empty.sum() >= 10 and np.array_equal(y[empty], np.broadcast_to(np.maximum(bias, 0), y[empty].shape))
    again = torch.full((n, width), float('nan'), device=DEV)
    hip.gat_heads(a.rowptr, a.colidx, Hd, heads, S, b_d, again, concat=concat, self_loop=self_loop)
    assert torch.equal(again, Y.contiguous())
    # ---- reverse
    run = lambda: _reverse(hip, a, at if directed else None, Hd, heads, S, Y, dY, b_d, as_d, an_d, tape, concat, self_loop)     # noqa: E731
    got, dh_buf = run()
    assert _guards_intact(got['dH'], dh_buf) and _guards_intact(dY, dy_buf) and _guards_intact(Y, y_buf) and _guards_intact(Hd, h_buf)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    host['ds'], host['dt'] = host['dS'][:, :heads], host['dS'][:, heads:]
    assert np.array_equal(host['dout'], dy * (y > 0))
    for q in ('dH', 'ds', 'dt'):
        assert np.isfinite(host[q]).all(), q
        err, where, head = _worst(host[q], want[q], want['scale_' + q], classes, C if q == 'dH' else 1)
        print('   ', q, '%.2e' % err, where, 'head', head, 'bound %.2e' % bound[q], 'float32 restatement %.2e' % case['f32'][q])
        assert err <= bound[q], (q, err, where, head)
    assert np.abs(host['dH'] - want['dH']).max() <= 2e-4 * np.abs(want['dH']).max()
    whole = max(np.abs(want['ds']).max(), np.abs(want['dt']).max())
    assert np.abs(host['ds'] - want['ds']).max() <= 2e-4 * whole and np.abs(host['dt'] - want['dt']).max() <= 2e-4 * whole
    if not self_loop:
        assert not host['dH'][empty & (np.bincount(a.colidx.cpu().numpy(), minlength=n) == 0)].any() and not host['ds'][empty].any()
    again, _ = run()
    assert all(torch.equal(got[k], again[k]) for k in got)             # no float atomics
    if not directed:                                                  # the wrapper (its own dHd, one structure for both walks): the same bits
        dout2, dS2, dH2 = hip.gat_heads_bwd(a.rowptr, a.colidx, Hd, heads, S, Y, dY, b_d, as_d, an_d, concat=concat, self_loop=self_loop,
                                            out_tape=None if concat else tape)
        assert torch.equal(dout2, got['dout']) and torch.equal(dS2, got['dS']) and torch.equal(dH2, got['dH'].contiguous())


@pytest.mark.parametrize('heads,C', ref.SHAPES)
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('self_loop', [True, False])
@pytest.mark.parametrize('directed', [False, True])
def test_forward_and_reverse_on_the_ladder_per_head(hip, graphs, heads, C, concat, self_loop, directed):
    _run_case(hip, graphs, ref.case(heads, C, concat, self_loop, directed), heads, C, concat, self_loop, directed, label='ladder')


@pytest.mark.parametrize('heads,C', ref.SHAPES)
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('self_loop,directed,own', [(True, False, False), (False, False, False), (True, True, False), (False, True, False),
                                                    (True, True, True)])
def test_the_maximum_at_every_position(hip, graphs, heads, C, concat, self_loop, directed, own):
    """Every (ladder row, head) has one entry whose neighbour scalar for that head is +120, at ref.planted_position; own: the ladder rows'
    own neighbour scalar is +120 (the self-loop term dominates).  A pass 1 that misses the entry gives exp(~119): not finite
    (tests/test_gat_heads_ladder_cpu.py:test_a_missed_maximum_is_not_finite).  S is built on the host; the bound comes from this case's own
    float32 restatement."""
    case = ref.planted_case(heads, C, concat, self_loop, directed, own)
    _run_case(hip, graphs, case, heads, C, concat, self_loop, directed, S_host=case['given'], label='planted own' if own else 'planted')


@pytest.mark.parametrize('heads,C', [(2, 8), (2, 12)])
def test_single_node_and_graphs_without_entries(hip, heads, C):
    """n = 1 and n = 5 with an empty colidx through the three entry points with several heads (an xor shape and an indexed one), n = 0
    writes nothing: tests/test_gat_reverse_degrees_gpu.py:test_single_node_and_graphs_without_entries, with its floor of FACTOR unit
    roundoffs where the restatement comes out exact."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    rng = np.random.default_rng(heads * C)
    hc = heads * C
    floor = ref.FACTOR * F32_EPS
    a_s, a_n = ((rng.standard_normal((C, heads, 1)) * 0.7 / np.sqrt(C)).astype(np.float32) for _ in range(2))
    none = np.zeros(0, dtype=np.int64)
    for n in (1, 5):
        a = DeviceCSR(torch.zeros(n + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, (n, n))
        hd = (rng.standard_normal((n, heads, C)) * 0.7 + 0.2).astype(np.float32)
        for concat in (True, False):
            width = hc if concat else C
            bias, dy = rng.uniform(-0.1, 0.3, width).astype(np.float32), rng.standard_normal((n, width)).astype(np.float32)
            (Hd, h_buf), (dY, _) = _sliced(shape=(n, hc)), _sliced(dy)
            S = torch.full((n, 2 * heads), float('nan'), device=DEV)
            hip.rowwise_xw_heads(_t(hd.reshape(n, hc)), torch.eye(hc, device=DEV).view(hc, heads, C).contiguous(), Hd, _t(a_s), _t(a_n), S)
            assert torch.equal(Hd, _t(hd.reshape(n, hc))) and _guards_intact(Hd, h_buf)
            for self_loop in (True, False):
                T, Ssrc, _ = one.with_self_loops(none, none, n, self_loop)
                want, f32 = ref.reference(hd, a_s, a_n, bias, dy, T, Ssrc, concat)
                Y, y_buf = _sliced(shape=(n, width))
                tape = torch.full((n, hc), float('nan'), device=DEV)
                hip.gat_heads(a.rowptr, a.colidx, Hd, heads, S, _t(bias), Y, concat=concat, self_loop=self_loop, out_tape=tape)
                y = Y.cpu().numpy()
                assert scaled_error(y, want['y'], want['scale_y']) <= max(ref.FACTOR * f32['y'], floor) and _guards_intact(Y, y_buf)
                got, dh_buf = _reverse(hip, a, None, Hd, heads, S, Y, dY, _t(bias), _t(a_s), _t(a_n), tape, concat, self_loop)
                host = {k: v.cpu().numpy() for k, v in got.items()}
                host['ds'], host['dt'] = host['dS'][:, :heads], host['dS'][:, heads:]
                assert _guards_intact(got['dH'], dh_buf) and np.array_equal(host['dout'], dy * (y > 0))
                if not self_loop:
                    assert np.array_equal(y, np.broadcast_to(np.maximum(bias, 0), y.shape))
                    assert not host['dH'].any() and not host['ds'].any() and not host['dt'].any()
                    continue
                for q in ('dH', 'ds', 'dt'):                            # one term per softmax: ds = dt = 0 up to the rounding of what cancels
                    assert scaled_error(host[q], want[q], want['scale_' + q]) <= max(ref.FACTOR * f32[q], floor), (q, n, concat)
                assert np.abs(want['ds']).max() < 1e-7 and np.abs(want['dt']).max() < 1e-7
    # n = 0: no launch, nothing written
    a = DeviceCSR(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, (0, 0))
    lib, f32t, i32 = hip.load(), torch.float32, torch.int32
    buf = {k: torch.full((4, hc), float('nan'), device=DEV) for k in ('X', 'W', 'H', 'Y', 'dY', 'dout', 'dH', 'scratch', 'tape', 'S', 'dS')}
    vec = {k: torch.full((hc,), float('nan'), device=DEV) for k in ('bias', 'a_s', 'a_n')}
    p = lambda k: hip._ptr(buf[k] if k in buf else vec[k], f32t)                                             # noqa: E731
    rp, ci = hip._ptr(a.rowptr, i32), hip._ptr_entries(a.colidx, i32, 'colidx')
    assert lib.amar_rowwise_xw_heads_f32(p('X'), hc, hc, p('W'), heads, C, p('H'), hc, p('a_s'), p('a_n'), p('S'), 0, hip._stream()) == 0
    for concat in (1, 0):
        assert lib.amar_gat_heads_f32(rp, ci, p('H'), hc, heads, C, p('S'), p('bias'), p('Y'), hc, p('tape'), concat, 1, 0, hip._stream()) == 0
        assert lib.amar_gat_heads_bwd_f32(rp, ci, rp, ci, p('H'), hc, heads, C, p('S'), p('Y'), hc, p('dY'), hc, p('bias'), p('a_s'), p('a_n'), p('tape'),
                                          p('dout'), p('scratch'), p('dS'), p('dH'), hc, concat, 1, 0, hip._stream()) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in list(buf.values()) + list(vec.values()))
