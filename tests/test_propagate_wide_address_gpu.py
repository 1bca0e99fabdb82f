"""The gather-address forms of the tiled propagation kernels (csrc/amar_propagate.hip) on tables whose SPAN reaches 2^32 bytes.

spmm_lt_kernel (and its GAT mode), spmm_xs_partial_kernel and gat_xs_partial_kernel pick 64-bit addresses, 32-bit byte offsets or
32-bit offsets into a dense table from n_cols * ld * 4.  The form depends on the span, not on the memory touched, so the tables
here are strided views over one buffer of 4 GiB (and 14 MiB): 2 048 rows, ld = 524 284 (2^32 - 32 768 bytes: the last 32-bit span,
the top columns' offsets above 2^31), ld = 524 288 (exactly 2^32: the first span of the 64-bit form, whose largest offset still
fits 32 bits) and ld = 526 336 (the offsets of the last seven columns need 33 bits: a 64-bit form that truncated its byte offset
would read row 0's gap).  Only the rows are written; the buffer is never cleared.
Every case asserts the form amar_propagate_route reports for its exact arguments before it launches, compares every form with the
float64 result, and asserts that all forms of a case — which differ in address arithmetic alone — give the same bits.
References: tests/propagate_wide_ref.py."""
import numpy as np
import pytest
import torch

from tests import propagate_wide_ref as ref
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ARENA_FLOATS = (ref.N - 1) * ref.LD_PAST + 64   # 4 GiB + 14 MiB: 2 048 rows at ld = 526 336 ([2^24 + 2 048, 32] at ld = 64 ends below 4 GiB + 512 KiB)
N = ref.N
FORM_OF = {'dense': 2, 'slice': 1, 'last32': 1, 'wide64': 0, 'past64': 0}
LD_OF = {'last32': ref.LD_32, 'wide64': ref.LD_64, 'past64': ref.LD_PAST}
LAYOUTS = ('dense', 'slice', 'last32', 'wide64', 'past64')


@pytest.fixture(scope='module')
def arena(hip):
    buf = torch.empty(ARENA_FLOATS, dtype=torch.float32, device=DEV)
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def graph(hip):
    """The small graph once: the gcn-filtered matrix with its factors (device), its float64 image (host), the edge-list CSR."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, gcn_filter_device
    from scipy import sparse
    g = ref.wide_graph()
    a = gcn_filter_device(torch.from_numpy(g['u']).to(DEV), torch.from_numpy(g['v']).to(DEV), N)
    rows, cols = ref.edge_list(g)
    e = DeviceCSR.from_scipy(sparse.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(N, N)), with_values=False, device=torch.device(DEV))
    deg = np.bincount(rows, minlength=N)
    assert deg[g['hub']] * 4 >= len(rows) and np.all(deg[g['isolated']] == 0) and deg[0] >= 40 and deg[N - 1] >= 40
    yield {'g': g, 'a': a, 'A': a.to_scipy().astype(np.float64), 'dinv': a.dinv.cpu().numpy().astype(np.float64), 'e': e,
           'rows': rows, 'cols': cols}
    torch.cuda.empty_cache()


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def place(arena, values, layout):
    """`values` [n, F] (dense, device) laid out as `layout`: itself; a column slice of a small wide buffer; the strided views."""
    n, F = values.shape
    if layout == 'dense':
        return values
    if layout == 'slice':
        wide = torch.zeros((n, F + 8), device=DEV)
        wide[:, 4:4 + F] = values
        return wide[:, 4:4 + F]
    view = arena.as_strided((n, F), (LD_OF[layout], 1))
    view.copy_(values)                                               # the rows only
    return view


def check_route(hip, kind, X, F, layout, flags=0, kernel=None):
    want = 1 if kind == 'xs' and layout == 'dense' else FORM_OF[layout]          # the XS product has no dense form
    r = hip.propagate_route(kind, X.shape[0], X.stride(0), F, flags)
    assert r['form'] == want, (kind, layout, r)
    if layout == 'last32':
        assert r['span_bytes'] == (1 << 32) - 32768 and ((N - 1) * ref.LD_32 + F) * 4 > 1 << 31
    if layout == 'wide64':
        assert r['span_bytes'] == 1 << 32
    if layout == 'past64':
        assert (N - 8) * ref.LD_PAST * 4 < 1 << 32 < (N - 7) * ref.LD_PAST * 4       # columns 2 041 .. 2 047: byte offsets past 32 bits
    if kernel is not None:
        assert r['kernel'] == kernel, (kind, layout, r)


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def spmm_epilogues(hip, run, img_rows, F, X, x0, b, w2, scale_next):
    """The three epilogues of one product on table X through `run` (hip.spmm_lt / hip.spmm_xs on a fixed image): plain; bias + ReLU +
    the next layer's product into a column slice of a wider buffer; the running sum / mean pair.  Returns the outputs."""
    n = img_rows
    y = nan(n, F)
    run(X, y)
    cat, hn = nan(n, 2 * F + 4), nan(n, F)
    cat[:, :4], cat[:, 4 + F:] = 0, 0
    run(X, cat[:, 4:4 + F], bias=b, relu=True, Wnext=w2, Hnext=hn, **({'scale_next': True} if scale_next else {}))
    assert bool((cat[:, :4] == 0).all()) and bool((cat[:, 4 + F:] == 0).all())
    y2, s1, mean = nan(n, F), nan(n, F), nan(n, F)
    run(X, y2, acc_in=x0, acc_out=s1)
    run(X, None, acc_in=s1, acc_out=mean, acc_div=3)
    assert torch.equal(y2, y)
    return {'plain': y, 'y1': cat[:, 4:4 + F].contiguous(), 'hn': hn, 's1': s1, 'mean': mean}


BOUNDS = {'plain': 2e-6, 'y1': 2e-6, 'hn': 3e-6, 's1': 2e-6, 'mean': 3e-6}       # as tests/test_kernels_gpu.py: 3e-6 after a second product / the mean


def compare_forms(tag, outs, want, bounds=BOUNDS, err=rel_err):
    """Every form against float64 within the bound; all forms the same bits.  Prints the largest error per output."""
    first = next(iter(outs))
    worst = {}
    for layout, got in outs.items():
        for name, bound in bounds.items():
            e = err(got[name].cpu().numpy(), want[name])
            worst[name] = max(worst.get(name, 0.0), e)
            assert e < bound, (tag, layout, name, e)
    print('WIDE {} forms={} max_err={}'.format(tag, ','.join(outs), ' '.join('{}={:.2e}'.format(k, v) for k, v in worst.items())))
    for layout, got in outs.items():
        for name in bounds:
            assert torch.equal(got[name], outs[first][name]), (tag, name, layout, 'differs from', first)


@pytest.mark.parametrize('F,pairs', [(4, True), (8, True), (8, False), (16, True), (16, False), (32, True), (32, False)])
def test_lt_spmm_address_forms(hip, arena, graph, F, pairs):
    """amar_spmm_lt_f32: dense (shift), slice (multiply), the last 32-bit span and the 64-bit form, on images with and without
    implicit pairs (the 64-bit form runs the pairs kernel on both), three epilogues each."""
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    from deep_cbrs_amar_renaissance_amd.utilities.math import _unit_entries
    a = graph['a']
    r, c, diag, off = _unit_entries(a, True)
    lt = lds_tiled.LdsTiled.build(r, c, N, N, F, diag, a.dinv, a.dinv, off, n_cu=3, pairs=pairs)
    assert lt.pairs == pairs and lt.n_tiles > 1 and lt.n_flagged > 0 and (lt.n_pairs > 0) == pairs
    rng = np.random.default_rng(F)
    x = rng.standard_normal((N, F)).astype(np.float32)
    x0 = rng.standard_normal((N, F)).astype(np.float32)
    b, w2 = rng.uniform(-0.5, 0.5, F).astype(np.float32), rng.uniform(-0.5, 0.5, (F, F)).astype(np.float32)
    table = torch.empty((N, F), device=DEV)
    hip.row_affine(_t(x), lt.row_scale, table)                       # S . x: what the value-free image gathers
    # A_hat x = S C (S x): against the float64 product of the fp32 table the kernel reads
    t64 = table.cpu().numpy().astype(np.float64)
    dinv = graph['dinv']
    want = ref.spmm_refs(graph['A'], t64 / np.where(dinv > 0, dinv, 1)[:, None], x0, b, w2, dinv)
    flags = 0 if pairs else hip.SPMM_LT_NOPAIRS
    outs = {}
    for layout in LAYOUTS:
        X = place(arena, table, layout)
        kernel = 'nopairs' if not pairs and FORM_OF[layout] != 0 else 'pairs'
        check_route(hip, 'lt', X, F, layout, flags, kernel)
        run = lambda X_, Y_, **kw: hip.spmm_lt(lt, X_, Y_, prescaled=True, **kw)
        outs[layout] = spmm_epilogues(hip, run, N, F, X, _t(x0), _t(b), _t(w2), True)
        again = nan(N, F)
        hip.spmm_lt(lt, X, again, prescaled=True)
        assert torch.equal(again, outs[layout]['plain'])
    compare_forms('lt F={} pairs={}'.format(F, int(pairs)), outs, want)


@pytest.mark.parametrize('F', [4, 8, 16, 32, 64])
@pytest.mark.parametrize('valued', [False, True])
@pytest.mark.parametrize('n_slices', [1, 5])
def test_xs_spmm_address_forms(hip, arena, graph, F, valued, n_slices, monkeypatch):
    """amar_spmm_xs_f32: valued and value-free images, one slice and five (no multiple of 8), the 32-bit form on a small slice and
    on the last 32-bit span, and the 64-bit form."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import XcdSliced
    a = graph['a']
    if valued:
        monkeypatch.setenv('AMAR_XS_VALUES', '1')
    xs = XcdSliced.from_csr(a, n_slices=n_slices)
    assert xs.n_slices == n_slices and (xs.vals is not None) == valued and (xs.row_scale is None) == valued
    rng = np.random.default_rng(100 + F)
    x = rng.standard_normal((N, F)).astype(np.float32)
    x0 = rng.standard_normal((N, F)).astype(np.float32)
    b, w2 = rng.uniform(-0.5, 0.5, F).astype(np.float32), rng.uniform(-0.5, 0.5, (F, F)).astype(np.float32)
    dinv = graph['dinv']
    if valued:
        table = _t(x)
        want = ref.spmm_refs(graph['A'], x.astype(np.float64), x0, b, w2, None)
    else:
        table = torch.empty((N, F), device=DEV)
        hip.row_affine(_t(x), xs.row_scale, table)
        want = ref.spmm_refs(graph['A'], table.cpu().numpy().astype(np.float64) / np.where(dinv > 0, dinv, 1)[:, None], x0, b, w2, dinv)
    kw0 = {} if valued else {'prescaled': True}
    outs = {}
    for layout in LAYOUTS:
        X = place(arena, table, layout)
        check_route(hip, 'xs', X, F, layout)
        run = lambda X_, Y_, **kw: hip.spmm_xs(xs, X_, Y_, **dict(kw0, **kw))
        outs[layout] = spmm_epilogues(hip, run, N, F, X, _t(x0), _t(b), _t(w2), not valued)
        again = nan(N, F)
        hip.spmm_xs(xs, X, again, **kw0)
        assert torch.equal(again, outs[layout]['plain'])
    compare_forms('xs F={} valued={} slices={}'.format(F, int(valued), n_slices), outs, want)


def _gat_inputs(seed, n_cols, C):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_cols, C)).astype(np.float32), (rng.standard_normal(n_cols) * 4).astype(np.float32),
            (rng.standard_normal(n_cols) * 4).astype(np.float32), rng.uniform(-0.3, 0.3, C).astype(np.float32))


@pytest.mark.parametrize('C', [8, 16, 32])
@pytest.mark.parametrize('self_loop', [True, False])
def test_gat_lt_address_forms(hip, arena, graph, C, self_loop):
    """amar_gat_lt_f32 on the same four layouts of H, against the dense float64 softmax."""
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    from deep_cbrs_amar_renaissance_amd.utilities.math import _unit_entries
    e = graph['e']
    rows, cols, diag, off = _unit_entries(e, False)
    rw = lds_tiled.GAT_ROWS_PER_WAVE[C]
    lt = lds_tiled.LdsTiled.build(rows, cols, N, N, C, diag, torch.ones(N, device=DEV), None, off, n_cu=3, split=64, rw=rw, split_growth=1.25)
    assert lt.n_flagged > 0 and lt.n_pairs > 0 and lt.n_tiles > 1
    h, ss, sn, b = _gat_inputs(C, N, C)
    r, c = graph['rows'], graph['cols']
    want = ref.gat_ref(r, c, N, h.astype(np.float64)[c], ss, sn[c], sn, h.astype(np.float64), b, self_loop)
    hd, outs = _t(h), {}
    for layout in LAYOUTS:
        H = place(arena, hd, layout)
        check_route(hip, 'gat_lt', H, C, layout)
        y = nan(N, C)
        hip.gat_lt(lt, e, H, _t(ss), _t(sn), _t(b), y, self_loop=self_loop)
        again = nan(N, C)
        hip.gat_lt(lt, e, H, _t(ss), _t(sn), _t(b), again, self_loop=self_loop)
        assert torch.equal(again, y)
        outs[layout] = {'gat': y}
    compare_forms('gat_lt C={} self_loop={}'.format(C, int(self_loop)), outs, {'gat': want}, {'gat': 2e-5}, ref.gat_err)


def _big_views(arena, F):
    """[2^24 + 2 048, F = 32] over the buffer: dense (2 GiB + 256 KiB: the shift form with offsets above 2^31), ld = 36 (the multiply
    form above 2^31), ld = 64 (more than 2^32 bytes: the 64-bit form)."""
    return {'dense': arena.as_strided((ref.BIG_N, F), (F, 1)), 'slice': arena.as_strided((ref.BIG_N, F), (F + 4, 1)),
            'wide64': arena.as_strided((ref.BIG_N, F), (2 * F, 1))}


@pytest.mark.parametrize('pairs', [True, False])
def test_lt_spmm_dense_table_above_two_gib(hip, arena, pairs):
    """The shift form reaches offsets above 2^31 only at F = 32: a real dense [2^24 + 2 048, 32] table, a 512-row block
    whose entries lie in the first and the last 1 024 columns; the same values at ld = 36 (multiply form) and ld = 64 (64-bit form)."""
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    F, n, off = 32, ref.BLOCK_ROWS, ref.BLOCK_OFFSET
    rows, cols, compact, base = ref.block_graph(ref.BIG_N, seed=3)
    rng = np.random.default_rng(9)
    scale, diag = rng.uniform(0.5, 1.5, n).astype(np.float32), rng.integers(1, 3, n).astype(np.float32)
    lt = lds_tiled.LdsTiled.build(_t(rows), _t(cols), n, ref.BIG_N, F, _t(diag), _t(scale), None, off, n_cu=2, pairs=pairs)
    assert lt.n_flagged + lt.n_pairs > 0 and lt.pairs == pairs and int(cols.max()) == ref.BIG_N - 1 and int(cols.min()) == 0
    vals = rng.standard_normal((2048, F)).astype(np.float32)         # the referenced rows: distinct values
    x0 = rng.standard_normal((n, F)).astype(np.float32)
    b, w2 = rng.uniform(-0.5, 0.5, F).astype(np.float32), rng.uniform(-0.5, 0.5, (F, F)).astype(np.float32)
    A = ref.block_matrix(rows, compact, n, 2048)
    own = vals.astype(np.float64)[off:off + n]
    y = scale.astype(np.float64)[:, None] * (diag.astype(np.float64)[:, None] * own + A @ vals.astype(np.float64))
    y1 = np.maximum(y + b, 0)
    s1 = x0.astype(np.float64) + y
    want = {'plain': y, 'y1': y1, 'hn': scale.astype(np.float64)[:, None] * (y1 @ w2.astype(np.float64)), 's1': s1, 'mean': (s1 + y) / 3}
    touched = _t(ref.referenced_rows(base))
    outs = {}
    for layout, X in _big_views(arena, F).items():
        r = hip.propagate_route('lt', ref.BIG_N, X.stride(0), F, 0 if pairs else hip.SPMM_LT_NOPAIRS)
        assert r['form'] == FORM_OF[layout] and r['kernel'] == ('nopairs' if not pairs and layout != 'wide64' else 'pairs')
        assert layout == 'wide64' or (1 << 31) < r['span_bytes'] < (1 << 32)
        X[touched] = _t(vals)
        run = lambda X_, Y_, **kw: hip.spmm_lt(lt, X_, Y_, prescaled=True, **kw)
        outs[layout] = spmm_epilogues(hip, run, n, F, X, _t(x0), _t(b), _t(w2), True)
    compare_forms('lt_block F=32 pairs={} dense>2GiB'.format(int(pairs)), outs, want)


@pytest.mark.parametrize('self_loop', [True, False])
def test_gat_lt_dense_table_above_two_gib(hip, arena, self_loop):
    """The matching GAT case: H dense [2^24 + 2 048, 32], at ld = 36 and at ld = 64."""
    from deep_cbrs_amar_renaissance_amd.utilities import lds_tiled
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR
    from scipy import sparse
    C, n, off = 32, ref.BLOCK_ROWS, ref.BLOCK_OFFSET
    rows, cols, compact, base = ref.block_graph(ref.BIG_N, seed=4)
    e = DeviceCSR.from_scipy(sparse.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, ref.BIG_N)), with_values=False,
                             device=torch.device(DEV))
    e.diag_offset = off
    lt = lds_tiled.LdsTiled.build(_t(rows), _t(cols), n, ref.BIG_N, C, torch.zeros(n, device=DEV), torch.ones(n, device=DEV), None, off, n_cu=2,
                                  split=64, rw=lds_tiled.GAT_ROWS_PER_WAVE[C], split_growth=1.25)
    h, ss_c, sn_c, b = _gat_inputs(11, 2048, C)                       # over the referenced rows
    gen = torch.Generator(device=DEV).manual_seed(5)
    ss = torch.randn(ref.BIG_N, device=DEV, generator=gen) * 4        # the bound is the maximum over ALL of s_neigh
    sn = torch.randn(ref.BIG_N, device=DEV, generator=gen) * 4
    touched = _t(ref.referenced_rows(base))
    ss[touched], sn[touched] = _t(ss_c), _t(sn_c)
    own = np.arange(off, off + n)
    want = ref.gat_ref(rows, compact, n, h.astype(np.float64)[compact], ss_c[own], sn_c[compact], sn_c[own], h.astype(np.float64)[own], b, self_loop)
    outs = {}
    for layout, H in _big_views(arena, C).items():
        r = hip.propagate_route('gat_lt', ref.BIG_N, H.stride(0), C)
        assert r['form'] == FORM_OF[layout] and (layout == 'wide64' or (1 << 31) < r['span_bytes'] < (1 << 32))
        H[touched] = _t(h)
        y = nan(n, C)
        hip.gat_lt(lt, e, H, ss, sn, _t(b), y, self_loop=self_loop)
        outs[layout] = {'gat': y}
    compare_forms('gat_lt_block C=32 self_loop={} dense>2GiB'.format(int(self_loop)), outs, {'gat': want}, {'gat': 2e-5}, ref.gat_err)


@pytest.mark.parametrize('C', [32, 16, 8])
def test_gat_xs_packed_table_of_four_gib(hip, arena, C):
    """amar_gat_xs_f32 gathers from its own packed [n_cols, 2C] table: the 64-bit form needs n_cols = 2^32 / (8 C) = 2^24 / 2^25 / 2^26
    nodes (the last is the column limit of the entry word).  A 512-row block with entries in the first, middle and last 1 024
    columns; H is generated on the device (in the buffer), the reference reads the referenced columns only; the same values with
    one column less take the 32-bit form and must give the same bits."""
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, XcdSliced
    from scipy import sparse
    n, off, n_cols = ref.BLOCK_ROWS, ref.BLOCK_OFFSET, (1 << 32) // (8 * C)
    outs, want = {}, None
    keep = {}
    for layout, nc in (('wide64', n_cols), ('dense', n_cols - 1)):
        rows, cols, compact, base = ref.block_graph(nc, seed=20 + C, blocks=('first', 'middle', 'last'))
        r = hip.propagate_route('gat_xs', nc, C, C)
        assert r['form'] == FORM_OF[layout] and r['span_bytes'] == nc * 8 * C
        e = DeviceCSR.from_scipy(sparse.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, nc)), with_values=False,
                                 device=torch.device(DEV))
        e.diag_offset = off
        xs = XcdSliced.from_csr(e, n_slices=5)
        touched = _t(ref.referenced_rows(base))
        H = arena[:nc * C].view(nc, C)
        if layout == 'wide64':
            gen = torch.Generator(device=DEV).manual_seed(C)
            H.normal_(generator=gen)
            ss, sn = torch.randn(nc, device=DEV, generator=gen) * 4, torch.randn(nc, device=DEV, generator=gen) * 4
            keep = {'h': H[touched].clone(), 'ss': ss[touched].clone(), 'sn': sn[touched].clone()}
            h, ss_c, sn_c = keep['h'].cpu().numpy(), keep['ss'].cpu().numpy(), keep['sn'].cpu().numpy()
            b = np.random.default_rng(C).uniform(-0.3, 0.3, C).astype(np.float32)
            own = np.arange(off, off + n)
            for self_loop in (True, False):
                want = want or {}
                want[self_loop] = ref.gat_ref(rows, compact, n, h.astype(np.float64)[compact], ss_c[own], sn_c[compact], sn_c[own],
                                              h.astype(np.float64)[own], b, self_loop)
        else:                                                        # one column less: the last range moves down by one, same values
            ss, sn = ss[:nc], sn[:nc]
            H[touched], ss[touched], sn[touched] = keep['h'], keep['ss'], keep['sn']
        outs[layout] = {}
        for self_loop in (True, False):
            y = nan(n, C)
            hip.gat_xs(xs, H, ss, sn, _t(b), y, self_loop=self_loop)
            outs[layout][self_loop] = y
        del xs                                                       # the packed table (4 GiB) goes back before the next is asked for
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    compare_forms('gat_xs C={} n_cols=2^{}'.format(C, n_cols.bit_length() - 1), outs, want, {True: 2e-5, False: 2e-5}, ref.gat_err)


@pytest.mark.parametrize('F', [8, 16, 32])
def test_sage_tail_has_no_64_bit_form_and_the_layer_takes_two_launches(hip, arena, graph, F, monkeypatch):
    """AMAR_SPMM_SAGE_TAIL on the 64-bit strided table: the C entry point refuses (AMAR_EUNSUPPORTED), GraphSageConv on the same view
    runs the aggregate + tail kernels and matches the one-launch result of the last 32-bit span."""
    from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
    from deep_cbrs_amar_renaissance_amd.utilities.lds_tiled import LdsTiled
    from tests import helpers
    monkeypatch.setenv('AMAR_SPMM_LT', '1')
    monkeypatch.setenv('AMAR_SPMM_KIND', 'xs')
    e = graph['e']
    img = e.tiled_mean_image(F, True)
    assert isinstance(img, LdsTiled)
    x = _t(np.random.default_rng(F).standard_normal((N, F)).astype(np.float32))
    layer = GraphSageConv(F, activation='relu')
    layer.build([(N, F), None])
    helpers.randomize_biases(layer, seed=2)
    calls = []
    monkeypatch.setattr(hip, 'spmm_lt', lambda *a, _f=hip.spmm_lt, **k: (calls.append('sage_tail' if k.get('sage_tail') is not None else 'aggregate'), _f(*a, **k))[1])
    monkeypatch.setattr(hip, 'sage_tail', lambda *a, _f=hip.sage_tail, **k: (calls.append('tail'), _f(*a, **k))[1])
    X = place(arena, x, 'last32')
    check_route(hip, 'lt', X, F, 'last32', hip.SPMM_SAGE_TAIL | (0 if img.pairs else hip.SPMM_LT_NOPAIRS), 'sage_tail')
    y_one = layer([X, e]).clone()
    assert calls == ['sage_tail']
    X = place(arena, x, 'wide64')
    r = hip.propagate_route('lt', N, X.stride(0), F, hip.SPMM_SAGE_TAIL, code=True)
    assert (r['code'], r['form'], r['kernel']) == (-2, 0, 'unsupported')
    with pytest.raises(hip.AmarError, match=r'code -2'):
        hip.spmm_lt(img, X, nan(N, F), prescaled=True, sage_tail=(layer.kernel, layer.bias))
    del calls[:]
    y_two = layer([X, e])
    assert calls == ['aggregate', 'tail']
    err = float((y_one - y_two).abs().max())
    print('WIDE sage F={} one-launch(last32) vs two-launch(wide64) max_abs_diff={:.2e}'.format(F, err))
    assert err < 2e-5                                               # the bound of test_sage_mean_on_lds_tiled
    y_dense = layer([x, e])
    assert torch.equal(y_dense, y_one)                               # shift form against the multiply form of the same launch
