"""Every kernel form of the row-wise X.W prologue and of the kernels next to it against float64 (tests/xw_ref.py), on every trip of
their capped grids (pytest -m gpu).

Each case first ASKS the launcher's own route function (capi.rowwise_xw_route / capi.sage_tail_route) and asserts the kernel and the
number of grid trips it claims to test, then runs the kernel twice: the two runs are equal bit for bit, every output element is inside
the bound xw_ref derives from the float32 summation (nothing is measured on the kernels), outputs start as NaN inside wider buffers
whose guard floats (before the view, between its rows, after it) keep their sentinel, and inputs sit between NaN guards.  The cases live
in xw_ref; the CPU suite checks the same routes with made-up addresses.

Kernel form                                             reached by (each asserts the route)
  rowwise_xw8_pieces_kernel<4>                          test_forms_small[pieces8-plain | -copy | -scale | -copy-scale]   n = 777, 1, 63, 64, 65
      second trip (n = 4 194 304 + 385)                 test_later_trips[trips-pieces8], [trips-pieces8-copy-scale]
  rowwise_xw_vec_kernel<8>                              test_forms_small[vec8-plain | -copy | -scale] (AMAR_XW_FORM=rows), [vec8-ids],
                                                        [vec8-ids-scale], [vec8-attn], [vec8-attn-copy]; test_alignment_fallbacks[fallback-W+4B*]
      second trip (n = 4 194 304 + 257)                 test_later_trips[trips-vec8], [trips-vec8-ids]   (the second in-trip slot of the last
                                                        trip is past the end for all but one thread; negative ids on both sides of the edge)
  rowwise_xw_vec_kernel<16>                             test_forms_small[vec16-plain | -copy | -scale | -ids | -ids-scale | -attn | -attn-copy],
                                                        test_alignment_fallbacks[fallback-16-W+4B-stays-vec16]
      second trip (n = 2 097 152 + 257)                 test_later_trips[trips-vec16]
  rowwise_xw_kernel, cp = 16, 8, 4, 32                  test_forms_small[generic-plain | -copy | -scale | -ids | -ids-scale]
      attention scalars, cp = 4, 8, 32, 64              test_forms_small[generic-attn-C3 | -C6 | -C24 | -C64]   (C = 3, 6, 24: padded butterfly lanes)
      every alignment fall-back, one at a time          test_alignment_fallbacks[fallback-X+4B | -H+4B | -copy+4B | -ldx-* | -ldh-* | -ldcopy-* | -16-*]
      second and third trip, cp = 64                    test_later_trips[trips-generic-C64-2], [trips-generic-C64-3]
      second trip with the butterfly, cp = 32           test_later_trips[trips-generic-attn-C24]
      second trip with row ids and row scale            test_later_trips[trips-generic-ids-scale-C64]
  the same H bits on pieces8 / vec8 / generic (8) and   test_same_bits_on_every_kernel[8], [16]   (attention scalars of the vector against the
      vec16 / generic (16)                              generic kernel: each inside its bound, their last bits may differ)
  amar_rowwise_xw_heads_f32 -> generic, 5 trips,        test_heads_prologue[heads4x4-F4-trips]    n = 524 291
      gat_heads_scalars_kernel second trip
  amar_rowwise_xw_heads_f32 -> vec16 / pieces8          test_heads_prologue[heads2x8-F16-vec16], [heads2x4-F8-pieces8]
  gat_pack_kernel second trip (n_cols = 32 773, C = 32) test_gat_pack_second_trip
  sage_tail_kernel<4 | 8 | 16 | 32 | 64>                test_sage_tail_forms[C-cp-F]  C = 4, 8, 12, 20, 36, 64 x F = 4, 24, 64 at M = 777
      second trip (M = 2 097 152 + 300)                 test_sage_tail_second_trip
"""
import numpy as np
import pytest
import torch

from tests import xw_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
SENTINEL = 7.0
LEAD = 8                                                                # guard floats before and after every view (32 bytes: keeps alignment)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Slab:
    """A [n, width] float32 device view with leading dimension `ld` that starts LEAD + off floats into a flat buffer filled with
    `fill`: guard floats before the view, between its rows (ld > width) and after it."""

    def __init__(self, n, width, ld=None, off=0, fill=NAN, data=None, blank=None):
        self.n, self.width, self.ld, self.fill = n, width, width if ld is None else ld, fill
        self.start = LEAD + off
        self.flat = torch.full((self.start + n * self.ld + LEAD,), fill, dtype=torch.float32, device=DEV)
        self.view = self.flat.as_strided((n, width), (self.ld, 1), self.start)
        if data is not None:
            self.view.copy_(_dev(data))
        elif blank is not None:
            self.view.fill_(blank)

    def _kept(self, t):
        return bool(torch.isnan(t).all()) if self.fill != self.fill else bool((t == self.fill).all())

    def guards_intact(self):
        end = self.start + self.n * self.ld
        ok = self._kept(self.flat[:self.start]) and self._kept(self.flat[end:])
        if self.ld > self.width:
            ok = ok and self._kept(self.flat.as_strided((self.n, self.ld - self.width), (self.ld, 1), self.start + self.width))
        return ok


def _vector(n):
    """(buffer, contiguous [n] view filled with NaN between sentinel guards)"""
    buf = torch.full((n + 2 * LEAD,), SENTINEL, dtype=torch.float32, device=DEV)
    v = buf[LEAD:LEAD + n]
    v.fill_(NAN)
    return buf, v


def _vector_guards_intact(buf, n):
    return bool((buf[:LEAD] == SENTINEL).all()) and bool((buf[LEAD + n:] == SENTINEL).all())


def _weights(w, off):
    """W [F, C] contiguous, `off` floats past a 16-byte boundary, between NaN guards."""
    flat = torch.full((LEAD + off + w.size + LEAD,), NAN, dtype=torch.float32, device=DEV)
    view = flat[LEAD + off:LEAD + off + w.size].view(w.shape)
    view.copy_(_dev(w))
    return view


class Call:
    """The device operands of one prologue call and its float64 expectations."""

    def __init__(self, case, n, x, w, a_self=None, a_neigh=None, scale=None, ids=None, xdev=None, want=None, absprod=None):
        F, C = case['F'], case['C']
        self.case, self.n, self.F, self.C = case, n, F, C
        self.X = xdev if xdev is not None else Slab(x.shape[0], F, case['ldx'] or F + 8, case['x_off'], data=x).view
        self.W = _weights(w, case['w_off'])
        self.ids = _dev(ids) if ids is not None else None
        self.scale = _dev(scale) if scale is not None else None
        self.attn = (_dev(a_self), _dev(a_neigh)) if case['attn'] else None
        # float64: the gathered, scaled product and its absolute sum (handed in where a module-wide table already has them)
        if want is None:
            want, absprod = ref.product(x, w), ref.abs_product(x, w)
        if ids is not None:
            pad = ids < 0
            want, absprod = want[np.where(pad, 0, ids)], absprod[np.where(pad, 0, ids)]
            want[pad], absprod[pad] = 0.0, 0.0
        if scale is not None:
            want, absprod = want * scale.astype(np.float64)[:, None], absprod * scale.astype(np.float64)[:, None]
        self.want, self.bound = want, (F + 2) * ref.U * absprod
        if case['attn']:
            self.s_want = ref.scalars(x, w, a_self, a_neigh)
            self.s_bound = (ref.scalars_bound(x, w, a_self), ref.scalars_bound(x, w, a_neigh))
        self.x_host = x

    def route(self, hip):
        H = Slab(self.n, self.C, self.case['ldh'] or self.C + 8, self.case['h_off'], fill=SENTINEL).view
        cp = Slab(self.n, self.F, self.case['ld_copy'] or self.F + 8, self.case['copy_off'], fill=SENTINEL).view if self.case['copy'] else None
        return hip.rowwise_xw_route(self.X, self.W, H, copy_to=cp, attn=self.attn is not None, row_ids=self.ids)

    def run(self, hip):
        c, n = self.case, self.n
        out = dict(H=Slab(n, self.C, c['ldh'] or self.C + 8, c['h_off'], fill=SENTINEL, blank=NAN))
        kw = {}
        if c['copy']:
            out['copy'] = Slab(n, self.F, c['ld_copy'] or self.F + 8, c['copy_off'], fill=SENTINEL, blank=NAN)
            kw['copy_to'] = out['copy'].view
        if self.attn is not None:
            out['ss'], out['sn'] = _vector(n), _vector(n)
            kw.update(a_self=self.attn[0], a_neigh=self.attn[1], s_self=out['ss'][1], s_neigh=out['sn'][1])
        hip.rowwise_xw(self.X, self.W, out['H'].view, row_scale=self.scale, row_ids=self.ids, **kw)
        torch.cuda.synchronize()
        return out

    def check(self, hip, kernel, trips=None, explicit_rows=()):
        cid = '{} n={}'.format(self.case['id'], self.n)
        r = self.route(hip)
        assert r == ref.expected_route(kernel, self.C, self.n), cid
        if trips is not None:
            assert r['trips'] == trips >= 2, cid
        a, b = self.run(hip), self.run(hip)
        assert torch.equal(_bits(a['H'].view), _bits(b['H'].view)), cid + ': H differs between two runs'
        assert a['H'].guards_intact() and b['H'].guards_intact(), cid + ': wrote outside H'
        got = a['H'].view.cpu().numpy()
        for row in explicit_rows:
            assert ref.within(got[row], self.want[row], self.bound[row]), '{}: row {} (a trip boundary or the last row)'.format(cid, row)
        assert ref.within(got, self.want, self.bound), '{}: H error / bound = {}'.format(cid, ref.worst(got, self.want, self.bound))
        if self.case['copy']:
            assert a['copy'].guards_intact(), cid + ': wrote outside copy_to'
            assert np.array_equal(a['copy'].view.cpu().numpy(), self.x_host[:self.n]) and torch.equal(_bits(a['copy'].view), _bits(b['copy'].view)), cid
        if self.attn is not None:
            for name, want, bound in (('ss', self.s_want[0], self.s_bound[0]), ('sn', self.s_want[1], self.s_bound[1])):
                assert torch.equal(_bits(a[name][1]), _bits(b[name][1])) and _vector_guards_intact(a[name][0], self.n), cid + ' ' + name
                s = a[name][1].cpu().numpy()
                for row in explicit_rows:
                    assert ref.within(s[row], want[row], bound[row]), '{}: {} row {}'.format(cid, name, row)
                assert ref.within(s, want, bound), '{}: {} error / bound = {}'.format(cid, name, ref.worst(s, want, bound))
        return a


def _set_form(monkeypatch, case):
    if case['env']:
        monkeypatch.setenv('AMAR_XW_FORM', 'rows')
    else:
        monkeypatch.delenv('AMAR_XW_FORM', raising=False)


def _small_call(case, n, table_rows=50):
    rows = table_rows if case['ids'] else n
    d = ref.draw(case['id'], rows, case['F'], case['C'])
    ids = ref.make_ids(n, rows, seed=n) if case['ids'] else None
    scale = ref.draw(case['id'] + '-scale', n, 1, 1)['scale'] if case['scale'] else None
    return Call(case, n, d['x'], d['w'], d['a_self'], d['a_neigh'], scale, ids)


# ---- forms at small n -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.FORM_CASES, ids=[c['id'] for c in ref.FORM_CASES])
def test_forms_small(hip, monkeypatch, case):
    _set_form(monkeypatch, case)
    for n in ref.SMALL_N:
        _small_call(case, n).check(hip, case['kernel'], explicit_rows=(0, n - 1))


@pytest.mark.parametrize('case', ref.FALLBACK_CASES, ids=[c['id'] for c in ref.FALLBACK_CASES])
def test_alignment_fallbacks(hip, monkeypatch, case):
    """One float of offset or a leading dimension that is no multiple of 4 moves the call to another kernel: same results."""
    _set_form(monkeypatch, case)
    call = _small_call(case, 777)
    for t, off in ((call.X, case['x_off']), (call.W, case['w_off'])):
        assert t.data_ptr() % 16 == 4 * off
    call.check(hip, case['kernel'], explicit_rows=(0, 776))


@pytest.mark.parametrize('F', [8, 16])
def test_same_bits_on_every_kernel(hip, monkeypatch, F):
    """'The same order of operations per output, k ascending': the same operands on every kernel that can take them give the same H bits,
    plain, scaled and with the attention scalars (those are inside their bound on each kernel; their last bits may differ)."""
    n = 777
    for variant in (dict(), dict(scale=True), dict(attn=True)):
        results = {}
        for kernel, kw in ref.SAME_BITS[F]:
            if variant.get('attn') and kernel == 'pieces8':
                continue
            case = ref.make_case('same-bits-{}'.format(F), kernel, F, F, **dict(kw, **variant))
            _set_form(monkeypatch, case)
            results[kernel] = _small_call(case, n).check(hip, kernel)['H'].view
        kernels = sorted(results)
        assert len(kernels) >= 2
        for k in kernels[1:]:
            assert torch.equal(_bits(results[kernels[0]]), _bits(results[k])), '{} and {} differ ({})'.format(kernels[0], k, variant)


# ---- later trips ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    """The long tables of the later-trip cases, drawn and multiplied in float64 once: F -> (x, w, X on the device between NaN guards,
    x . w, |x| . |w|); and the 1 000-row tables the id cases gather from."""
    made = {}

    def get(key):
        if key not in made:
            kind, F, C, rows = key
            d = ref.draw('big-{}-{}-{}'.format(kind, F, C), rows, F, C)
            ld = F if kind == 'long' else F + 8
            made[key] = dict(d, X=Slab(rows, F, ld, data=d['x']).view, want=ref.product(d['x'], d['w']), absprod=ref.abs_product(d['x'], d['w']))
        return made[key]
    yield get
    made.clear()


@pytest.mark.parametrize('case', ref.TRIP_CASES, ids=[c['id'] for c in ref.TRIP_CASES])
def test_later_trips(hip, monkeypatch, big, case):
    _set_form(monkeypatch, case)
    n, F, C = case['n'], case['F'], case['C']
    per_trip = ref.trip_rows(case['kernel'], C)
    assert n > per_trip and n % per_trip != 0
    edges = tuple(range(per_trip, n, per_trip))
    if case['ids']:
        t = big(('table', F, C, case['table']))
        ids, rows = ref.make_ids(n, case['table'], seed=n, edges=edges), case['table']
    else:
        longest = max(c['n'] for c in ref.TRIP_CASES if (c['F'], c['C']) == (F, C) and not c['ids'])
        t = big(('long', F, C, longest))
        ids, rows = None, n
    scale = ref.draw(case['id'] + '-scale', n, 1, 1)['scale'] if case['scale'] else None
    dense = case['ldx'] == F
    call = Call(case, n, t['x'][:rows], t['w'], t['a_self'], t['a_neigh'], scale, ids,
                xdev=t['X'][:rows] if dense or case['ids'] else None, want=t['want'][:rows], absprod=t['absprod'][:rows])
    call.check(hip, case['kernel'], trips=case['trips'], explicit_rows=ref.boundary_rows(n, per_trip))


# ---- the multi-head prologue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,C,F,n,kernel,trips', [(4, 4, 4, 524291, 'generic', 5), (2, 8, 16, 777, 'vec16', 1), (2, 4, 8, 777, 'pieces8', 1)],
                         ids=['heads4x4-F4-trips', 'heads2x8-F16-vec16', 'heads2x4-F8-pieces8'])
def test_heads_prologue(hip, monkeypatch, heads, C, F, n, kernel, trips):
    monkeypatch.delenv('AMAR_XW_FORM', raising=False)
    HC = heads * C
    rng = np.random.default_rng(ref.hash_id('heads-{}-{}-{}'.format(heads, C, F)))
    x, w3 = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((F, heads, C)).astype(np.float32)
    a_s, a_n = rng.standard_normal((C, heads, 1)).astype(np.float32), rng.standard_normal((C, heads, 1)).astype(np.float32)
    X, W = Slab(n, F, F + 8, data=x).view, _weights(w3, 0)
    A_s, A_n = _dev(a_s), _dev(a_n)
    pairs_per_trip = ref.TRIP_BLOCKS * 256                              # gat_heads_scalars_kernel: one thread per (row, head)
    s_trips = -(-n * heads // pairs_per_trip)

    def run():
        Hd = Slab(n, HC, HC + 8, fill=SENTINEL, blank=NAN)
        S = Slab(n, 2 * heads, fill=SENTINEL, blank=NAN)
        hip.rowwise_xw_heads(X, W, Hd.view, A_s, A_n, S.view)
        torch.cuda.synchronize()
        return Hd, S

    r = hip.rowwise_xw_route(X, W.view(F, HC), Slab(n, HC, HC + 8).view)
    assert r == ref.expected_route(kernel, HC, n) and r['trips'] == trips
    if trips > 1:
        assert s_trips == 2 and (n * heads) % pairs_per_trip != 0
    (Hd, S), (Hd2, S2) = run(), run()
    assert torch.equal(_bits(Hd.view), _bits(Hd2.view)) and torch.equal(_bits(S.view), _bits(S2.view))
    assert Hd.guards_intact() and S.guards_intact()
    hd_want, s_want = ref.heads(x, w3, a_s, a_n)
    hd_bound, s_bound = ref.product_bound(x, w3.reshape(F, HC)), ref.heads_bound(x, w3, a_s, a_n)
    hd, s = Hd.view.cpu().numpy(), S.view.cpu().numpy()
    rows = set(ref.boundary_rows(n, ref.trip_rows(kernel, HC))) | set(ref.boundary_rows(n, pairs_per_trip // heads))
    for row in sorted(rows):
        assert ref.within(hd[row], hd_want[row], hd_bound[row]) and ref.within(s[row], s_want[row], s_bound[row]), row
    assert ref.within(hd, hd_want, hd_bound), ref.worst(hd, hd_want, hd_bound)
    assert ref.within(s, s_want, s_bound), ref.worst(s, s_want, s_bound)


# ---- gat_pack_kernel --------------------------------------------------------------------------------------------------------------------
def test_gat_pack_second_trip(hip):
    """amar_gat_xs_f32 at C = 32 on 32 773 nodes: the packed table [H | s_neigh | 0 ..] has 2 097 472 floats, 320 more than one trip of
    gat_pack_kernel's capped grid.  The packed table bit for bit, the layer against the row kernel and the dense float64 softmax."""
    from scipy import sparse
    from deep_cbrs_amar_renaissance_amd.utilities.math import DeviceCSR, XcdSliced
    n, C = 32773, 32
    total, per_trip = n * 2 * C, ref.TRIP_BLOCKS * 256
    assert per_trip < total < 2 * per_trip
    assert hip.propagate_route('gat_xs', n, C + 8, C)['form'] == 2
    rows, cols = ref.sparse_edges(n, 4, seed=11)
    m = sparse.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n))
    a = DeviceCSR.from_scipy(m, with_values=False)
    xs = XcdSliced.from_csr(a)
    rng = np.random.default_rng(11)
    h = rng.standard_normal((n, C)).astype(np.float32)
    ss, sn = (rng.standard_normal(n) * 4).astype(np.float32), (rng.standard_normal(n) * 4).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, C).astype(np.float32)
    H = Slab(n, C, C + 8, data=h).view
    SS, SN, B = _dev(ss), _dev(sn), _dev(b)
    y_row = torch.empty((n, C), device=DEV)
    hip.gat_layer(a.rowptr, a.colidx, H, SS, SN, B, y_row, self_loop=True)
    ys = []
    for _ in range(2):
        Y = Slab(n, C, C + 8, fill=SENTINEL, blank=NAN)
        hip.gat_xs(xs, H, SS, SN, B, Y.view, self_loop=True)
        torch.cuda.synchronize()
        assert Y.guards_intact()
        ys.append(Y.view)
    assert torch.equal(_bits(ys[0]), _bits(ys[1]))
    packed = xs._gat_scratch[C][0].cpu().numpy()
    want_packed = np.zeros((n, 2 * C), np.float32)
    want_packed[:, :C], want_packed[:, C] = h, sn
    edge = per_trip // (2 * C)                                          # the row the second trip starts in
    for row in (edge - 1, edge, n - 1):
        assert np.array_equal(packed[row].view(np.int32), want_packed[row].view(np.int32)), row
    assert np.array_equal(packed.view(np.int32), want_packed.view(np.int32))
    want = ref.gat_layer(rows, cols, h, ss, sn, b, self_loop=True)
    got, tol = ys[0].cpu().numpy(), ref.GAT_TOL * max(1.0, np.abs(want).max())
    assert np.isfinite(got).all()
    for row in (edge - 1, edge, n - 1):
        assert np.abs(got[row] - want[row]).max() < tol, row
    assert np.abs(got - want).max() < tol and np.abs(got - y_row.cpu().numpy()).max() < tol


# ---- GraphSAGE tail ---------------------------------------------------------------------------------------------------------------------
def _sage_tail_case(hip, F, C, M, cp, trips, explicit_rows):
    rng = np.random.default_rng(F * 100 + C)
    x, g = rng.standard_normal((M, F)).astype(np.float32), rng.standard_normal((M, F)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (2 * F, C)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    zero_row = min(7, M - 1)
    x[zero_row], g[zero_row] = 0, 0
    r = hip.sage_tail_route(F, C, M)
    assert r == dict(cp=cp, blocks=min(-(-M // 256), ref.TRIP_BLOCKS), trips=trips)
    X, G, W = Slab(M, F, F + 8, data=x).view, Slab(M, F, F + 4, data=g).view, _weights(w, 0)

    def run(bias):
        Y = Slab(M, C, C + 4, fill=SENTINEL, blank=NAN)
        hip.sage_tail(X, G, W, _dev(bias), Y.view)
        torch.cuda.synchronize()
        assert Y.guards_intact(), 'wrote outside Y'
        return Y.view

    y, y2 = run(b), run(b)
    assert torch.equal(_bits(y), _bits(y2))
    got, want = y.cpu().numpy(), ref.sage_tail(x, g, w, b)
    scale = max(1e-30, np.abs(want).max())
    for row in explicit_rows + (zero_row,):
        assert np.abs(got[row] - want[row]).max() / scale < ref.SAGE_TAIL_TOL, row
    assert ref.rel_err(got, want) < ref.SAGE_TAIL_TOL
    # without a bias the zero row's pre-activation is exactly zero: max(sum z^2, 1e-12) keeps it 0, not 0 / 0
    b0 = np.zeros(C, np.float32)
    got0 = run(b0).cpu().numpy()
    assert np.all(got0[zero_row] == 0.0)
    assert ref.rel_err(got0, ref.sage_tail(x, g, w, b0)) < ref.SAGE_TAIL_TOL


@pytest.mark.parametrize('F', ref.SAGE_TAIL_F)
@pytest.mark.parametrize('C,cp', list(zip(ref.SAGE_TAIL_C, (4, 8, 16, 32, 64, 64))))
def test_sage_tail_forms(hip, C, cp, F):
    _sage_tail_case(hip, F, C, ref.SAGE_TAIL_M, cp, 1, (0, ref.SAGE_TAIL_M - 1))


def test_sage_tail_second_trip(hip):
    F, C, M = ref.SAGE_TAIL_TRIP['F'], ref.SAGE_TAIL_TRIP['C'], ref.SAGE_TAIL_TRIP['M']
    per_trip = ref.TRIP_BLOCKS * 256
    assert M > per_trip and M % per_trip != 0
    _sage_tail_case(hip, F, C, M, 4, 2, tuple(ref.boundary_rows(M, per_trip)))
