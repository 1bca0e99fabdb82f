"""amar_propagate_route on the host (no GPU): which gather-address form (0: 64-bit, 1: 32-bit byte offsets, 2: 32-bit offsets into a
dense table) and which LT kernel a tiled propagation launch takes.  The launchers (amar_spmm_lt_f32, amar_gat_lt_f32, amar_spmm_xs_f32,
amar_gat_xs_f32) call the same host function, so these are their thresholds; their refusals are checked on the launchers themselves
too, with made-up addresses on arguments they refuse before they touch the device.  And GraphSageConv's choice between the one-launch
tail and the two-launch path, from tensor shapes and strides alone."""
import ctypes

import pytest
import torch

from deep_cbrs_amar_renaissance_amd import capi

BASE = 0x7F0000100000                                                  # 16-byte aligned, never dereferenced
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
SAGE, NOPAIRS = capi.SPMM_SAGE_TAIL, capi.SPMM_LT_NOPAIRS
TWO32 = 1 << 32

# width -> column bits of the packed entry word: 31 - ceil(log2(LDS rows per wave)); LT: 128 KB / (4 F 16) rows = 512 / 256 / 128 / 64,
# GAT on LT: 216 / 124 / 64 rows (amar_gat_lt_rows_per_wave); XS: the row inside its 64-row block rides above a 26-bit column
WIDTHS = {'lt': {4: 22, 8: 23, 16: 24, 32: 25}, 'gat_lt': {8: 23, 16: 24, 32: 25}, 'xs': {4: 26, 8: 26, 16: 26, 32: 26, 64: 26},
          'gat_xs': {8: 26, 16: 26, 32: 26}}
CASES = [(kind, w) for kind, ws in WIDTHS.items() for w in ws]


def route(kind, n_cols, ld, width, flags=0):
    return capi.propagate_route(kind, n_cols, ld, width, flags, code=True)


def row_floats(kind, ld, width):
    """Floats between two gathered rows: the leading dimension, except for the packed table of gat_xs (2C, whatever ldh)."""
    return 2 * width if kind == 'gat_xs' else ld


def form32(kind, ld, width):
    """The 32-bit form of a kind: 2 with a compile-time row width (LT kinds on a dense table, the packed table of gat_xs), else 1."""
    return 2 if kind == 'gat_xs' or (kind in ('lt', 'gat_lt') and ld == width) else 1


@pytest.mark.parametrize('kind,width', CASES)
def test_exactly_two_to_the_32_bytes_is_the_64_bit_form(kind, width):
    """n_cols * ld * 4 == 2^32 is the first span of the 64-bit form; one row less (2^32 - 4 ld bytes) the last of the 32-bit one."""
    for n_cols in (2048, 1 << 16, 1 << 20):
        ld = TWO32 // (4 * n_cols)                                     # a slice: ld > width
        if kind == 'gat_xs':                                           # the packed table decides: n_cols = 2^32 / (8 C), ldh is not looked at
            n_cols, ld = TWO32 // (8 * width), width + 4
        assert n_cols * row_floats(kind, ld, width) * 4 == TWO32
        r = route(kind, n_cols, ld, width)
        assert (r['code'], r['form'], r['span_bytes']) == (OK, 0, TWO32), (n_cols, r)
        r = route(kind, n_cols - 1, ld, width)
        assert (r['code'], r['form']) == (OK, form32(kind, ld, width)) and r['span_bytes'] == TWO32 - 4 * row_floats(kind, ld, width), (n_cols, r)
        if n_cols < 1 << WIDTHS[kind][width]:
            assert route(kind, n_cols + 1, ld, width)['form'] == 0
    # the last 32-bit shape of the GPU tests (2 048 columns, ld = 524 284: 2^32 - 32 768 bytes) and their 64-bit one
    if kind != 'gat_xs':
        assert route(kind, 2048, 524284, width)['form'] == 1 and route(kind, 2048, 524284, width)['span_bytes'] == TWO32 - 32768
        assert route(kind, 2048, 524288, width)['form'] == 0


@pytest.mark.parametrize('kind,width', CASES)
def test_dense_against_slice(kind, width):
    dense, sliced = route(kind, 3000, width, width), route(kind, 3000, width + 4, width)
    assert dense['code'] == OK and sliced['code'] == OK
    if kind in ('lt', 'gat_lt'):
        assert (dense['form'], sliced['form']) == (2, 1)               # a shift against a multiply
    elif kind == 'xs':
        assert (dense['form'], sliced['form']) == (1, 1)               # one 32-bit kernel form: the multiply, dense or not
    else:
        assert (dense['form'], sliced['form']) == (2, 2)               # the packed table is dense whatever H's leading dimension
    assert dense['kernel'] == 'pairs' and sliced['kernel'] == 'pairs'


@pytest.mark.parametrize('kind,width', CASES)
def test_column_bit_limit(kind, width):
    bits = WIDTHS[kind][width]
    r = route(kind, 1 << bits, width, width)
    assert r['code'] == OK and (r['col_bits'], r['max_cols']) == (bits, 1 << bits)
    r = route(kind, (1 << bits) + 1, width, width)
    assert r['code'] == EUNSUPPORTED and r['form'] == -1 and r['max_cols'] == 1 << bits


def test_dense_tables_reach_the_64_bit_form_only_at_the_widest_width():
    """Under its column bits a DENSE LT table spans at most 2^cbits * F * 4 bytes: 2^26, 2^28, 2^30 at F = 4, 8, 16 — never past 2^31 —
    and exactly 2^32 at F = 32, where the 64-bit form is reached by the one shape of 2^25 rows (DESIGN.md has the table)."""
    for kind in ('lt', 'gat_lt'):
        for width, bits in WIDTHS[kind].items():
            r = route(kind, 1 << bits, width, width)
            assert r['span_bytes'] == (1 << bits) * width * 4
            if width < 32:
                assert r['span_bytes'] <= 1 << 30 and r['form'] == 2
            else:
                assert r['span_bytes'] == TWO32 and r['form'] == 0
                assert route(kind, (1 << bits) - 1, width, width)['form'] == 2
                assert route(kind, (1 << 24) + 2048, width, width)['form'] == 2      # the dense table above 2^31 bytes of the GPU tests
                assert route(kind, (1 << 24) + 2048, width, width)['span_bytes'] > 1 << 31
    # the packed table of gat_xs: the 64-bit form at n_cols = 2^32 / (8 C) = 2^26, 2^25, 2^24, the first of them the column limit itself
    for width, n_cols in ((8, 1 << 26), (16, 1 << 25), (32, 1 << 24)):
        assert route('gat_xs', n_cols, width, width)['form'] == 0 and route('gat_xs', n_cols - 1, width, width)['form'] == 2


@pytest.mark.parametrize('width', [4, 8, 16, 32])
def test_lt_kernel_variants(width):
    small, big = (3000, width + 4), (2048, 524288)
    assert route('lt', *small, width)['kernel'] == 'pairs'
    r = route('lt', *small, width, NOPAIRS)
    assert r['code'] == OK and r['kernel'] == ('nopairs' if width >= 8 else 'pairs')       # F = 4 has no lean step
    r = route('lt', 3000, width, width, NOPAIRS)
    assert r['form'] == 2 and r['kernel'] == ('nopairs' if width >= 8 else 'pairs')
    # the 64-bit form runs the kernel with the pair logic on an image without pairs
    r = route('lt', *big, width, NOPAIRS)
    assert (r['code'], r['form'], r['kernel']) == (OK, 0, 'pairs')
    # the fused GraphSAGE tail: 32-bit forms of F >= 8; the 64-bit form is refused
    for shape in (small, (3000, width)):
        r = route('lt', *shape, width, SAGE)
        assert (r['code'], r['kernel']) == ((OK, 'sage_tail') if width >= 8 else (EUNSUPPORTED, 'unsupported'))
        assert route('lt', *shape, width, SAGE | NOPAIRS)['kernel'] == ('sage_tail' if width >= 8 else 'unsupported')
    r = route('lt', *big, width, SAGE)
    assert (r['code'], r['form'], r['kernel']) == (EUNSUPPORTED, 0, 'unsupported')
    assert route('lt', 2048, 524284, width, SAGE)['code'] == (OK if width >= 8 else EUNSUPPORTED)
    # the flags mean nothing to the other kinds
    for kind in ('gat_lt', 'xs', 'gat_xs'):
        if width in WIDTHS[kind]:
            assert route(kind, *big, width, SAGE | NOPAIRS) == route(kind, *big, width)


def test_argument_refusals_of_the_query():
    lib, info = capi.load(), capi.PropagateRouteInfo()
    assert lib.amar_propagate_route(0, 100, 8, 8, 0, None) == EINVAL
    assert lib.amar_propagate_route(4, 100, 8, 8, 0, ctypes.byref(info)) == EINVAL and lib.amar_propagate_route(-1, 100, 8, 8, 0, ctypes.byref(info)) == EINVAL
    for kind in WIDTHS:
        assert route(kind, -1, 8, 8)['code'] == EINVAL
        assert route(kind, 100, 4, 8)['code'] == EINVAL                # ld < width
        assert route(kind, 100, 10, 8)['code'] == (OK if kind == 'gat_xs' else EINVAL)     # ld % 4: the pack kernel reads H by scalars
        assert route(kind, 100, 12, 12)['code'] == EUNSUPPORTED and route(kind, 100, 128, 128)['code'] == EUNSUPPORTED
        assert route(kind, 0, 8, 8)['code'] == OK
    assert route('lt', 100, 64, 64)['code'] == EUNSUPPORTED and route('xs', 100, 64, 64)['code'] == OK
    assert route('gat_lt', 100, 4, 4)['code'] == EUNSUPPORTED and route('gat_xs', 100, 4, 4)['code'] == EUNSUPPORTED
    # order of the checks, as in the launchers: the LT kinds look at the width and the columns before the leading dimension,
    # the XS kinds at the leading dimension first
    assert route('lt', (1 << 23) + 1, 9, 8)['code'] == EUNSUPPORTED and route('gat_lt', (1 << 23) + 1, 9, 8)['code'] == EUNSUPPORTED
    assert route('xs', (1 << 26) + 1, 9, 8)['code'] == EINVAL and route('lt', 100, 13, 12)['code'] == EUNSUPPORTED
    with pytest.raises(ValueError):
        capi.propagate_route('lt', 100, 4, 8)
    with pytest.raises(capi.AmarError):
        capi.propagate_route('lt', 2048, 524288, 8, SAGE)
    assert capi.propagate_route('lt', 2048, 524288, 8) == dict(form=0, kernel='pairs', col_bits=23, max_cols=1 << 23, span_bytes=TWO32)


# ---- the launchers themselves on the same arguments: nothing of these reaches the device -------------------------------------------
def lt_code(n_cols, ld, F, flags=0, n_rows=64):
    a = BASE
    sage = bool(flags & SAGE)
    return capi.load().amar_spmm_lt_f32(a, a, a, a, a, a, a, 1, 2, 1, a, a, a, ld, n_cols, a, a, F, n_rows, F, flags, a if sage else None,
                                        None, 0, None, 0, 1.0, a if sage else None, F if sage else 0, None, 0, None)


def gat_lt_code(n_cols, ld, C, n_rows=64):
    a, lib = BASE, capi.load()
    return lib.amar_gat_lt_f32(a, a, a, a, a, a, a, 1, 2, 1, lib.amar_gat_lt_rows_per_wave(C), a, a, a, a, ld, C, a, a, a, a, a, C, 1, n_rows, n_cols, 0, None)


def xs_code(n_cols, ld, F, n_rows=64):
    a = BASE
    return capi.load().amar_spmm_xs_f32(a, a, None, None, None, 8, a, ld, n_cols, None, a, a, F, n_rows, F, 0, None, None, 0, None, 0, 1.0,
                                        None, 0, None, 0, None)


def gat_xs_code(n_cols, ld, C, n_rows=64):
    a = BASE
    return capi.load().amar_gat_xs_f32(a, a, 8, a, ld, C, a, a, a, a, a, a, C, 1, n_rows, n_cols, 0, None)


LAUNCHERS = {'lt': lt_code, 'gat_lt': gat_lt_code, 'xs': xs_code, 'gat_xs': gat_xs_code}


@pytest.mark.parametrize('kind,width', CASES)
def test_launchers_refuse_what_the_query_refuses(kind, width):
    launch, bits = LAUNCHERS[kind], WIDTHS[kind][width]
    malformed = [((1 << bits) + 1, width), ((1 << bits) + 1, width + 4), (3000, width - 4), (3000, width + 1), (3000, width + 2),
                 ((1 << bits) + 1, width + 1)]
    for n_cols, ld in malformed:
        want = route(kind, n_cols, ld, width)['code']
        if kind == 'gat_xs' and ld > width:
            assert want == (OK if n_cols <= 1 << bits else EUNSUPPORTED)
            if want == OK:
                continue                                               # a well-formed call: it would launch
        assert want in (EINVAL, EUNSUPPORTED), (n_cols, ld)
        assert launch(n_cols, ld, width) == want, (n_cols, ld)


def test_launchers_refuse_unknown_widths_and_the_64_bit_sage_tail():
    for kind, launch in LAUNCHERS.items():
        for width in (12, 20, 128) + ((64,) if kind == 'lt' else ()) + ((4,) if kind.startswith('gat') else ()):
            assert route(kind, 3000, width, width)['code'] == EUNSUPPORTED == launch(3000, width, width), (kind, width)
    for F in (8, 16, 32):
        assert route('lt', 2048, 524288, F, SAGE)['code'] == EUNSUPPORTED == lt_code(2048, 524288, F, SAGE)
        assert route('lt', 1 << 25, 32, 32, SAGE)['code'] == EUNSUPPORTED == lt_code(1 << 25, 32, 32, SAGE)
    assert route('lt', 3000, 4, 4, SAGE)['code'] == EUNSUPPORTED == lt_code(3000, 4, 4, SAGE)
    # an empty call returns before anything is decided
    assert lt_code(3000, 8, 8, n_rows=0) == OK and xs_code(3000, 8, 8, n_rows=0) == OK


# ---- GraphSageConv asks the same function ---------------------------------------------------------------------------------------------
class _Graph:
    """What GraphSageConv reads of its graph: an edge-list CSR without values whose mean image is LDS-tiled."""
    vals = None

    def __init__(self, n, image):
        self.shape, self._image = (n, n), image

    def tiled_mean_image(self, f, self_loops):
        return self._image


@pytest.mark.parametrize('n,ld,one_launch', [((1 << 25) - 1, 32, True), (1 << 25, 32, False), (2048, 524284, True), (2048, 524288, False)])
def test_graphsage_takes_two_launches_where_the_fused_tail_has_no_kernel(monkeypatch, n, ld, one_launch):
    """A dense F = 32 table of exactly 2^25 rows spans 2^32 bytes: amar_spmm_lt_f32 has no fused tail for it (64-bit addresses), so the
    layer must run the aggregate on the image and the tail kernel — built here from shapes and strides only (meta tensors)."""
    from deep_cbrs_amar_renaissance_amd.layers.graphsage_conv import GraphSageConv
    from deep_cbrs_amar_renaissance_amd.utilities.lds_tiled import LdsTiled
    monkeypatch.setenv('AMAR_SPMM_KIND', 'xs')
    image = object.__new__(LdsTiled)
    x = torch.empty_strided((n, 32), (ld, 1), dtype=torch.float32, device='meta')
    assert capi.sage_tail_on_lt_supported(x, 32) == one_launch
    calls = []
    monkeypatch.setattr(capi, 'spmm_lt', lambda img, X, Y, **kw: calls.append(('spmm_lt', sorted(kw))))
    monkeypatch.setattr(capi, 'spmm_xs', lambda img, X, Y, **kw: calls.append(('spmm_xs', img is image, X is x, tuple(Y.shape), kw)))
    monkeypatch.setattr(capi, 'sage_tail', lambda X, agg, kernel, bias, out: calls.append(('sage_tail', X is x, tuple(agg.shape), tuple(out.shape))))
    layer = GraphSageConv(32, activation='relu')
    layer.build([(n, 32), None])
    y = layer.call([x, _Graph(n, image)])
    assert tuple(y.shape) == (n, 32)
    if one_launch:
        assert calls == [('spmm_lt', ['Hnext', 'prescaled', 'sage_tail'])]
    else:
        assert calls == [('spmm_xs', True, True, (n, 32), {'prescaled': True}), ('sage_tail', True, (n, 32), (n, 32))]
