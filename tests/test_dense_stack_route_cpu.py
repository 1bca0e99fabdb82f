"""amar_dense_stack_route / amar_dense_stack_bwd_route on the host (no GPU): the row form, the workgroup count, the LDS request and the
16-byte-load flags of the one-launch Dense-stack kernels, asked with made-up device addresses — the functions look at alignment and
NULL only, the HOST arrays (W, bias, dims, ...) are real.  The launchers call the same functions, so these are the launchers'
thresholds; the refusals that return before any launch are checked on the launchers themselves too."""
import ctypes

import pytest

from deep_cbrs_amar_renaissance_amd import capi

BASE = 0x7F0000100000                                                  # 16-byte aligned; + 8: half way between two boundaries
EINVAL, EUNSUPPORTED = -1, -2
CODE = {None: 0, 'relu': 1, 'sigmoid': 2}
assert all(capi.ACT_CODES[k] == v for k, v in CODE.items())


def _addr(i, off=0):
    return BASE + 0x1000000 * i + off


def _ld(width):
    return (width + 3) // 4 * 4 + 4


class Fwd:
    """The arguments of amar_dense_stack_f32 for a stack of `dims` at made-up addresses; `edit` changes them by name."""

    def __init__(self, M, dims, acts=None, xcopy=True, **edit):
        n = len(dims) - 1
        self.n, self.M = n, M
        acts = acts if acts is not None else ['relu'] * n
        self.v = dict(X=_addr(0), ldx=_ld(dims[0]), ids=None, Xcopy=_addr(1) if xcopy else None, ldxc=_ld(dims[0]), n_layers=n,
                      W=[_addr(2 + l) for l in range(n)], bias=[_addr(8 + l) for l in range(n)], dims=list(dims),
                      acts=[CODE.get(a, a) for a in acts], Y=[_addr(14 + l) for l in range(n)], ldy=[_ld(d) for d in dims[1:]], M=M)
        self.v.update(edit)

    def args(self):
        v = self.v

        def arr(ctype, values):
            return None if values is None else (ctype * max(1, len(values)))(*values)
        self.keep = [arr(ctypes.c_void_p, v['W']), arr(ctypes.c_void_p, v['bias']), arr(ctypes.c_int32, v['dims']), arr(ctypes.c_int32, v['acts']),
                     arr(ctypes.c_void_p, v['Y']), arr(ctypes.c_int64, v['ldy'])]
        return [v['X'], v['ldx'], v['ids'], v['Xcopy'], v['ldxc'], v['n_layers']] + self.keep + [v['M']]

    def route(self, code=False):
        info = capi.DenseStackRouteInfo()
        rc = capi.load().amar_dense_stack_route(*self.args(), ctypes.byref(info))
        if code:
            return rc
        assert rc == 0, rc
        return info.as_dict(self.n)

    def launch(self):
        return capi.load().amar_dense_stack_f32(*self.args(), None)

    def desc(self):
        return capi.DenseStackDesc(*[capi._as_pointer(a) for a in self.args()])


class Bwd:
    """The arguments of amar_dense_stack_bwd_f32 likewise."""

    def __init__(self, M, dims, acts=None, ytop=True, dx0=True, **edit):
        n = len(dims) - 1
        self.n, self.M = n, M
        acts = acts if acts is not None else ['relu'] * n
        self.v = dict(dYtop=_addr(0), lddy=_ld(dims[-1]), Ytop=_addr(1) if ytop else None, ldytop=_ld(dims[-1]), n_layers=n,
                      X=[_addr(2 + l) for l in range(n)], ldx=[_ld(d) for d in dims[:-1]], W=[_addr(8 + l) for l in range(n)], dims=list(dims),
                      acts=[CODE.get(a, a) for a in acts], dX0=_addr(14) if dx0 else None, lddx0=_ld(dims[0]),
                      dW=[_addr(15 + l) for l in range(n)], db=[_addr(20 + l) for l in range(n)], workspace=_addr(25), flags=0, M=M)
        self.v.update(edit)

    def args(self):
        v = self.v

        def arr(ctype, values):
            return None if values is None else (ctype * max(1, len(values)))(*values)
        self.keep = {k: arr(t, v[k]) for k, t in (('X', ctypes.c_void_p), ('ldx', ctypes.c_int64), ('W', ctypes.c_void_p), ('dims', ctypes.c_int32),
                                                  ('acts', ctypes.c_int32), ('dW', ctypes.c_void_p), ('db', ctypes.c_void_p))}
        k = self.keep
        return [v['dYtop'], v['lddy'], v['Ytop'], v['ldytop'], v['n_layers'], k['X'], k['ldx'], k['W'], k['dims'], k['acts'], v['dX0'], v['lddx0'],
                k['dW'], k['db'], v['workspace'], v['flags'], v['M']]

    def route(self, code=False):
        info = capi.DenseStackBwdRouteInfo()
        rc = capi.load().amar_dense_stack_bwd_route(*self.args(), ctypes.byref(info))
        if code:
            return rc
        assert rc == 0, rc
        return info.as_dict(self.n)

    def launch(self):
        return capi.load().amar_dense_stack_bwd_f32(*self.args(), None)

    def desc(self):
        return capi.DenseStackBwdDesc(*[capi._as_pointer(a) for a in self.args()])


def lds_formula(dims):
    """include/amar_hip.h: (2 * 64 * (D + 2) + max_l Kp_l (Np_l + 2)) floats."""
    up = [(d + 15) // 16 * 16 for d in dims]
    return 4 * (2 * 64 * (max(up) + 2) + max(k * (n + 2) for k, n in zip(up[:-1], up[1:])))


# ---- row forms and workgroup counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,rows,groups', [(1, 16, 1), (16, 16, 1), (17, 16, 2), (4096, 16, 256), (4097, 64, 65), (8192, 64, 128), (8193, 64, 129)])
def test_forward_row_form_threshold(M, rows, groups):
    r = Fwd(M, [24, 24, 24]).route()
    assert (r['rows'], r['groups']) == (rows, groups) and r['lds_bytes'] == lds_formula([24, 24, 24])


@pytest.mark.parametrize('M,rows,groups', [(1, 16, 1), (17, 16, 2), (1024, 16, 64), (1025, 64, 17), (2048, 64, 32), (4096, 64, 64)])
def test_reverse_row_form_threshold(M, rows, groups):
    r = Bwd(M, [24, 24, 24]).route()
    assert (r['rows'], r['groups']) == (rows, groups) and r['lds_bytes'] == lds_formula([24, 24, 24])
    assert capi.load().amar_dense_stack_bwd_groups(M) == groups


def test_reverse_refuses_more_than_4096_rows():
    assert Bwd(4097, [24, 24, 24]).route(code=True) == EUNSUPPORTED and Bwd(4097, [24, 24, 24]).launch() == EUNSUPPORTED


@pytest.mark.parametrize('M', [1, 16, 17, 1024, 1025, 4096])
@pytest.mark.parametrize('dims', [[24, 24, 24], [5, 7, 3], [128, 128, 128, 128, 128], [96, 64, 64, 1], [48, 48]])
def test_reverse_workspace_follows_the_header_layout(M, dims):
    """workspace + 4 + sum_{j<l} G (K_j N_j + N_j): [G][K_l N_l] then [G][N_l]."""
    lib = capi.load()
    n = len(dims) - 1
    G = -(-M // (16 if M <= 1024 else 64))
    assert lib.amar_dense_stack_bwd_groups(M) == G == Bwd(M, dims).route()['groups']
    want = 4 + sum(G * (dims[l] * dims[l + 1] + dims[l + 1]) for l in range(n))
    assert lib.amar_dense_stack_bwd_workspace_floats(M, n, (ctypes.c_int32 * (n + 1))(*dims)) == want
    assert lib.amar_dense_stack_bwd_groups(-1) == EINVAL and lib.amar_dense_stack_bwd_workspace_floats(M, 5, (ctypes.c_int32 * 6)(*([8] * 6))) == EINVAL


def test_lds_request_of_the_widest_stack_fits():
    """Four layers of 128 columns: the largest request either kernel makes, under the 160 KB amar_allow_lds may grant."""
    dims = [128] * 5
    want = 4 * (2 * 64 * 130 + 128 * 130)
    assert lds_formula(dims) == want == 133120 < 160 * 1024
    assert Fwd(4097, dims).route()['lds_bytes'] == want and Fwd(17, dims).route()['lds_bytes'] == want
    assert Bwd(4096, dims).route()['lds_bytes'] == want and Bwd(17, dims).route()['lds_bytes'] == want
    assert Fwd(100, [1, 1]).route()['lds_bytes'] == lds_formula([1, 1]) == 4 * (2 * 64 * 18 + 16 * 18)


# ---- the 16-byte-load flags, each on each of its conditions -----------------------------------------------------------------
def test_forward_vector_flags():
    dims = [24, 48, 64, 1]
    r = Fwd(300, dims).route()
    assert r['vec_x'] and r['vec_w'] == [True, True, False]             # (a single output column is no multiple of 4)
    assert not Fwd(300, [22, 48, 64, 1]).route()['vec_x']               # width % 4
    assert not Fwd(300, dims, ldx=29).route()['vec_x']                  # leading dimension % 4
    assert not Fwd(300, dims, X=_addr(0, 8)).route()['vec_x']           # address % 16
    assert not Fwd(300, dims, X=_addr(0, 4)).route()['vec_x']
    assert not Fwd(300, dims, Xcopy=_addr(1, 8)).route()['vec_x']       # ... and Xcopy's, where it is given
    assert not Fwd(300, dims, ldxc=29).route()['vec_x']
    assert Fwd(300, dims, xcopy=False, ldxc=29).route()['vec_x']        # (not looked at otherwise)
    assert Fwd(300, dims, ids=_addr(30, 4)).route()['vec_x']            # (ids are 4-byte values)
    for l in range(2):
        w = [_addr(2 + j, 8 if j == l else 0) for j in range(3)]
        assert Fwd(300, dims, W=w).route()['vec_w'] == [j != l for j in range(2)] + [False]
    assert Fwd(300, [24, 46, 64, 1]).route()['vec_w'] == [False, True, False]
    assert Fwd(300, [24, 48, 62, 1]).route()['vec_w'] == [True, False, False]
    # the flags do not depend on the row form
    assert {k: v for k, v in Fwd(4097, dims).route().items() if k.startswith('vec')} == {k: v for k, v in r.items() if k.startswith('vec')}


def test_reverse_vector_flags():
    dims = [24, 48, 64, 4]
    r = Bwd(300, dims).route()
    assert r['vec_top'] and r['vec_x'] == [True] * 3 and r['vec_w'] == [True] * 3
    assert not Bwd(300, [24, 48, 64, 1]).route()['vec_top'] and Bwd(300, [24, 48, 64, 1]).route()['vec_w'] == [True, True, False]
    assert not Bwd(300, dims, lddy=9).route()['vec_top'] and not Bwd(300, dims, dYtop=_addr(0, 8)).route()['vec_top']
    assert not Bwd(300, dims, ldytop=9).route()['vec_top'] and not Bwd(300, dims, Ytop=_addr(1, 8)).route()['vec_top']
    assert Bwd(300, dims, ytop=False, ldytop=9).route()['vec_top']      # (Ytop is not looked at where it is not given)
    for l in range(3):
        x = [_addr(2 + j, 8 if j == l else 0) for j in range(3)]
        assert Bwd(300, dims, X=x).route()['vec_x'] == [j != l for j in range(3)]
        ld = [_ld(d) + (1 if j == l else 0) for j, d in enumerate(dims[:-1])]
        assert Bwd(300, dims, ldx=ld).route()['vec_x'] == [j != l for j in range(3)]
        w = [_addr(8 + j, 8 if j == l else 0) for j in range(3)]
        assert Bwd(300, dims, W=w).route()['vec_w'] == [j != l for j in range(3)]
    r = Bwd(300, [22, 48, 62, 4]).route()
    assert r['vec_x'] == [False, True, False] and r['vec_w'] == [True, False, True]
    # dX0 is stored by single floats: its alignment changes nothing; nor do the flags
    assert Bwd(300, dims, dX0=_addr(14, 4), lddx0=25).route() == Bwd(300, dims).route() == Bwd(300, dims, flags=capi.DENSE_BWD_DEFER).route()


# ---- refusals that return before any launch: the same code from the route function and from the launcher ---------------------
def _both(case):
    a, b = case.route(code=True), case.launch()
    assert a == b, (a, b)
    return a


@pytest.mark.parametrize('make', [Fwd, Bwd])
def test_refusals(make):
    dims = [24, 24, 24]
    assert make(100, dims).route(code=True) == 0
    assert _both(make(100, dims, n_layers=0)) == EINVAL
    assert _both(make(100, [8] * 6)) == EUNSUPPORTED                     # five layers
    for l in range(3):
        assert _both(make(100, [0 if j == l else 24 for j in range(3)])) == EINVAL
        assert _both(make(100, [129 if j == l else 24 for j in range(3)])) == EUNSUPPORTED
    assert make(100, [128, 128, 128]).route(code=True) == 0
    assert _both(make(100, dims, acts=['relu', 3])) == EINVAL and _both(make(100, dims, acts=[-1, 'relu'])) == EINVAL
    assert _both(make(-1, dims)) == EINVAL
    for name in ('W', 'dims', 'acts'):
        case = make(100, dims)
        case.v[name] = None
        assert _both(case) == EINVAL, name
    assert _both(make(100, dims, W=[_addr(2), None])) == EINVAL
    lib = capi.load()
    c = make(100, dims)
    assert (lib.amar_dense_stack_route if make is Fwd else lib.amar_dense_stack_bwd_route)(*c.args(), None) == EINVAL


def test_forward_refusals():
    dims = [24, 24, 24]
    assert _both(Fwd(100, dims, ldx=23)) == EINVAL and _both(Fwd(100, dims, ldxc=23)) == EINVAL
    assert Fwd(100, dims, xcopy=False, ldxc=0).route(code=True) == 0
    assert _both(Fwd(100, dims, ldy=[24, 23])) == EINVAL and _both(Fwd(100, dims, ldy=[23, 24])) == EINVAL
    assert _both(Fwd(100, dims, X=None)) == EINVAL
    for name in ('bias', 'Y', 'ldy'):
        assert _both(Fwd(100, dims, **{name: None})) == EINVAL, name
    assert _both(Fwd(100, dims, Y=[None, _addr(15)])) == EINVAL
    # a NULL bias[l] is a layer without a bias, not an error
    assert Fwd(100, dims, bias=[None, _addr(9)]).route(code=True) == 0 and Fwd(100, dims, bias=[None, None]).route(code=True) == 0


def test_forward_of_no_rows_is_ok_without_a_launch():
    empty = Fwd(0, [24, 24, 24])
    assert empty.launch() == 0
    assert empty.route() == dict(rows=16, groups=0, lds_bytes=lds_formula([24, 24, 24]), vec_x=True, vec_w=[True, True])
    other = Fwd(0, [16, 48])
    d0, d1 = empty.desc(), other.desc()
    assert capi.load().amar_dense_stack_pair_f32(ctypes.byref(d0), ctypes.byref(d1), None) == 0
    assert capi.load().amar_dense_stack_pair_f32(None, ctypes.byref(d1), None) == EINVAL
    bad = Fwd(0, [16, 129]).desc()
    assert capi.load().amar_dense_stack_pair_f32(ctypes.byref(d0), ctypes.byref(bad), None) == EUNSUPPORTED


def test_reverse_refusals():
    dims = [24, 24, 24]
    assert _both(Bwd(0, dims)) == EINVAL                                # an empty batch has no reverse pass
    assert _both(Bwd(100, dims, lddy=23)) == EINVAL and _both(Bwd(100, dims, ldytop=23)) == EINVAL and _both(Bwd(100, dims, lddx0=23)) == EINVAL
    assert Bwd(100, dims, ytop=False, ldytop=0, dx0=False, lddx0=0).route(code=True) == 0
    assert _both(Bwd(100, dims, ldx=[24, 23])) == EINVAL and _both(Bwd(100, dims, ldx=[23, 24])) == EINVAL
    for name in ('dYtop', 'X', 'ldx', 'dW', 'db', 'workspace'):
        assert _both(Bwd(100, dims, **{name: None})) == EINVAL, name
    for name, first in (('X', 2), ('dW', 15), ('db', 20)):
        assert _both(Bwd(100, dims, **{name: [_addr(first), None]})) == EINVAL, name


def test_reverse_pair_refuses_mixed_row_forms():
    """Two stacks of one batch share a row tile: 1 024 rows (16-row workgroups) with 1 025 (64-row) is refused before any launch."""
    lib = capi.load()
    small, large = Bwd(1024, [24, 24, 24]), Bwd(1025, [16, 48])
    assert small.route()['rows'] == 16 and large.route()['rows'] == 64
    d0, d1 = small.desc(), large.desc()
    assert lib.amar_dense_stack_bwd_pair_f32(ctypes.byref(d0), ctypes.byref(d1), None) == EUNSUPPORTED
    assert lib.amar_dense_stack_bwd_pair_f32(ctypes.byref(d1), ctypes.byref(d0), None) == EUNSUPPORTED
    assert lib.amar_dense_stack_bwd_pair_f32(ctypes.byref(d0), None, None) == EINVAL
    bad = Bwd(1024, [24, 24, 24], lddy=23).desc()
    assert lib.amar_dense_stack_bwd_pair_f32(ctypes.byref(d0), ctypes.byref(bad), None) == EINVAL
    empty = Bwd(0, [24, 24, 24]).desc()
    assert lib.amar_dense_stack_bwd_pair_f32(ctypes.byref(d0), ctypes.byref(empty), None) == EINVAL
