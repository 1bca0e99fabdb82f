"""Reference of the one-head GAT reverse tests (tests/test_gat_reverse_ref_cpu.py, tests/test_gat_reverse_degrees_gpu.py).
TEST INFRASTRUCTURE ONLY: numpy and torch on the CPU, no device.

`degree_graph` is an edge multiset whose row (and, directed, column) lengths sit one below, on and one above every stride of the kernels'
walks; `gat_reverse64` is float64 autograd of the restated forward (tests/test_dropout_gpu.py:_gat64) with per-element error scales,
`gat_reverse32` the same formulas in float32, whose error against float64 is what the kernels' bound is a multiple of.

Error scales (notation of the comment above GatBwdArgs in csrc/amar_train.hip; l_ij = LeakyReLU'(s_i + t_j), m_ij = keep_ij * scale), each
the sum of the magnitudes of the terms the element is made of, as in tests/entry_point_ref.py:
    scale_y [i, c] = sum_j |alpha_ij m_ij h_jc| + |b_c|
    e_ij           = alpha_ij l_ij (m_ij sum_c |g_ic h_jc| + sum_c |g_ic| scale_y[i, c])
    scale_ds[i]    = sum_j e_ij            scale_dt[j] = sum_i e_ij
    scale_dH[j, c] = sum_i |alpha_ij m_ij g_ic| + scale_ds[j] |a_s[c]| + scale_dt[j] |a_n[c]|
e_ij stands where sum |d pre_ij| first suggests itself, because d pre_ij = alpha_ij (d alpha_ij - c_i) l_ij is a difference, not a term:
in a row over one source (a single entry, parallel entries of one pair, only the added self loop) d alpha_ij = c_i and d pre_ij is
1e-9 d alpha_ij (the denominator's epsilon) exactly, and wherever a row's logits share a sign sum_j d pre_ij = c_i (1 - sum_j alpha_ij)
vanishes the same way.  Any float32 evaluation leaves the rounding of the cancelled numbers there: measured against sum |d pre_ij| and
|ds_j a_s[c]| the float32 restatement below misses float64 by factors up to 1e4 on this graph (rows 0 and 20, nodes nothing points at),
so no multiple of its error could serve as a bound.  e_ij is the sum of |terms| of d alpha_ij = m_ij g_i . h_j and of
c_i = g_i . (out_i - b); it is never below |d pre_ij| (asserted).  That these larger scales still tell a walk that skips a trip from
rounding is what tests/test_gat_reverse_ref_cpu.py:test_truncated_walks_miss_the_bound_by_a_hundred_times shows.
"""
import functools

import numpy as np
import torch
from scipy import sparse

from tests.entry_point_ref import KERNEL_FACTOR, scaled_error

N = 203                                                                # 50 full workgroups of 4 rows and one of 3
LADDER = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
NS_OF_WIDTH = {4: 64, 8: 32, 16: 16, 24: 8, 32: 8, 48: 4, 64: 4}       # entries per trip of the edge walk: 64 / LPN
WIDTHS = (4, 8, 16, 24, 32, 48, 64)
HUB_ENTRIES, HUB_PARALLEL = 300, 260
# node roles (ids)
LADDER_ROWS = tuple(range(0, 19))
HUB, HUB_COL = 19, 20
LADDER_COLS = tuple(range(21, 40))                                     # directed only; ordinary nodes otherwise
ONLY_SOURCES, ONLY_TARGETS = tuple(range(40, 45)), tuple(range(45, 50))    # directed only
ISOLATED = tuple(range(50, 62))
FIRST_ORDINARY = 62

FACTOR = KERNEL_FACTOR                                                 # a kernel may miss float64 by FACTOR times what gat_reverse32 misses it by
CAP_GRADIENT, CAP_FORWARD = 2e-4, 1e-5                                 # the project's whole-array criteria (test_training_gpu.py:test_gat_bwd_kernel)
GRAPH_SEED = 7
# seeds of draw_inputs per (C, directed).  tests/test_gat_reverse_ref_cpu.py holds each to its two conditions: every ladder row and the
# 300-entry row keep at least half of their outputs positive under both self_loop settings and both rates, and every truncation of
# test_truncated_walks_miss_the_bound_by_a_hundred_times moves the float64 reference by at least 100 bounds.
INPUT_SEEDS = {(4, False): 31, (8, False): 0, (16, False): 18, (24, False): 4, (32, False): 41, (48, False): 3, (64, False): 4,
               (4, True): 31, (8, True): 0, (16, True): 0, (24, True): 0, (32, True): 11, (48, True): 3, (64, True): 0}
DROP_SEED, DROP_SITE, DROP_STEP, DROP_RATE = 1234567, 8, 11, 0.35
# worst scaled error of gat_reverse32 against gat_reverse64 over every case of the GPU test (7 widths x self_loop x directed x rate), as
# measured when the tests were written; test_gat_reverse_ref_cpu.py keeps the record within 5 % of a fresh measurement
F32_FIGURES = {'y': 6.095e-6, 'dH': 4.849e-6, 'ds': 5.028e-7, 'dt': 2.743e-7}


@functools.lru_cache(maxsize=None)
def degree_graph(directed, seed=GRAPH_SEED):
    """(scipy coo matrix with parallel entries kept, tgt, src): `tgt` (row) and `src` (column) of every entry in CSR order (rows, then
    columns, parallel entries adjacent).  203 nodes, no diagonal.  Rows 0..18 hold exactly LADDER[k] entries; row 19 holds 300, of which
    260 are parallel entries of (19, 20); nodes 50..61 have no entry in either direction; ordinary rows are Poisson with duplicates.
    directed: columns 21..39 hold exactly LADDER[k] entries, nodes 40..44 occur only as sources (columns), 45..49 only as targets (rows).
    Not directed: the multiset plus its transpose; the counts above are those of the symmetrised rows (nothing points at the ladder
    nodes or the hub, so their rows are their own entries mirrored), ordinary rows draw Poisson(4) each way."""
    rng = np.random.default_rng(seed)
    special = set(LADDER_ROWS) | {HUB, HUB_COL} | set(ISOLATED)
    if directed:
        special |= set(LADDER_COLS) | set(ONLY_SOURCES) | set(ONLY_TARGETS)
    ordinary = np.array([v for v in range(N) if v not in special])
    as_columns = np.concatenate([ordinary, ONLY_SOURCES]) if directed else ordinary
    as_rows = np.concatenate([ordinary, ONLY_TARGETS]) if directed else ordinary
    r, c = [], []
    for node, count in zip(LADDER_ROWS, LADDER):
        r.append(np.full(count, node)), c.append(rng.choice(as_columns, count, replace=False))
    r.append(np.full(HUB_ENTRIES, HUB))
    c.append(np.concatenate([np.full(HUB_PARALLEL, HUB_COL), rng.choice(ordinary, HUB_ENTRIES - HUB_PARALLEL, replace=False)]))
    if directed:
        for node, count in zip(LADDER_COLS, LADDER):
            r.append(rng.choice(as_rows, count, replace=False)), c.append(np.full(count, node))
        for node in ONLY_SOURCES:
            r.append(rng.choice(ordinary, 3, replace=False)), c.append(np.full(3, node))
        for node in ONLY_TARGETS:
            r.append(np.full(3, node)), c.append(rng.choice(ordinary, 3, replace=False))
    deg = rng.poisson(8 if directed else 4, len(ordinary))
    rows = np.repeat(ordinary, deg)
    cols = rng.choice(ordinary, len(rows))
    cols = np.where(cols == rows, ordinary[(np.searchsorted(ordinary, rows) + 1) % len(ordinary)], cols)        # no diagonal
    dup = rng.random(len(rows)) < 0.1                                  # a tenth of the ordinary entries twice
    r += [rows, rows[dup]]
    c += [cols, cols[dup]]
    r, c = np.concatenate(r).astype(np.int64), np.concatenate(c).astype(np.int64)
    if not directed:
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
    order = np.lexsort((c, r))
    tgt, src = r[order], c[order]
    m = sparse.coo_matrix((np.ones(len(tgt), dtype=np.float32), (tgt, src)), shape=(N, N))
    # ---- what the tests rely on
    rows_n, cols_n = np.bincount(tgt, minlength=N), np.bincount(src, minlength=N)
    counts = sparse.csr_matrix(m)                                      # (sums parallel entries: a count per pair)
    assert (tgt != src).all()
    assert tuple(rows_n[list(LADDER_ROWS)]) == LADDER and rows_n[HUB] == HUB_ENTRIES
    assert counts[HUB, HUB_COL] == HUB_PARALLEL > 255 and counts[HUB].nnz == 1 + HUB_ENTRIES - HUB_PARALLEL
    assert len(ISOLATED) >= 10 and not rows_n[list(ISOLATED)].any() and not cols_n[list(ISOLATED)].any()
    pair = tgt[ordinary.min() <= tgt] * N + src[ordinary.min() <= tgt]
    assert len(np.unique(pair)) < len(pair), "ordinary rows must hold duplicated entries"
    assert N % 4 == 3 and rows_n[N - 1] > 0                            # the last workgroup is short and has work
    if directed:
        assert tuple(cols_n[list(LADDER_COLS)]) == LADDER
        assert (rows_n[list(ONLY_SOURCES)] == 0).all() and (cols_n[list(ONLY_SOURCES)] > 0).all() and len(ONLY_SOURCES) >= 5
        assert (cols_n[list(ONLY_TARGETS)] == 0).all() and (rows_n[list(ONLY_TARGETS)] > 0).all() and len(ONLY_TARGETS) >= 5
        assert (counts != counts.T).nnz > 0
    else:
        assert (counts != counts.T).nnz == 0 and counts[HUB_COL, HUB] == HUB_PARALLEL
    tgt.setflags(write=False), src.setflags(write=False)
    return m, tgt, src


def row_class(directed):
    """Per node: 'ladder' (a ladder row or, directed, a ladder column), 'hub row' (the 300-entry row), 'hub column' (node 20, which its
    260 parallel entries point at) or 'ordinary'."""
    names = np.array(['ordinary'] * N, dtype=object)
    names[list(LADDER_ROWS)] = 'ladder'
    if directed:
        names[list(LADDER_COLS)] = 'ladder'
    names[HUB], names[HUB_COL] = 'hub row', 'hub column'
    return names


def with_self_loops(tgt, src, n, self_loop, keep=None, loops=None):
    """The edge list the layer sums over: the stored entries, then one self loop per node (keep / loops: their dropout bits)."""
    if not self_loop:
        return tgt, src, keep
    tgt, src = np.concatenate([tgt, np.arange(n)]), np.concatenate([src, np.arange(n)])
    return tgt, src, None if keep is None else np.concatenate([keep, loops])


def draw_inputs(C, directed, seed=None):
    """(h [N, C], a_s, a_n, bias [C], dy [N, C]) float32.  The attention vectors are drawn at 0.7 / sqrt(C), so that the logits spread
    by about one at every width (both LeakyReLU branches, softmax weights within a row a few e-folds apart); H and the bias lean
    positive (mean 0.2 and 0.1), which keeps most outputs of a long row, a weighted mean of many H rows, above the ReLU's kink."""
    rng = np.random.default_rng(INPUT_SEEDS[(C, bool(directed))] if seed is None else seed)
    h = (rng.standard_normal((N, C)) * 0.7 + 0.2).astype(np.float32)
    a_s, a_n = ((rng.standard_normal(C) * 0.7 / np.sqrt(C)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-0.1, 0.3, C).astype(np.float32)
    dy = rng.standard_normal((N, C)).astype(np.float32)
    # the logits of a ladder row, of the 300-entry row and (directed) of a ladder column straddle zero: H of such a node moves along a_s
    # (a_n) until its s_i (t_j) is minus the midpoint of the two middle distinct values of its sources' t (its targets' s), so that no
    # logit sits on LeakyReLU's kink, where float32 and float64 would take different branches.  With one sign only, LeakyReLU' is one
    # constant in the row and ds_i = sum_j d pre_ij = l c_i (1 - sum_j alpha_ij) is zero whichever entries the row holds.
    _, tgt, src = degree_graph(bool(directed))
    h64, as64, an64 = h.astype(np.float64), a_s.astype(np.float64), a_n.astype(np.float64)
    s, t = h64 @ as64, h64 @ an64

    def middle(values):
        v = np.unique(values)
        return None if len(v) == 1 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])       # (one value: nothing to straddle)
    for node in LADDER_ROWS + (HUB,):
        mid = middle(t[src[tgt == node]])
        if mid is not None:
            h64[node] += as64 * ((-mid - s[node]) / (as64 @ as64))
    for node in LADDER_COLS if directed else ():
        mid = middle(s[tgt[src == node]])
        if mid is not None:
            h64[node] += an64 * ((-mid - t[node]) / (an64 @ an64))
    return h64.astype(np.float32), a_s, a_n, bias, dy


def edge_masks(tgt, src, n, self_loop, rate, seed=DROP_SEED, step=DROP_STEP, site=DROP_SITE):
    """(keep_scale per entry of with_self_loops' list, or None for rate None): the bits of data.datasets.dropout_edge_mask."""
    if rate is None:
        return None
    from deep_cbrs_amar_renaissance_amd.data.datasets import dropout_edge_mask, dropout_scale
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    keep, loops = dropout_edge_mask(seed, step, site, rowptr, src, self_loop, rate)
    _, _, keep = with_self_loops(tgt, src, n, self_loop, keep, loops)
    return keep.astype(np.float64) * float(dropout_scale(rate))


def _forward(h, a_s, a_n, bias, T, S, n, keep_scale):
    """test_dropout_gpu.py:_gat64 in the dtype of `h`, keeping the intermediates."""
    dt = h.dtype
    s, t = h @ a_s, h @ a_n
    s.retain_grad(), t.retain_grad()
    pre = s[T] + t[S]
    e = torch.where(pre > 0, pre, torch.tensor(0.2, dtype=dt) * pre)
    mx = torch.full((n,), -1e30, dtype=dt).scatter_reduce(0, T, e.detach(), 'amax')
    ex = torch.exp(e - mx[T])
    alpha = ex / (torch.zeros(n, dtype=dt).index_add(0, T, ex) + torch.tensor(1e-9, dtype=dt))[T]
    w = alpha if keep_scale is None else alpha * keep_scale
    out = torch.zeros_like(h).index_add(0, T, w[:, None] * h[S])
    return torch.relu(out + bias), s, t, pre, alpha, w


def _reverse(dtype, h, a_s, a_n, bias, dy, tgt, src, n, keep_scale):
    T, S = torch.as_tensor(np.array(tgt), dtype=torch.long), torch.as_tensor(np.array(src), dtype=torch.long)
    ten = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype)                              # noqa: E731
    ht = ten(h).requires_grad_(True)
    ks = None if keep_scale is None else ten(keep_scale)
    y, s, t, pre, alpha, w = _forward(ht, ten(a_s), ten(a_n), ten(bias), T, S, n, ks)
    (y * ten(dy)).sum().backward()
    return y.detach(), ht.grad, s.grad, t.grad, (pre.detach(), alpha.detach(), w.detach())


def gat_reverse64(h, a_s, a_n, bias, dy, tgt, src, n, keep_scale=None):
    """Float64 autograd of the restated forward over the entries (tgt, src) (self loops included by the caller: with_self_loops).
    Returns a dict of float64 arrays: y, dH, ds, dt and scale_y, scale_dH, scale_ds, scale_dt (module docstring)."""
    y, dh, ds, dt, (pre, alpha, w) = (_np(v) for v in _reverse(torch.float64, h, a_s, a_n, bias, dy, tgt, src, n, keep_scale))
    tgt, src = np.asarray(tgt), np.asarray(src)
    h64, b64, as64, an64 = (np.asarray(v, dtype=np.float64) for v in (h, bias, a_s, a_n))
    g = np.asarray(dy, dtype=np.float64) * (y > 0)
    m = np.ones(len(tgt)) if keep_scale is None else np.asarray(keep_scale, dtype=np.float64)
    add_t = lambda v: _segment(v, tgt, n)                                                                    # noqa: E731
    add_s = lambda v: _segment(v, src, n)                                                                    # noqa: E731
    out = add_t(w[:, None] * h64[src])
    scale_y = add_t(np.abs(w[:, None] * h64[src])) + np.abs(b64)
    dalpha = m * np.einsum('ec,ec->e', g[tgt], h64[src])
    c = add_t(alpha * dalpha)
    leak = np.where(pre > 0, 1.0, 0.2)
    dpre = alpha * (dalpha - c[tgt]) * leak
    # per entry: the magnitudes of the terms of d alpha_ij and of c_i, through alpha_ij l_ij (module docstring)
    e = alpha * leak * (m * np.einsum('ec,ec->e', np.abs(g[tgt]), np.abs(h64[src])) + np.einsum('ic,ic->i', np.abs(g), scale_y)[tgt])
    res = {'y': y, 'dH': dh, 'ds': ds, 'dt': dt, 'scale_y': scale_y, 'scale_ds': add_t(e), 'scale_dt': add_s(e)}
    res['scale_dH'] = add_s(np.abs(w[:, None] * g[tgt])) + np.outer(res['scale_ds'], np.abs(as64)) + np.outer(res['scale_dt'], np.abs(an64))
    assert (res['scale_ds'] >= add_t(np.abs(dpre))).all() and (res['scale_dt'] >= add_s(np.abs(dpre))).all()
    # the formulas the scales are built from are the gradient's own: they reproduce autograd
    res['formula'] = {'out': out, 'ds': add_t(dpre), 'dt': add_s(dpre),
                      'dH': add_s(w[:, None] * g[tgt]) + np.outer(add_t(dpre), as64) + np.outer(add_s(dpre), an64)}
    return res


def gat_reverse32(h, a_s, a_n, bias, dy, tgt, src, n, keep_scale=None):
    """The same formulas evaluated by torch in float32 on the CPU: {'y', 'dH', 'ds', 'dt'} as float32 arrays."""
    y, dh, ds, dt, _ = _reverse(torch.float32, h, a_s, a_n, bias, dy, tgt, src, n, keep_scale)
    out = {'y': y.numpy(), 'dH': dh.numpy(), 'ds': ds.numpy(), 'dt': dt.numpy()}
    assert all(v.dtype == np.float32 for v in out.values()), "the float32 evaluation was promoted"
    return out


def _np(v):
    return v.numpy() if isinstance(v, torch.Tensor) else tuple(x.numpy() for x in v)


def _segment(v, index, n):
    out = np.zeros((n,) + v.shape[1:])
    np.add.at(out, index, v)
    return out


QUANTITIES = ('y', 'dH', 'ds', 'dt')


def errors(got, want):
    """{quantity: scaled error of got[quantity] against the float64 result `want`}."""
    return {q: scaled_error(got[q], want[q], want['scale_' + q]) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def case(C, self_loop, directed, rate):
    """One case of the GPU test, computed once: inputs, entry list, float64 reference and the float32 restatement's errors.  Shared and
    left unchanged by the tests that use it."""
    _, tgt, src = degree_graph(directed)
    h, a_s, a_n, bias, dy = draw_inputs(C, directed)
    T, S, _ = with_self_loops(tgt, src, N, self_loop)
    ks = edge_masks(tgt, src, N, self_loop, rate)
    want = gat_reverse64(h, a_s, a_n, bias, dy, T, S, N, ks)
    f32 = errors(gat_reverse32(h, a_s, a_n, bias, dy, T, S, N, ks), want)
    return {'inputs': (h, a_s, a_n, bias, dy), 'edges': (T, S, ks), 'want': want, 'f32': f32, 'bound': {q: FACTOR * f32[q] for q in QUANTITIES}}


def truncations(length):
    """The entry counts k a row of `length` entries is cut to: the largest multiple of NS below its length for each of the five NS, and 64."""
    ks = {((length - 1) // ns) * ns for ns in (64, 32, 16, 8, 4)}
    if length > 64:
        ks.add(64)
    return sorted(ks)


def truncated(tgt, src, node, k, by_column=False):
    """Mask over the stored entries (CSR order) that drops those of row `node` past its first k; by_column: those of column `node` past
    the first k in the order of the stable transpose (by row, parallel entries in place: CSR order restricted to the column)."""
    own = np.flatnonzero((src if by_column else tgt) == node)
    keep = np.ones(len(tgt), dtype=bool)
    keep[own[k:]] = False
    return keep
