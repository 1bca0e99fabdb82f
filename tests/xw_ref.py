"""float64 references, bounds and the case table of the row-wise X.W prologue (amar_rowwise_xw_f32, amar_rowwise_xw_gather_f32,
amar_rowwise_xw_heads_f32), of the GraphSAGE tail (amar_sage_tail_f32) and of the GAT layer behind gat_pack_kernel.  numpy only: the CPU
suite checks the references and the routes of the cases, tests/test_xw_forms_gpu.py runs the cases on the device.

Bounds.  Every output of the prologue kernels is  fmaf over k ascending from 0  (F roundings), then at most one multiplication by the
row scale: against the exact product the error is below (F + 1) u sum_k |x_k w_kc| to first order, u = 2^-24; the bound used is
    (F + 2) . 2^-24 . (|x| @ |w|) . |scale|
(what tests/test_towers_one_launch_gpu.py holds the two 8-wide forms to).  An attention scalar adds C products and at most C additions
on top of the F of every H it sums (the vector kernels: fmaf over c ascending; the generic kernel: a product per lane and a butterfly of
log2(cp) levels; the heads kernel: fmaf over c ascending), so it is held to
    (F + C + 2) . 2^-24 . ((|x| @ |w|) @ |a|).
Nothing here is measured on a kernel."""
import numpy as np

U = 2.0 ** -24
TRIP_BLOCKS = 8192                                                      # the grid cap of every kernel in this file


# ---- the product --------------------------------------------------------------------------------------------------------------------
def _rows(x, row_ids):
    """(the gathered rows of x as float64, the mask of zero rows)"""
    x = np.asarray(x, dtype=np.float64)
    if row_ids is None:
        return x, None
    ids = np.asarray(row_ids, dtype=np.int64)
    pad = ids < 0
    g = x[np.where(pad, 0, ids)]
    g[pad] = 0.0
    return g, pad


def product(x, w, row_ids=None, row_scale=None, copy_to=False):
    """H = diag(row_scale) . (X[row_ids] . W) in float64; a negative id gives a zero row.  copy_to=True returns (H, the copy of X) and is
    refused together with row_ids, as the entry points refuse it."""
    if copy_to and row_ids is not None:
        raise ValueError("the row-gather form computes H only")
    g, _ = _rows(x, row_ids)
    h = g @ np.asarray(w, dtype=np.float64)
    if row_scale is not None:
        h = h * np.asarray(row_scale, dtype=np.float64)[:, None]
    return (h, np.asarray(x, dtype=np.float32).copy()) if copy_to else h


def abs_product(x, w, row_ids=None, row_scale=None):
    """(|x| @ |w|) . |scale|: the absolute sum every bound is a multiple of."""
    g, _ = _rows(x, row_ids)
    s = np.abs(g) @ np.abs(np.asarray(w, dtype=np.float64))
    if row_scale is not None:
        s = s * np.abs(np.asarray(row_scale, dtype=np.float64))[:, None]
    return s


def product_bound(x, w, row_ids=None, row_scale=None):
    F = np.asarray(w).shape[0]
    return (F + 2) * U * abs_product(x, w, row_ids, row_scale)


# ---- attention scalars --------------------------------------------------------------------------------------------------------------
def scalars(x, w, a_self, a_neigh):
    """(s_self, s_neigh) = (H . a_self, H . a_neigh) of the un-scaled product, float64."""
    h = product(x, w)
    return h @ np.asarray(a_self, dtype=np.float64).ravel(), h @ np.asarray(a_neigh, dtype=np.float64).ravel()


def scalars_bound(x, w, a):
    F, C = np.asarray(w).shape
    return (F + C + 2) * U * (abs_product(x, w) @ np.abs(np.asarray(a, dtype=np.float64).ravel()))


def heads(x, w3, a_self, a_neigh):
    """Multi-head prologue in float64.  w3 [F, heads, C]; a_self, a_neigh [C, heads] (element (c, h) at c * heads + h).  Returns
    (Hd [n, heads * C], S [n, 2 * heads]): per row the heads' self scalars, then their neighbour scalars."""
    F, H, C = w3.shape
    hd = product(x, w3.reshape(F, H * C))
    h3 = hd.reshape(-1, H, C)
    a_s, a_n = (np.asarray(a, dtype=np.float64).reshape(C, H) for a in (a_self, a_neigh))
    S = np.concatenate([np.einsum('nhc,ch->nh', h3, a_s), np.einsum('nhc,ch->nh', h3, a_n)], axis=1)
    return hd, S


def heads_bound(x, w3, a_self, a_neigh):
    """The bound of `heads`' S, element by element: C terms on top of the F of every Hd."""
    F, H, C = w3.shape
    s3 = abs_product(x, w3.reshape(F, H * C)).reshape(-1, H, C)
    a_s, a_n = (np.abs(np.asarray(a, dtype=np.float64).reshape(C, H)) for a in (a_self, a_neigh))
    return (F + C + 2) * U * np.concatenate([np.einsum('nhc,ch->nh', s3, a_s), np.einsum('nhc,ch->nh', s3, a_n)], axis=1)


def within(got, want, bound):
    """Every element inside its bound (a NaN is outside)."""
    return bool((np.abs(np.asarray(got, dtype=np.float64) - want) <= bound).all())


def worst(got, want, bound):
    """The largest error as a fraction of its bound, for messages."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.nanmax(ratio)) if not np.isnan(err).any() else float('nan')


def product_f32(x, w):
    """The kernels' order of operations in numpy float32 without fused multiply-add: k ascending from 0."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    h = np.zeros((x.shape[0], w.shape[1]), dtype=np.float32)
    for k in range(w.shape[0]):
        h = (h + x[:, k:k + 1] * w[k:k + 1, :]).astype(np.float32)
    return h


# ---- GraphSAGE tail -----------------------------------------------------------------------------------------------------------------
SAGE_TAIL_TOL = 2e-6                                                    # test_sage_tail's: largest error over the largest |reference|


def sage_tail(x, agg, w, b):
    """relu(l2_normalize([x || agg] . W + b)) in float64, tf.nn.l2_normalize's max(sum z^2, 1e-12) clamp."""
    z = np.concatenate([x, agg], axis=1).astype(np.float64) @ np.asarray(w, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    return np.maximum(z / np.sqrt(np.maximum((z * z).sum(axis=1, keepdims=True), 1e-12)), 0.0)


def rel_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(1e-30, np.abs(want).max()))


# ---- GAT layer (the dense float64 softmax of tests/test_kernels_gpu.py::test_gat_xcd_sliced) ----------------------------------------
GAT_TOL = 2e-5


def gat_layer(rows, cols, h, s_self, s_neigh, bias, self_loop=True):
    n, C = h.shape
    if self_loop:
        rows, cols = np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)])
    e = s_self.astype(np.float64)[rows] + s_neigh.astype(np.float64)[cols]
    e = np.where(e > 0, e, 0.2 * e)
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, rows, e)
    ex = np.exp(e - mx[rows])
    den = np.zeros(n)
    np.add.at(den, rows, ex)
    num = np.zeros((n, C))
    np.add.at(num, rows, ex[:, None] * h.astype(np.float64)[cols])
    return np.maximum(num / (den + 1e-9)[:, None] + bias, 0.0)


def sparse_edges(n, avg_deg, seed):
    """(rows, cols) of a random directed edge list without diagonal: Poisson degrees, a tenth of the rows empty, duplicates kept."""
    rng = np.random.default_rng(seed)
    deg = rng.poisson(avg_deg, size=n)
    deg[rng.integers(0, n, size=max(1, n // 10))] = 0
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, size=len(rows))
    keep = rows != cols
    return rows[keep], cols[keep]


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def rows_per_block(kernel, C):
    cp = 1
    while cp < C:
        cp <<= 1
    return {'pieces8': 512, 'vec8': 512, 'vec16': 256, 'generic': 256 // cp}[kernel]


def trip_rows(kernel, C):
    """Rows one trip of the capped grid covers: the second trip starts one row later."""
    return TRIP_BLOCKS * rows_per_block(kernel, C)


def expected_route(kernel, C, n):
    """The dict capi.rowwise_xw_route returns for `n` rows on `kernel`."""
    cp, rpb = 256 // rows_per_block('generic', C), rows_per_block(kernel, C)
    blocks = min(-(-n // rpb), TRIP_BLOCKS)
    return dict(kernel=kernel, cp=cp, rows_per_block=rpb, blocks=blocks, trips=-(-n // (blocks * rpb)) if blocks else 0)


def boundary_rows(n, per_trip):
    """The rows on either side of every trip boundary, and the last row."""
    rows = {n - 1}
    for edge in range(per_trip, n, per_trip):
        rows.update((edge - 1, edge))
    return sorted(r for r in rows if 0 <= r < n)


def make_ids(n, table_rows, seed, edges=()):
    """int32 row ids of length n over a table of `table_rows` rows: duplicates, id 0, negative ids, a negative id at position 0 (the row
    the past-the-end clamp of the vector kernel re-reads) and negative ids on both sides of every row in `edges`."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, table_rows, size=n).astype(np.int32)
    ids[rng.random(n) < 0.07] = -1
    ids[0] = -1
    if n > 1:
        ids[n - 1] = 0
    if n > 4:
        ids[1], ids[2], ids[3] = 0, ids[4], -7
    for e in edges:
        for r in (e - 1, e):
            if 0 < r < n:
                ids[r] = -1
    return ids


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# Forms at small n.  `kernel` is the route the case must take; `env` sets AMAR_XW_FORM=rows; ldx / ldh / ld_copy are leading dimensions
# (None: width + 8, a column slice between guard columns); *_off are offsets in floats from a 16-byte boundary.
SMALL_N = (777, 1, 63, 64, 65)


def make_case(id, kernel, F, C, **kw):
    """One prologue call: the kernel it must route to, its shape and the switches listed above."""
    d = dict(id=id, kernel=kernel, F=F, C=C, env=False, copy=False, scale=False, ids=False, attn=False,
             ldx=None, ldh=None, ld_copy=None, x_off=0, h_off=0, w_off=0, copy_off=0)
    d.update(kw)
    return d


FORM_CASES = [
    make_case('pieces8-plain', 'pieces8', 8, 8),
    make_case('pieces8-copy', 'pieces8', 8, 8, copy=True),
    make_case('pieces8-scale', 'pieces8', 8, 8, scale=True),
    make_case('pieces8-copy-scale', 'pieces8', 8, 8, copy=True, scale=True),
    make_case('vec8-ids', 'vec8', 8, 8, ids=True),                          # (row ids at F = C = 8 are the vector kernel's: no pieces form)
    make_case('vec8-ids-scale', 'vec8', 8, 8, ids=True, scale=True),
    make_case('vec8-plain', 'vec8', 8, 8, env=True),
    make_case('vec8-copy', 'vec8', 8, 8, env=True, copy=True),
    make_case('vec8-scale', 'vec8', 8, 8, env=True, scale=True),
    make_case('vec8-attn', 'vec8', 8, 8, attn=True),
    make_case('vec8-attn-copy', 'vec8', 8, 8, attn=True, copy=True),
    make_case('vec16-plain', 'vec16', 16, 16),
    make_case('vec16-copy', 'vec16', 16, 16, copy=True),
    make_case('vec16-scale', 'vec16', 16, 16, scale=True),
    make_case('vec16-ids', 'vec16', 16, 16, ids=True),
    make_case('vec16-ids-scale', 'vec16', 16, 16, ids=True, scale=True),
    make_case('vec16-attn', 'vec16', 16, 16, attn=True),
    make_case('vec16-attn-copy', 'vec16', 16, 16, attn=True, copy=True),
    make_case('generic-plain', 'generic', 7, 12, ldx=9),
    make_case('generic-copy', 'generic', 7, 12, ldx=9, copy=True, ld_copy=11),
    make_case('generic-scale', 'generic', 24, 8, scale=True),
    make_case('generic-ids', 'generic', 5, 3, ids=True, ldx=5, ldh=3),
    make_case('generic-ids-scale', 'generic', 16, 32, ids=True, scale=True),
    make_case('generic-attn-C3', 'generic', 5, 3, attn=True, ldh=3),
    make_case('generic-attn-C6', 'generic', 8, 6, attn=True, copy=True),
    make_case('generic-attn-C24', 'generic', 16, 24, attn=True),
    make_case('generic-attn-C64', 'generic', 64, 64, attn=True, copy=True),
]

# Alignment fall-backs: one condition of the pieces form flipped at a time (F = C = 8, n = 777).
FALLBACK_CASES = [
    make_case('fallback-W+4B', 'vec8', 8, 8, w_off=1),
    make_case('fallback-W+4B-copy-scale', 'vec8', 8, 8, w_off=1, copy=True, scale=True),
    make_case('fallback-X+4B', 'generic', 8, 8, x_off=1),
    make_case('fallback-H+4B', 'generic', 8, 8, h_off=1),
    make_case('fallback-copy+4B', 'generic', 8, 8, copy=True, copy_off=1),
    make_case('fallback-ldx-1mod4', 'generic', 8, 8, ldx=17),
    make_case('fallback-ldx-2mod4', 'generic', 8, 8, ldx=10),
    make_case('fallback-ldx-3mod4', 'generic', 8, 8, ldx=11),
    make_case('fallback-ldh-1mod4', 'generic', 8, 8, ldh=9),
    make_case('fallback-ldh-2mod4', 'generic', 8, 8, ldh=18),
    make_case('fallback-ldh-3mod4', 'generic', 8, 8, ldh=15),
    make_case('fallback-ldcopy-1mod4', 'generic', 8, 8, copy=True, ld_copy=13),
    make_case('fallback-ldcopy-2mod4', 'generic', 8, 8, copy=True, ld_copy=14),
    make_case('fallback-ldcopy-3mod4', 'generic', 8, 8, copy=True, ld_copy=19),
    make_case('fallback-16-X+4B', 'generic', 16, 16, x_off=1),
    make_case('fallback-16-ldh-2mod4', 'generic', 16, 16, ldh=18),
    make_case('fallback-16-W+4B-stays-vec16', 'vec16', 16, 16, w_off=1),    # (the 16-wide kernel stages W through LDS by scalars)
]

# Later trips: the smallest n with trips >= 2 and a ragged last trip.  `table`: the ids index a table of that many rows.
TRIP_CASES = [
    make_case('trips-generic-C64-2', 'generic', 4, 64, n=32771, trips=2),
    make_case('trips-generic-C64-3', 'generic', 4, 64, n=65537, trips=3),
    make_case('trips-generic-attn-C24', 'generic', 4, 24, n=65541, trips=2, attn=True),
    make_case('trips-generic-ids-scale-C64', 'generic', 4, 64, n=32771, trips=2, ids=True, scale=True, table=1000),
    make_case('trips-vec16', 'vec16', 16, 16, n=2097152 + 257, trips=2, ldx=16, ldh=16),
    make_case('trips-vec8', 'vec8', 8, 8, n=4194304 + 257, trips=2, env=True, ldx=8, ldh=8),
    make_case('trips-vec8-ids', 'vec8', 8, 8, n=4194304 + 257, trips=2, ids=True, table=1000, ldx=8, ldh=8),
    make_case('trips-pieces8', 'pieces8', 8, 8, n=4194304 + 385, trips=2, ldx=8, ldh=8),
    make_case('trips-pieces8-copy-scale', 'pieces8', 8, 8, n=4194304 + 385, trips=2, copy=True, scale=True, ldx=8, ldh=8, ld_copy=8),
]

# The same operands on every kernel that can take them: equal H bits.
SAME_BITS = {8: (('pieces8', {}), ('vec8', dict(env=True)), ('generic', dict(ldh=9))),
             16: (('vec16', {}), ('generic', dict(ldh=17)))}

SAGE_TAIL_C = (4, 8, 12, 20, 36, 64)
SAGE_TAIL_F = (4, 24, 64)
SAGE_TAIL_M = 777
SAGE_TAIL_TRIP = dict(F=4, C=4, M=2097152 + 300)


def draw(case_id, n, F, C):
    """The float32 operands of one case, seeded by its id: x [n, F], w [F, C], a_self, a_neigh [C], scale [n] in [0.25, 2)."""
    rng = np.random.default_rng(abs(hash_id(case_id)) + n)
    return dict(x=rng.standard_normal((n, F)).astype(np.float32), w=rng.standard_normal((F, C)).astype(np.float32),
                a_self=rng.standard_normal(C).astype(np.float32), a_neigh=rng.standard_normal(C).astype(np.float32),
                scale=rng.uniform(0.25, 2.0, n).astype(np.float32))


def hash_id(s):
    """A seed from a case id that does not change between processes."""
    v = 0
    for ch in s.encode():
        v = (v * 131 + ch) % (1 << 31)
    return v
