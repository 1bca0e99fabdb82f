"""Plain numpy float64 restatements of the separate training kernels of csrc/amar_train.hip (amar_wgrad_f32, amar_scatter_add_rows_f32,
amar_act_bwd_f32, amar_row_affine_f32, amar_l2norm_fwd_f32 / amar_l2norm_bwd_f32) with the element-wise error bounds the tests hold
the kernels to.  The bounds are derived, not measured: a float32 sum of n terms t_i, added in ANY order, each term a product rounded
once (or fused into the addition), differs from the exact sum by at most gamma(n + 1) * sum |t_i| with gamma(n) = n u / (1 - n u),
u = 2**-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2, eq. 3.5 for the product); one more rounding
is left for a final addition or store."""
import numpy as np

U = 2.0 ** -24                                                         # unit roundoff of float32


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def wgrad_ref(x, dz):
    """(dW, db, bound_w, bound_b): dW = x^T . dz and db = column sums of dz in float64; bound_w = gamma(M + 2) * (|x|^T . |dz|) and
    bound_b = gamma(M + 2) * sum |dz| per element (x None: dW and bound_w are None)."""
    dz64 = np.asarray(dz, dtype=np.float64)
    g = float(gamma(dz64.shape[0] + 2))
    db, bound_b = dz64.sum(0), g * np.abs(dz64).sum(0)
    if x is None:
        return None, db, None, bound_b
    x64 = np.asarray(x, dtype=np.float64)
    return x64.T @ dz64, db, g * (np.abs(x64).T @ np.abs(dz64)), bound_b


def scatter_ref(src, ids, base, dst0):
    """(sum, bound): dst0 with src[m] added to row ids[m] - base, in float64, and gamma(count + 1) * (|dst0| + sum |src rows|) per
    element, count = the rows added to that destination row."""
    rows = np.asarray(ids, dtype=np.int64) - int(base)
    src64 = np.asarray(src, dtype=np.float64)
    out, mag = np.array(dst0, dtype=np.float64), np.abs(np.asarray(dst0, dtype=np.float64))
    count = np.zeros(out.shape[0], dtype=np.int64)
    np.add.at(out, rows, src64)
    np.add.at(mag, rows, np.abs(src64))
    np.add.at(count, rows, 1)
    return out, gamma(count + 1)[:, None] * mag


def scatter_sequential_f32(src, ids, base, dst0):
    """The float32 result the owner kernel promises bit for bit: the rows of every id added in ascending position order, starting from
    the first one, and that sum added to dst0 once."""
    rows = np.asarray(ids, dtype=np.int64) - int(base)
    src = np.asarray(src, dtype=np.float32)
    out = np.array(dst0, dtype=np.float32)
    order = np.argsort(rows, kind='stable')                            # positions grouped by destination row, ascending inside a group
    starts = np.flatnonzero(np.r_[True, rows[order][1:] != rows[order][:-1]]) if len(order) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(order)]
    # one step adds the k-th position of every group that has one: float32 additions, element-wise, in position order per group
    acc = src[order[starts]].copy() if len(order) else np.zeros((0, src.shape[1]), np.float32)
    k = 1
    live = np.flatnonzero(ends - starts > k)
    while len(live):
        acc[live] = acc[live] + src[order[starts[live] + k]]
        k += 1
        live = live[ends[live] - starts[live] > k]
    if len(order):
        out[rows[order[starts]]] = out[rows[order[starts]]] + acc
    return out


def act_bwd_ref(dy, y, act):
    """dz = dy * act'(y) with y the layer OUTPUT: relu -> dy where y > 0, sigmoid -> dy y (1 - y), None -> dy."""
    dy64, y64 = np.asarray(dy, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if act == 'relu':
        return np.where(y64 > 0, dy64, 0.0)
    if act == 'sigmoid':
        return dy64 * y64 * (1.0 - y64)
    assert act is None
    return dy64.copy()


def fma_f32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, bit for bit: a * b is exact in float64 (two 24-bit significands), the float64 sum p + c is rounded
    once to 53 bits, and rounding that to float32 differs from rounding the exact sum only where the float64 sum was inexact AND landed
    exactly half way between two float32 values; there the sign of the float64 rounding error (TwoSum) says which neighbour is right."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # exact sum = s + err
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.where(s > r64, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))).astype(np.float64)
    half = (err != 0) & np.isfinite(s) & (s != r64) & (np.abs(s - r64) == np.abs(other - s))   # s exactly between r and its neighbour
    right = np.where(err > 0, np.maximum(r64, other), np.minimum(r64, other))
    r = np.where(half, right, r64)
    return r.astype(np.float32)


def row_affine_ref(a, scale, b=None):
    """(a + b) * scale[row]"""
    v = np.asarray(a, dtype=np.float64)
    if b is not None:
        v = v + np.asarray(b, dtype=np.float64)
    return v * np.asarray(scale, dtype=np.float64)[:, None]


L2_CLAMP = 1e-12


def l2norm_ref(z, act):
    """(inv, nrm, y): inv = 1 / sqrt(max(sum z^2, 1e-12)) per row, nrm = z * inv, y = act(nrm) (act 'relu' or None)."""
    z64 = np.asarray(z, dtype=np.float64)
    inv = 1.0 / np.sqrt(np.maximum((z64 * z64).sum(1), L2_CLAMP))
    nrm = z64 * inv[:, None]
    return inv, nrm, (np.maximum(nrm, 0.0) if act == 'relu' else nrm.copy())


def l2norm_bwd_ref(dy, z, act):
    """(dz, scale): the gradient of sum(dy * act(l2_normalize(z))) with respect to z in float64 — dn = dy * [nrm > 0] (relu) or dy,
    dz = inv * (dn - nrm * (nrm . dn)), and dz = inv * dn on a clamped row, where nrm = 1e6 * z is linear in z.  scale = inv * (|dn| +
    |nrm| * sum |nrm dn|) is the magnitude of what is added up per element: dz itself cancels (to exactly zero for one column), so an
    error relative to |dz| is unbounded and the tests measure it against this."""
    z64, dy64 = np.asarray(z, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    sq = (z64 * z64).sum(1)
    inv, nrm, _ = l2norm_ref(z64, act)
    dn = np.where(nrm > 0, dy64, 0.0) if act == 'relu' else dy64
    free = (sq > L2_CLAMP)[:, None]
    dot = np.where(free, (nrm * dn).sum(1, keepdims=True), 0.0)
    dz = inv[:, None] * (dn - nrm * dot)
    scale = inv[:, None] * (np.abs(dn) + np.abs(nrm) * np.where(free, np.abs(nrm * dn).sum(1, keepdims=True), 0.0))
    return dz, scale
