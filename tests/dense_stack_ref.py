"""Reference for the one-launch Dense-stack kernels (amar_dense_stack_f32 / amar_dense_stack_bwd_f32).  TEST INFRASTRUCTURE ONLY.

numpy float64, written from the formulas of include/amar_hip.h:
    forward   y_0 = X[ids],  y_{l+1} = act_l(y_l . W_l + b_l)                         (b_l absent: a zero bias)
    reverse   dZ_top = dYtop * act'(Ytop) (or dYtop itself),  dW_l = X_l^T . dZ_l,  db_l = column sums of dZ_l,
              dX_l = dZ_l . W_l^T,  dZ_{l-1} = dX_l * act'(X_l),  dX0 = dX_0
on the float32 operands widened exactly, together with the per-element bounds tests/test_dense_stack_forms_gpu.py holds the kernels
to.  Nothing here rounds to float32.  U = 2^-24 (tests/dense_bwd_ref.py, whose act_grad / dx_bound / dz_bound are reused).

Every bound below is derived from the float32 summation bound gamma_n = n U / (1 - n U) < (n + 1) U for n <= 130, or is a figure the
suite already uses for these kernels (SIGMOID_TOL, REDUCED_TOL); none was measured on the kernels.
"""
import numpy as np

from tests.dense_bwd_ref import U, act_grad, dx_bound, dz_bound

SIGMOID_TOL = 3e-6            # test_dense_stack_one_launch's figure for this kernel; applied per element (sigmoid outputs lie in (0, 1))
REDUCED_TOL = 5e-6            # test_dense_stack_bwd_one_launch's helpers.rel_err bound on the reduced dW / db


def activate(z, act):
    if act is None:
        return z
    if act == 'relu':
        return np.maximum(z, 0)
    if act == 'sigmoid':
        return 1 / (1 + np.exp(-z))
    raise ValueError(act)


def forward_layer(x, w, b, act):
    """(want, bound) of ONE layer from its float32 input `x` (the device's own output of the layer before): the bound covers this
    layer's arithmetic alone.  none / relu: K products, K additions (the bias among them) in float32, any order:
    |got - want| <= (K + 2) U (|x| . |W| + |b|); relu is 1-Lipschitz and exact.  sigmoid: __expf's error is no multiple of U."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b64 = np.zeros(w64.shape[1]) if b is None else np.asarray(b, dtype=np.float64)
    want = activate(x64 @ w64 + b64, act)
    if act == 'sigmoid':
        return want, np.full(want.shape, SIGMOID_TOL)
    return want, (w64.shape[0] + 2) * U * (np.abs(x64) @ np.abs(w64) + np.abs(b64))


def _abs_act_slope(y, act):
    y = np.asarray(y, dtype=np.float64)
    if act is None:
        return np.ones_like(y)
    return (y > 0).astype(np.float64) if act == 'relu' else np.abs(y * (1.0 - y))


def reverse(xs, ws, acts, top, top_is_dz):
    """The float64 chain and the error bound carried down it.  xs: the L + 1 saved activations (xs[0] the stack's input, xs[L] = Ytop),
    ws: the L kernels, top: dYtop.  Returns dict(dz=[L], err=[L], dx0, dx0_bound) with
        err[L-1] = dz_bound(dZ_top)                     (exact, or 4 U |dZ| under sigmoid': three roundings)
        e_dx_l   = (N_l + 2) U (|dZ_l| . |W_l|^T) + err[l] . |W_l|^T          (dx_bound plus the inherited error through the product)
        err[l-1] = e_dx_l * |act'(X_l)|  (+ 4 U |dZ_{l-1}| under sigmoid')     relu' masks are exact: they depend on X_l alone
        dx0_bound = e_dx_0"""
    L = len(ws)
    xs64 = [np.asarray(x, dtype=np.float64) for x in xs]
    ws64 = [np.asarray(w, dtype=np.float64) for w in ws]
    top_act = None if top_is_dz else acts[L - 1]
    dz = act_grad(top, xs64[L], top_act)
    err = dz_bound(dz, top_act)
    dzs, errs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        dzs[l], errs[l] = dz, err
        n = ws64[l].shape[1]
        dx = dz @ ws64[l].T
        e_dx = dx_bound(n, np.abs(dz) @ np.abs(ws64[l]).T) + err @ np.abs(ws64[l]).T
        if l > 0:
            dz = act_grad(dx, xs64[l], acts[l - 1])
            err = e_dx * _abs_act_slope(xs64[l], acts[l - 1]) + dz_bound(dz, acts[l - 1])
    return dict(dz=dzs, err=errs, dx0=dx, dx0_bound=e_dx)


def partials(x, dz, err, rows):
    """The per-workgroup partial sums of one layer: group g owns rows [g rows, (g + 1) rows).  Returns (dw [G, K, N], dw_bound,
    db [G, N], db_bound, dw_mag [K, N], db_mag [N]):
        |got - want| <= (rows + 2) U (|X|^T . |dZ|) + |X|^T . err     over the group's rows only; db likewise with ones for X.
    *_mag: the magnitudes over ALL rows (for the bound of a reduced sum)."""
    x64 = np.asarray(x, dtype=np.float64)
    M = x64.shape[0]
    G = -(-M // rows)
    pad = G * rows - M
    xp, zp, ep = (np.concatenate([a, np.zeros((pad, a.shape[1]))]).reshape(G, rows, a.shape[1]) for a in (x64, dz, err))
    xt, xt_abs = xp.transpose(0, 2, 1), np.abs(xp).transpose(0, 2, 1)  # [G, K, rows]
    dw, dw_mag = xt @ zp, xt_abs @ np.abs(zp)
    dw_bound = (rows + 2) * U * dw_mag + xt_abs @ ep
    db, db_mag = zp.sum(1), np.abs(zp).sum(1)
    db_bound = (rows + 2) * U * db_mag + ep.sum(1)
    return dw, dw_bound, db, db_bound, dw_mag.sum(0), db_mag.sum(0)


def reduced_bound(part_bound, mag_all, groups):
    """A reduced gradient = the G partials added one after the other in float32: the partials' own bounds, plus G additions of values
    whose magnitudes sum to at most mag_all: (G + 1) U mag_all."""
    return part_bound.sum(0) + (groups + 1) * U * mag_all
