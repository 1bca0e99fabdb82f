"""Reference for amar_dense_bwd_f32 (the reverse pass of one linear map).  TEST INFRASTRUCTURE ONLY.

numpy float64, written from the formulas of include/amar_hip.h:
    dZ = dY * act'(Y)      (Y the layer's OUTPUT: relu' = [Y > 0], sigmoid' = Y (1 - Y))
    dX = dZ . W^T          dW = X^T . dZ          db = column sums of dZ
on the float32 operands widened exactly, plus the magnitudes the per-element bounds of tests/test_dense_bwd_routes_gpu.py are taken
against.  Nothing here rounds to float32: what the kernels lose to their own float32 arithmetic is what the tests bound.
"""
import numpy as np

U = 2.0 ** -24                                                         # unit roundoff of float32


def act_grad(dy, y, act):
    dy = np.asarray(dy, dtype=np.float64)
    if act is None:
        return dy.copy()
    y = np.asarray(y, dtype=np.float64)
    if act == 'relu':
        return dy * (y > 0)                                            # (-0.0 > 0 is False: no gradient through a negative zero)
    if act == 'sigmoid':
        return dy * y * (1.0 - y)
    raise ValueError(act)


def dense_bwd(x, y, dy, w, act):
    """dict(dz, dx, dw, db, dx_mag): the last is |dZ| . |W|^T, the sum of magnitudes a float32 dot product's error is relative to.
    x / w may be None (no dw / no dx)."""
    dz = act_grad(dy, y, act)
    out = {'dz': dz, 'db': dz.sum(0), 'dx': None, 'dw': None, 'dx_mag': None}
    if w is not None:
        w64 = np.asarray(w, dtype=np.float64)
        out['dx'], out['dx_mag'] = dz @ w64.T, np.abs(dz) @ np.abs(w64).T
    if x is not None:
        out['dw'] = np.asarray(x, dtype=np.float64).T @ dz
    return out


def dx_bound(n, dx_mag, extra_mag=0.0):
    """|got - want| <= (N + 2) 2^-24 (|dZ| . |W|^T) for a float32 sum of N <= 128 products in any order (N - 1 additions and one
    multiplication round each term at most N times: gamma_N = N u / (1 - N u) < (N + 1) u; dZ itself carries up to three roundings under
    sigmoid').  extra_mag: the magnitude of a value the sum is added to (accumulate_dx: one more term, one more rounding, inside the + 2)."""
    return (n + 2) * U * (dx_mag + extra_mag)


def dz_bound(dz, act):
    """dZ is a copy of dY (None) or a selection from it (relu): exact.  sigmoid': dy * y * (1 - y) is two multiplications and a
    subtraction in float32, three roundings, (1 + u)^3 - 1 < 4 u."""
    return 0.0 * np.abs(dz) if act in (None, 'relu') else 4 * U * np.abs(dz)
