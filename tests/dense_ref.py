"""What tests/test_dense_route_cpu.py and tests/test_dense_forms_gpu.py share (numpy only): the float64 restatement of amar_dense_f32 with the
per-element magnitude of its terms, the error bounds derived from it, and ONE table of named cases, each with the route it must take —
the host test asks amar_dense_route for every row with made-up addresses, the GPU test asks it on the live tensors and then launches."""
import collections
import functools

import numpy as np

U = 2.0 ** -24                                                         # float32 unit roundoff

ACTS = ('none', 'relu', 'sigmoid')                                     # capi's names: None, 'relu', 'sigmoid'


def capi_act(act):
    return None if act == 'none' else act


# ---- float64 restatement ------------------------------------------------------------------------------------------------------------------
def pre_activation(x, w, b=None, ids=None, w_transposed=False):
    """z = X[ids] . W + b in float64 and S = sum_k |x_k| |w_k| + |b|, per element.  W is [K, N], or [N, K] with w_transposed."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if ids is not None:
        x64 = x64[np.asarray(ids)]
    if w_transposed:
        w64 = w64.T
    z, s = x64 @ w64, np.abs(x64) @ np.abs(w64)
    if b is not None:
        b64 = np.asarray(b, dtype=np.float64)
        z, s = z + b64, s + np.abs(b64)
    return z, s


def sigmoid(z):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-z))


def activation(z, act):
    return np.maximum(z, 0.0) if act == 'relu' else sigmoid(z) if act == 'sigmoid' else z


def dense_ref(x, w, b=None, act='none', ids=None, w_transposed=False):
    """(act(X[ids] . W + b), S) in float64."""
    z, s = pre_activation(x, w, b, ids, w_transposed)
    return activation(z, act), s


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------
# The f32 matrix instruction is a k-ordered fma chain from 0: K roundings, then one for the bias; k padded to the tile contributes exact
# zeros.  The recursive-summation bound for K + 1 terms is gamma(K + 1) S; (K + 3) u S is that figure with room for its own 1 / (1 - n u)
# (K <= 2^20).  Derived, not measured.  ReLU is 1-Lipschitz: the same bound.
def linear_bound(K, s):
    return (K + 3) * U * s


# The sigmoid is 1/4-Lipschitz, so the error of z arrives divided by 4; on top comes what evaluating 1 / (1 + exp(-z)) in float32 on a
# float32 z leaves.  sigmoid_f32_eval_error measures that with numpy float32 against float64 on the z of every case below
# (measure_sigmoid_term: SIGMOID_F32_MEASURED is its record, tests/test_dense_route_cpu.py re-measures it); the device's expf may differ
# from numpy's by an ulp, hence the factor 2.  The suite's own figure for sigmoid outputs is 1e-6 absolute: the constant stays below it.
SIGMOID_F32_MEASURED = 9.37e-8
SIGMOID_FACTOR = 2.0
SIGMOID_F32_EVAL = SIGMOID_FACTOR * SIGMOID_F32_MEASURED


def sigmoid_bound(K, s):
    return linear_bound(K, s) / 4.0 + SIGMOID_F32_EVAL


def bound(K, s, act):
    return sigmoid_bound(K, s) if act == 'sigmoid' else linear_bound(K, s)


def sigmoid_f32_eval_error(z):
    """max |float32 evaluation - float64 value| of 1 / (1 + exp(-z)) over the float32 roundings of z."""
    zf = np.asarray(z).astype(np.float32)
    with np.errstate(over='ignore'):
        got = np.float32(1) / (np.float32(1) + np.exp(-zf))
    assert got.dtype == np.float32
    return float(np.abs(got.astype(np.float64) - sigmoid(zf.astype(np.float64))).max())


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
# kernel / vec_x / vec_w / w_trans: the route the case must take.  x_shift: X is a view one float into an aligned buffer whose leading
# dimension stays a multiple of 4; w_shift: W is a contiguous view one float into a flat buffer.
Case = collections.namedtuple('Case', 'name M K N kernel vec_x vec_w w_trans x_shift w_shift')


def _case(kernel, M, K, N, vec_x=True, vec_w=True, w_trans=False, x_shift=False, w_shift=False):
    name = '{}{}{}-{}x{}x{}{}{}'.format(kernel, '' if kernel != 'guarded' else '_' + 'ft'[vec_x] + 'ft'[vec_w], '_wt' if w_trans else '',
                                        M, K, N, '_xshift' if x_shift else '', '_wshift' if w_shift else '')
    return Case(name, M, K, N, kernel, vec_x, vec_w, w_trans, x_shift, w_shift)


CASES = (
    # 64 x 64 tiles, two k-tiles of 32 in flight: one, three and five k-tiles (the prologue's second fetch and the loop's second half each
    # taken and not taken), one row, a full tile, one row past it, three row tiles, the last M
    _case('small', 1, 32, 64), _case('small', 64, 32, 64), _case('small', 65, 96, 128), _case('small', 130, 160, 64), _case('small', 4096, 32, 64),
    # guard-free 128 x 64: the first M past small, K = 16 (one k-tile), K = 48 with three column blocks, nine row tiles padded to 16
    _case('full', 4097, 32, 64), _case('full', 130, 16, 64), _case('full', 333, 48, 192), _case('full', 1100, 48, 256),
    # 128 x 128: one valid row in the last of 25 row tiles (tiles 25..31 return at once), three k-tiles, two column blocks, one
    _case('tile128', 3073, 16, 1024), _case('tile128', 3073, 48, 1024), _case('tile128', 15361, 16, 256), _case('tile128', 31745, 16, 128),
    _case('guarded', 130, 24, 24), _case('guarded', 257, 20, 68),
    _case('guarded', 64, 17, 64, vec_x=False), _case('guarded', 200, 32, 64, vec_x=False, x_shift=True),
    _case('guarded', 100, 48, 1, vec_w=False), _case('guarded', 64, 32, 66, vec_w=False), _case('guarded', 64, 32, 64, vec_w=False, w_shift=True),
    _case('guarded', 64, 17, 65, vec_x=False, vec_w=False), _case('guarded', 1, 1, 1, vec_x=False, vec_w=False),
    # W transposed ([N, K]): K and N tails with three column blocks, the reverse of a 768 -> 256 layer, every vec pair
    _case('guarded', 130, 100, 132, w_trans=True), _case('guarded', 300, 256, 768, w_trans=True),
    _case('guarded', 64, 17, 65, vec_x=False, vec_w=False, w_trans=True), _case('guarded', 129, 64, 200, w_trans=True),
    _case('guarded', 64, 17, 64, vec_x=False, w_trans=True), _case('guarded', 64, 32, 66, vec_w=False, w_trans=True),
)
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

TABLE_EXTRA = 37                                                       # rows of the gathered table beyond M
VARIANTS = tuple((with_bias, with_ids) for with_bias in (True, False) for with_ids in (False, True))


def expected_grid(case):
    """(grid_x, grid_y, n_col_blocks) the case's kernel needs."""
    if case.kernel == 'small':
        return -(-case.M // 64), case.N // 64, case.N // 64
    ncb = case.N // 128 if case.kernel == 'tile128' else -(-case.N // 64)
    return -(-(-(-case.M // 128)) // 8) * 8 * ncb, 1, ncb


@functools.lru_cache(maxsize=2)
def case_inputs(name):
    """The case's float32 operands: table [M + TABLE_EXTRA, K] (X is its first M rows, or table[ids]), W ([K, N], or [N, K] transposed),
    bias [N], and ids [M] int32 — out of order, with repeats, over the whole table."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng([c.M, c.K, c.N, int(c.w_trans), int(c.x_shift), int(c.w_shift)])
    table = rng.standard_normal((c.M + TABLE_EXTRA, c.K)).astype(np.float32)
    w = rng.uniform(-0.3, 0.3, (c.N, c.K) if c.w_trans else (c.K, c.N)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, c.N).astype(np.float32)
    ids = rng.integers(0, c.M + TABLE_EXTRA, c.M).astype(np.int32)
    if c.M > 2:
        ids[0], ids[1], ids[2] = c.M + TABLE_EXTRA - 1, 0, c.M + TABLE_EXTRA - 1          # the last row, the first, a repeat: not ascending
    for t in (table, w, b, ids):
        t.setflags(write=False)
    return table, w, b, ids


@functools.lru_cache(maxsize=2)
def case_reference(name, with_bias, with_ids):
    """(z, S) of the case in float64 (read-only; the activations follow from z)."""
    c = CASE_BY_NAME[name]
    table, w, b, ids = case_inputs(name)
    z, s = pre_activation(table if with_ids else table[:c.M], w, b if with_bias else None, ids if with_ids else None, c.w_trans)
    z.setflags(write=False)
    s.setflags(write=False)
    return z, s


def measure_sigmoid_term():
    """The worst float32 evaluation error of the sigmoid over the z of every case and variant."""
    return max(sigmoid_f32_eval_error(case_reference(c.name, with_bias, with_ids)[0]) for c in CASES for with_bias, with_ids in VARIANTS)
