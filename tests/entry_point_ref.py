"""Float64 restatements of the C-ABI entry points that tests/test_entry_points_gpu.py calls directly.  TEST INFRASTRUCTURE ONLY.

Plain numpy, written from the formulas of include/amar_hip.h; no torch, no device.  tests/test_entry_points_cpu.py pins every function
here to what the project already trusts (oracle.models / oracle.layers / oracle.train, torch float64 autograd, the float32 Keras expression
of test_training_kernels), so the reference of the GPU tests is itself checked on a machine without a GPU.

Error scales.  A sum of products is compared element by element against tol * (sum of |terms| of THAT element), not against the largest
magnitude of the array (helpers.rel_err).  For the two-branch head the terms are the scorer's; behind a trunk of fewer than 16 units they are
those of the last two layers (see `dual_head`), because a numpy float32 evaluation of a 4-wide trunk already misses 5e-6 of the scorer's
terms alone (they vanish where the ReLU outputs are nearly zero).  test_entry_points_cpu.py holds the numpy float32 evaluation against the
resulting bound.
"""
import numpy as np

F32_EPS = 2.0 ** -24                                                   # unit roundoff of float32
NARROW_TRUNK = 16                                                      # trunk widths below this get the two-layer scale of `dual_head`


def act(x, name):
    if name in (None, 'none', 'linear'):
        return x
    if name == 'relu':
        return np.maximum(x, 0)
    if name == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-x))
    raise ValueError(name)


# ---- two-branch head (amar_dual_chain_f32) --------------------------------------------------------------------------------------

def draw_dual_head(rng, D, W, n_branch, n_trunk, table_rows, table_std=1.5):
    """Seeded tables and weights of one head: 2 x 2 tables [rows, D] with entries of a few units, Glorot-uniform kernels (the product's
    initialiser) and biases U(+-0.2); n_trunk counts the scorer (trunk dims [2D, W, .., W, 1])."""
    g = lambda k, n: rng.uniform(-1, 1, (k, n)).astype(np.float32) * np.float32(np.sqrt(6.0 / (k + n)))    # noqa: E731
    b = lambda n: rng.uniform(-0.2, 0.2, n).astype(np.float32)                                            # noqa: E731
    tdims = [2 * D] + [W] * (n_trunk - 1) + [1]
    return {'A': [(rng.standard_normal((table_rows, D)) * table_std).astype(np.float32) for _ in range(2)],
            'B': [(rng.standard_normal((table_rows, D)) * table_std).astype(np.float32) for _ in range(2)],
            'branch': [[(g(D, D), b(D)) for _ in range(n_branch)] for _ in range(2)],
            'trunk': [(g(k, n), b(n)) for k, n in zip(tdims[:-1], tdims[1:])], 'trunk_dims': tdims}


def dual_head(A, B, rows_a, rows_b, branch, trunk, in_act, branch_acts, trunk_acts):
    """(out [P], scale [P]) in float64.  A, B: two tables each; rows_*: two index arrays each (ids - base, or arange(P) for a table read
    in place); branch: two lists of (kernel, bias); trunk: list of (kernel, bias), the last one the 1-unit scorer.
    scale = sum_k |w_k x_k| + |bias|: the scorer's own terms on the float64 activations x.  Behind a trunk narrower than a 16-wide tile
    (W < NARROW_TRUNK) the term sums u_k = (|x'| . |W| + |b|)_k of the layer that produced x_k are added through |w_k|: there the scorer's
    few terms can all (nearly) vanish while that layer's rounding error still arrives."""
    f = lambda t: np.asarray(t, dtype=np.float64)                                                         # noqa: E731
    xs, us = [], []
    for br in range(2):
        a, b = f(A[br])[rows_a[br]], f(B[br])[rows_b[br]]
        x, u = act(a + b, in_act), np.abs(a) + np.abs(b)
        for (w, bias), name in zip(branch[br], branch_acts):
            x, u = act(x @ f(w) + f(bias), name), np.abs(x) @ np.abs(f(w)) + np.abs(f(bias))
        xs.append(x)
        us.append(u)
    x, u = np.concatenate(xs, axis=1), np.concatenate(us, axis=1)
    for (w, bias), name in zip(trunk[:-1], trunk_acts[:-1]):
        x, u = act(x @ f(w) + f(bias), name), np.abs(x) @ np.abs(f(w)) + np.abs(f(bias))
    w, bias = trunk[-1]
    z = x @ f(w) + f(bias)
    scale = (np.abs(x) + (u if x.shape[1] < NARROW_TRUNK else 0.0)) @ np.abs(f(w)) + np.abs(f(bias))
    return act(z, trunk_acts[-1])[:, 0], scale[:, 0]


def dual_head_f32(A, B, rows_a, rows_b, branch, trunk, in_act, branch_acts, trunk_acts):
    """The same head in numpy float32 (the error of this evaluation is what the bounds of the device kernels are held against)."""
    one = np.float32(1)
    a32 = lambda x, n: np.maximum(x, 0) if n == 'relu' else (one / (one + np.exp(-x)) if n == 'sigmoid' else x)   # noqa: E731
    xs = []
    for br in range(2):
        x = a32(np.asarray(A[br], np.float32)[rows_a[br]] + np.asarray(B[br], np.float32)[rows_b[br]], in_act)
        for (w, bias), name in zip(branch[br], branch_acts):
            x = a32(x @ w + bias, name)
        xs.append(x)
    x = np.concatenate(xs, axis=1)
    for (w, bias), name in zip(trunk, trunk_acts):
        x = a32(x @ w + bias, name)
    assert x.dtype == np.float32
    return x[:, 0]


# ---- element-wise head kernels ---------------------------------------------------------------------------------------------------

def attention_weight(ta, tb):
    """wa of FusionLayer('attention'): the two-way softmax over tanh(ta), tanh(tb) is sigmoid(tanh ta - tanh tb)."""
    return 1.0 / (1.0 + np.exp(np.tanh(tb) - np.tanh(ta)))


def attention_mix(a, b, ta, tb):
    wa = attention_weight(ta, tb)
    return wa * a + (1.0 - wa) * b


def attention_mix_bwd(dout, a, b, ta, tb):
    """(dA, dB, dTA, dTB): the direct paths and the gradients of the two products."""
    ca, cb = np.tanh(ta), np.tanh(tb)
    wa = 1.0 / (1.0 + np.exp(cb - ca))
    g = dout * (a - b) * wa * (1.0 - wa)
    return dout * wa, dout * (1.0 - wa), g * (1.0 - ca * ca), -g * (1.0 - cb * cb)


def add3_act(a, b, c, name):
    return act(a + b + c, name)


def locality_scale(x, w):
    return x / (1.0 + np.exp(-w))[:, None]


def locality_scale_bwd(dout, x, w):
    """(dX, dw): dX = dOut * s, dw[row] = s (1 - s) * (dOut[row] . X[row]), s = sigmoid(w[row])."""
    s = 1.0 / (1.0 + np.exp(-w))
    return dout * s[:, None], s * (1.0 - s) * np.sum(dout * x, axis=1)


def worst_scaled_error(fn, args, scales):
    """max over every output of |fn(float32 args) - fn(float64 args)| / scale: the error a float32 numpy evaluation of the
    SAME formula leaves, the constant the kernels' bounds are taken from.  scales: one array per output."""
    a64 = [np.asarray(v, dtype=np.float64) for v in args]
    a32 = [np.asarray(v, dtype=np.float32) for v in args]
    with np.errstate(over='ignore', under='ignore'):
        r64, r32 = fn(*a64), fn(*a32)
    if not isinstance(r64, tuple):
        r64, r32 = (r64,), (r32,)
    worst = 0.0
    for want, got, sc in zip(r64, r32, scales):
        assert got.dtype == np.float32, "the float32 evaluation was promoted"
        live = sc > 0
        worst = max(worst, float((np.abs(got.astype(np.float64) - want)[live] / sc[live]).max()))
    return worst


def scaled_error(got, want, scale):
    """max |got - want| / scale over the elements with a non-zero scale; elements with scale 0 must match exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    live = scale > 0
    assert np.array_equal(got[~live], want[~live])
    return float((np.abs(got - want)[live] / scale[live]).max()) if live.any() else 0.0


# float32 forms of the same formulas (every constant float32, so numpy does not promote): what `worst_scaled_error` evaluates
def _one(x):
    return x.dtype.type(1)


def attention_mix_t(a, b, ta, tb):
    wa = _one(a) / (_one(a) + np.exp(np.tanh(tb) - np.tanh(ta)))
    return wa * a + (_one(a) - wa) * b


def attention_mix_bwd_t(dout, a, b, ta, tb):
    one = _one(a)
    ca, cb = np.tanh(ta), np.tanh(tb)
    wa = one / (one + np.exp(cb - ca))
    g = dout * (a - b) * wa * (one - wa)
    return dout * wa, dout * (one - wa), g * (one - ca * ca), -g * (one - cb * cb)


def sigmoid_t(x):
    return _one(x) / (_one(x) + np.exp(-x))


def locality_scale_t(x, w):
    return x / (_one(x) + np.exp(-w))[:, None]


def locality_scale_bwd_t(dout, x, w):
    s = _one(x) / (_one(x) + np.exp(-w))
    return dout * s[:, None], s * (_one(x) - s) * np.sum(dout * x, axis=1, dtype=x.dtype)


# ---- optimizer kernels --------------------------------------------------------------------------------------------------------------

def adam_lr_t(t, lr, b1, b2):
    """keras.optimizers.Adam's bias-corrected step size for step t (t = 1 for the first step), float64."""
    return float(lr) * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)


def adam_step(w, g, m, v, lr_t, b1, b2, eps, l2=0.0):
    """(w, m, v) after amar_adam_dev_f32: g' = g + 2 l2 w, the two moments, w -= lr_t m / (sqrt(v) + eps)."""
    w, g, m, v = (np.asarray(t, dtype=np.float64) for t in (w, g, m, v))
    g = g + 2.0 * l2 * w
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def sum_groups_f32(partials):
    """Partial gradients [G, n] added in the order 0 .. G-1 in float32: the explicit reduction amar_adam_multi_f32 promises the bits of."""
    partials = np.asarray(partials, dtype=np.float32)
    total = partials[0].copy()
    for k in range(1, partials.shape[0]):
        total = total + partials[k]
    return total


def bce_terms_f32(p, y):
    """(loss_terms, dz) of Keras' backend binary_crossentropy on probabilities, evaluated in float32 as Keras does (1 - 1e-7 is not
    representable: the upper clip lands on 1 - 1.19e-7); dz = dL/dlogit through the final sigmoid, L the mean over the batch."""
    p, y = np.asarray(p, dtype=np.float32), np.asarray(y, dtype=np.float32)
    e32, one = np.float32(1e-7), np.float32(1)
    pc = np.clip(p, e32, one - e32)
    terms = -(y * np.log(pc + e32) + (one - y) * np.log(one - pc + e32))
    inside = (p >= e32) & (p <= one - e32)
    dz = -(y / (pc + e32) - (one - y) / (one - pc + e32)) / np.float32(len(p)) * inside * p * (one - p)
    return terms, dz


def bce_mean_loss(p, y):
    """The float64 mean loss with the clip points float32 arithmetic produces (float32(1e-7), 1 - float32(1e-7) rounded to float32)."""
    e32 = np.float32(1e-7)
    lo, hi, eps = float(e32), float(np.float32(1) - e32), float(e32)
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.float64)
    pc = np.clip(p, lo, hi)
    return float(-np.mean(y * np.log(pc + eps) + (1.0 - y) * np.log(1.0 - pc + eps)))


def ulp_neighbours(x):
    """(next float32 below, x, next float32 above)."""
    x = np.float32(x)
    return np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))


# ---- seeded inputs shared by the CPU and the GPU tests, and the bounds taken from them ------------------------------------------------

PLANTED_T = (0.0, 20.0, -20.0, 100.0, -100.0)                          # +-20 and +-100 saturate tanh: wa reaches sigmoid(+-2)


def draw_attention_inputs(rng, M, D):
    """(dout, a, b, ta, tb) float32 [M, D]: ta, tb ~ N(0, 3^2); the first 25 elements carry every pair of PLANTED_T, the next ones a == b."""
    dout, a, b = (rng.standard_normal((M, D)).astype(np.float32) for _ in range(3))
    ta, tb = ((rng.standard_normal((M, D)) * 3).astype(np.float32) for _ in range(2))
    n = min(M * D, 25)
    ta.reshape(-1)[:n] = [PLANTED_T[k // 5] for k in range(n)]
    tb.reshape(-1)[:n] = [PLANTED_T[k % 5] for k in range(n)]
    b.reshape(-1)[25:40] = a.reshape(-1)[25:40]
    return dout, a, b, ta, tb


def attention_scales(dout, a, b):
    """Forward: max(|a|, |b|).  Reverse: |dOut| for the direct paths, |dOut| |a - b| for dTA / dTB (1 - tanh^2 cancels near saturation,
    so the error is measured against what multiplies it, not against the result)."""
    dout, a, b = (np.asarray(t, dtype=np.float64) for t in (dout, a, b))
    d, ab = np.abs(dout), np.abs(a - b)
    return np.maximum(np.abs(a), np.abs(b)), (d, d, d * ab, d * ab)


def draw_locality_inputs(rng, M, W):
    """(dout, x, w): w ~ N(0, 2^2) with +-100 planted in the first rows (sigmoid' = 0 there: dw must be 0, not NaN)."""
    dout, x = (rng.standard_normal((M, W)).astype(np.float32) for _ in range(2))
    w = (rng.standard_normal(M) * 2).astype(np.float32)
    w[:min(M, 4)] = [100.0, -100.0, 100.0, -100.0][:min(M, 4)]
    return dout, x, w


def locality_scales(dout, x):
    dout, x = np.asarray(dout, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.abs(x), (np.abs(dout), np.sum(np.abs(dout * x), axis=1))


def draw_add3_inputs(rng, M, W, name):
    """(a, b, c): N(0, 1) rows; sums of +-100 planted for the sigmoid (results 1 and 0), exact-zero sums for ReLU."""
    a, b, c = (rng.standard_normal((M, W)).astype(np.float32) for _ in range(3))
    n = min(M * W, 6)
    fa, fb, fc = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    if name == 'sigmoid':
        fa[:n], fb[:n], fc[:n] = [40, -40, 30, -30, 100, -100][:n], [35, -35, 30, -30, 0, 0][:n], [25, -25, 40, -40, 0, 0][:n]
    else:
        fa[:n], fb[:n], fc[:n] = [1.5, -2, 0, 0.25, 3, -0.0][:n], [-1, 1, 0, 0.25, -1, 0.0][:n], [-0.5, 1, 0, -0.5, -2, -0.0][:n]
    return a, b, c


def add3_scale(a, b, c, name):
    """|a| + |b| + |c| for the sum; through the sigmoid its derivative s (1 - s), plus the result's own rounding (s itself); results below
    float32's normal range carry absolute accuracy only, hence the floor."""
    a, b, c = (np.asarray(t, dtype=np.float64) for t in (a, b, c))
    terms = np.abs(a) + np.abs(b) + np.abs(c)
    if name != 'sigmoid':
        return terms
    s = 1.0 / (1.0 + np.exp(-(a + b + c)))
    return s + terms * s * (1.0 - s) + 1e-30


def add3_act_t(a, b, c, name):
    v = a + b + c
    return sigmoid_t(v) if name == 'sigmoid' else (np.maximum(v, 0) if name == 'relu' else v)


# A kernel is allowed KERNEL_FACTOR times the worst scaled error of the float32 numpy evaluation (`*_t` above) against float64 on
# draw_*_inputs(default_rng(2024), 5000, 64): the device's expf / tanhf are accurate to 1-2 ulp rather than correctly rounded, and the order
# of its few operations may differ.  `f32_numpy_figures()` measures them (on the CPU, whoever calls it); F32_NUMPY_FIGURES records what it
# gave when the tests were written (tests/test_entry_points_cpu.py keeps the record within 5 % of the measurement).
KERNEL_FACTOR = 4.0
F32_NUMPY_FIGURES = {'attention_mix': 2.197e-7, 'attention_mix_bwd': 1.367e-7, 'locality_scale': 1.124e-7, 'locality_scale_bwd': 1.313e-7,
                     'add3_none': 1.121e-7, 'add3_relu': 1.131e-7, 'add3_sigmoid': 1.372e-7}
_FIGURES = {}


def f32_numpy_figures():
    if not _FIGURES:
        rng = np.random.default_rng(2024)
        dout, a, b, ta, tb = draw_attention_inputs(rng, 5000, 64)
        fs, bs = attention_scales(dout, a, b)
        _FIGURES['attention_mix'] = worst_scaled_error(attention_mix_t, (a, b, ta, tb), (fs,))
        _FIGURES['attention_mix_bwd'] = worst_scaled_error(attention_mix_bwd_t, (dout, a, b, ta, tb), bs)
        dout, x, w = draw_locality_inputs(rng, 5000, 64)
        fs, bs = locality_scales(dout, x)
        _FIGURES['locality_scale'] = worst_scaled_error(locality_scale_t, (x, w), (fs,))
        _FIGURES['locality_scale_bwd'] = worst_scaled_error(locality_scale_bwd_t, (dout, x, w), bs)
        for name in ('none', 'relu', 'sigmoid'):
            a, b, c = draw_add3_inputs(rng, 5000, 64, name)
            _FIGURES['add3_' + name] = worst_scaled_error(lambda p, q, r: add3_act_t(p, q, r, name), (a, b, c), (add3_scale(a, b, c, name),))
    return dict(_FIGURES)


def adam_scales(w, parts, m, v, lr_t, b1, b2, eps, l2):
    """Per-element scales (w, m, v) of one Adam step whose gradient is the sum of `parts` [G, n]: the moments against the sum of the
    magnitudes of their terms, the weight against the update those magnitudes would give (the moment's cancellation reaches the update
    undiminished) plus |w| (the stored result carries its rounding: with 1e-6 of this scale the update itself is held to 1e-6 of its
    terms + 1e-6 |w|, where float32 storage alone costs 6e-8 |w|)."""
    parts = np.asarray(parts, dtype=np.float64).reshape(-1, np.size(w))
    w64, m64, v64 = (np.asarray(t, dtype=np.float64) for t in (w, m, v))
    g = np.abs(parts).sum(0) + 2.0 * l2 * np.abs(w64)
    ms = b1 * np.abs(m64) + (1.0 - b1) * g
    vs = b2 * np.abs(v64) + (1.0 - b2) * g * g
    v_true = b2 * v64 + (1.0 - b2) * (parts.sum(0) + 2.0 * l2 * w64) ** 2
    return lr_t * ms / (np.sqrt(v_true) + eps) + np.abs(w64), ms, vs
