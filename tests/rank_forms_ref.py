"""Reference and form grid for the score stage the three fused rankers share (csrc/amar_rank_score.inc: amar_recommend_f32,
amar_recommend_group_f32, amar_rank_of_f32), and a Python restatement of their host-side route (amar_rank_route).

    score(u, i) = rest( in_act( Tu[u] + Ti[i] ) )        rest = Dense layers, then Dense(1): every layer and the dot with its own
                                                         activation out of None / 'relu' / 'sigmoid'

`scores` evaluates that in numpy at a chosen precision: float64 is the reference, float32 only sizes the tolerance (`bound`).
FORMS holds one head per way the fragment can go wrong; `build` draws its weights and tables.  Plain numpy; no library code."""
import collections

import numpy as np

N_USERS = 19                                  # two workgroups of 16 selectors, the second one partly filled
TIE_ROWS = lambda n: (1, n // 2, n - 1)       # item rows that hold the same vector when n > 4: exact ties by construction


def act(x, name):
    if name is None:
        return x
    if name == 'relu':
        return np.maximum(x, x.dtype.type(0))
    if name == 'sigmoid':
        one = x.dtype.type(1)
        return one / (one + np.exp(-x))
    raise ValueError(name)


def pre_scores(tu, ti, layers, acts, in_act, dtype):
    """[n_users, n_items] in `dtype`: the dot's value before its activation.  layers = [(W [K, N], b [N])], the last one N = 1;
    acts = one name per layer (the last one is the dot's and is not applied here)."""
    tu, ti = np.asarray(tu, dtype=dtype), np.asarray(ti, dtype=dtype)
    x = act(tu[:, None, :] + ti[None, :, :], in_act)
    for (w, b), a in zip(layers[:-1], acts[:-1]):
        x = act(x @ np.asarray(w, dtype=dtype) + np.asarray(b, dtype=dtype), a)
    w, b = layers[-1]
    return (x @ np.asarray(w, dtype=dtype) + np.asarray(b, dtype=dtype))[..., 0]


def scores(tu, ti, layers, acts, in_act, dtype=np.float64):
    out = act(pre_scores(tu, ti, layers, acts, in_act, dtype), acts[-1])
    assert out.dtype == dtype
    return out


def bound(s32, s64):
    """What a float32 evaluation in another summation order may differ from float64 by: 8 x the numpy float32 restatement's own
    error (<= 128 terms per layer added in another order), and never below the 1e-6 the sigmoid-ended tests already hold."""
    return max(1e-6, 8.0 * float(np.abs(s32.astype(np.float64) - s64).max()))


# ---- the form grid -------------------------------------------------------------------------------------------------------------
# ld: 'c1' contiguous tables, '+4' and 'x2' column windows of wider NaN-filled tensors (ld = c1 + 4, 2 c1) at a column offset of 4.
# dot_bias: None = drawn like the others; ('zero_share', q): set so that the share q of all pairs has a negative pre-activation
# (a relu dot then returns exactly 0 for them).
Form = collections.namedtuple('Form', 'name c1 hidden in_act acts dot_act ld dot_bias seed what')


def _f(name, c1, hidden, what, in_act='relu', acts=None, dot_act='sigmoid', ld='c1', dot_bias=None, seed=0):
    acts = ['relu'] * len(hidden) if acts is None else list(acts)
    assert len(acts) == len(hidden)
    return Form(name, c1, list(hidden), in_act, acts, dot_act, ld, dot_bias, seed, what)


RANK_MAX_LAYERS = 8
FORMS = [
    _f('c1_4', 4, [16], 'ragged first k-step: one float4 of sixteen features (f < c1 guard, lane groups 1..3 idle)', ld='+4'),
    _f('c1_20', 20, [16], 'ragged second k-step: c1 % 16 == 4', ld='x2'),
    _f('c1_36', 36, [24], 'ragged third k-step, MAXT 4'),
    _f('c1_48', 48, [48], 'the default head of the models: 48 -> 48 -> 1', ld='+4'),
    _f('c1_52', 52, [32], 'ragged fourth k-step: c1 % 16 == 4, MAXT 4', ld='x2'),
    _f('c1_100', 100, [16], 'ragged seventh k-step, MAXT 8 from c1 alone', ld='+4'),
    _f('c1_124', 124, [40], 'ragged last k-step of the widest c1: c1 % 16 == 12', ld='x2'),
    _f('hid_2', 16, [2], 'a hidden layer of two units: fourteen padded rows in its only tile'),
    _f('hid_3_17', 32, [3, 17], 'odd widths 3 and 17: a padded tile row count and a second tile of one row'),
    _f('hid_33_65', 64, [33, 65], 'widths one past a tile edge, the second one past MAXT 4: the widest layer is the last hidden one'),
    _f('hid_127', 32, [127], 'one short of the widest tile budget; c1 two tiles only'),
    _f('wide_hidden', 4, [128], 'MAXT / PT come from a hidden layer, tile_stride from c1 = 4 alone'),
    _f('wide_c1', 128, [2], 'the reverse: c1 fills MAXT 8, the hidden layer is one ragged tile', ld='+4'),
    _f('deep', 16, [16] * RANK_MAX_LAYERS, 'RANK_MAX_LAYERS MFMA layers plus the dot'),
    _f('in_none', 20, [24], 'in_act none: negative inputs reach the first product', in_act=None),
    _f('in_sigmoid', 20, [24], 'in_act sigmoid: padded lanes of the ragged k-step must stay 0, not 0.5', in_act='sigmoid', ld='+4'),
    _f('sig_hidden_ragged', 36, [17, 33], 'sigmoid hidden layers after ragged widths: 0.5 in padded tile rows must meet zero weights',
       acts=['sigmoid', 'sigmoid']),
    _f('sig_hidden_dot', 16, [3], 'a sigmoid layer right before the dot: 0.5 in padded rows must meet a zero dot weight', acts=['sigmoid'],
       dot_act=None),
    _f('mixed_acts', 32, [24, 40, 8], 'none / sigmoid / relu hidden layers in one stack', in_act=None, acts=[None, 'sigmoid', 'relu']),
    _f('dot_none', 32, [32], 'a linear dot: scores of both signs (threshold, -inf padding and the tie walk below zero)', dot_act=None),
    _f('dot_relu_zeros', 16, [16], 'a relu dot whose bias leaves 40 % of the pairs at exactly 0: a bulk tie', dot_act='relu',
       dot_bias=('zero_share', 0.4)),
    _f('dot_relu_wide', 100, [65], 'the same bulk tie on MAXT 8 with ragged widths', dot_act='relu', dot_bias=('zero_share', 0.4), ld='x2'),
]
FORM_NAMES = [f.name for f in FORMS]


def dims_of(form):
    return [form.c1] + form.hidden + [1]


def acts_of(form):
    return form.acts + [form.dot_act]


def build(form, n_items, n_users=N_USERS, dims=None, seed=None):
    """The head's weights and the two tables for `n_items` items: {'tu', 'ti', 'layers', 'dims', 'acts', 'in_act'} (float32).
    Items TIE_ROWS(n) share one vector when n > 4.  The weights depend on the form and the seed only (a 'zero_share' dot bias
    also on the tables it is measured on)."""
    dims = dims_of(form) if dims is None else list(dims)
    index = FORM_NAMES.index(form.name) if form.name in FORM_NAMES else len(FORM_NAMES)
    rng = np.random.default_rng(1000 + 97 * index + (form.seed if seed is None else seed))
    layers = [(rng.normal(0, 1 / np.sqrt(k), size=(k, n)).astype(np.float32), rng.uniform(-0.1, 0.1, size=n).astype(np.float32))
              for k, n in zip(dims[:-2], dims[1:-1])]
    layers.append((rng.normal(0, 4 / np.sqrt(dims[-2]), size=(dims[-2], 1)).astype(np.float32), rng.uniform(-0.1, 0.1, size=1).astype(np.float32)))
    rng_t = np.random.default_rng(rng.integers(1 << 30) + n_items)
    tu = rng_t.normal(0, 1, size=(n_users, dims[0])).astype(np.float32)
    ti = rng_t.normal(0, 1, size=(n_items, dims[0])).astype(np.float32)
    if n_items > 4:
        first, *rest = TIE_ROWS(n_items)
        for r in rest:
            ti[r] = ti[first]
    acts = acts_of(form)
    if form.dot_bias is not None:
        kind, share = form.dot_bias
        assert kind == 'zero_share'
        w, b = layers[-1]
        pre = pre_scores(tu, ti, layers[:-1] + [(w, np.zeros(1, dtype=np.float32))], acts, form.in_act, np.float64)
        # a bias in the widest gap of the pre-activations near the wanted quantile: no pair sits within rounding of zero
        v = np.unique(pre)
        at = int(np.clip(round(share * len(v)), 1, len(v) - 1))
        lo, hi = max(1, at - max(2, len(v) // 50)), min(len(v) - 1, at + max(2, len(v) // 50))
        cut = lo + int(np.argmax(np.diff(v[lo - 1:hi + 1])))
        layers[-1] = (w, np.array([-(v[cut - 1] + v[cut]) / 2.0], dtype=np.float32))
    return {'tu': tu, 'ti': ti, 'layers': layers, 'dims': dims, 'acts': acts, 'in_act': form.in_act}


def windowed(table, ld):
    """(wide float32 array filled with NaN, column offset): `table` sits in wide[:, off:off + c1]; wide has ld columns."""
    n, c1 = table.shape
    if ld == 'c1':
        return np.ascontiguousarray(table), 0
    cols, off = (c1 + 4, 4) if ld == '+4' else (2 * c1, 4)
    wide = np.full((n, cols), np.nan, dtype=np.float32)
    wide[:, off:off + c1] = table
    return wide, off


def item_counts(route):
    """The smallest catalogues that reach every path of a launch with this route: one item; one step and a ragged second one;
    one tile and a ragged second step of the second tile."""
    step = 16 * route['pt']
    return [1, step + 3, route['tile_items'] + step + 3]


# ---- the host route, restated (csrc/amar_rank_score.h: rank_pack_args, rank_shape, the LDS sums) ---------------------------------
EINVAL, EUNSUPPORTED = -1, -2
RANK_OF_MAX_TARGETS, RANK_UB, RANK_WAVES, TILE_BYTES = 64, 16, 4, 32 * 1024
SELECT_BYTES = 16640                          # sixteen selectors (amar_rank_select.h: two lists, two candidate buffers, four words)
LDS_LIMIT, LDS_PLAIN = 160 * 1024, 64 * 1024


def tiles16(n):
    return (n + 15) // 16


def route(kind, dims):
    """What amar_rank_route must answer for `dims`: (code, dict of its fields or None)."""
    n_layers = len(dims) - 1
    if kind not in ('recommend', 'group', 'rank_of'):
        return EINVAL, None
    if n_layers < 2 or n_layers > RANK_MAX_LAYERS + 1:
        return EUNSUPPORTED, None
    c1 = dims[0]
    if c1 < 4 or c1 % 4:
        return EINVAL, None
    if c1 > 128 or dims[-1] != 1:
        return EUNSUPPORTED, None
    floats = 0
    for l in range(n_layers):
        k, n = dims[l], dims[l + 1]
        if k < 1 or n < 1:
            return EINVAL, None
        if l == n_layers - 1:
            floats += 16 * tiles16(k) + 4
        else:
            if n == 1:
                return EUNSUPPORTED, None
            floats += tiles16(n) * tiles16(k) * 256 + 16 * tiles16(n)
    widest = max(dims[:-1])
    if widest > 128:
        return EUNSUPPORTED, None
    maxt = 1 if widest <= 16 else (2 if widest <= 32 else (4 if widest <= 64 else 8))
    pt = {1: 4, 2: 4, 4: 2, 8: 1}[maxt]
    stride = 16 * tiles16(c1) + 4
    step = 16 * pt
    tile_items = max(step, min(256, TILE_BYTES // (4 * stride)) // step * step)
    lds = ((floats + 3) & ~3) * 4 + tile_items * stride * 4
    lds += SELECT_BYTES if kind != 'rank_of' else RANK_WAVES * step * stride * 4 + RANK_UB * (6 * RANK_OF_MAX_TARGETS + 2) * 4
    return 0, {'maxt': maxt, 'pt': pt, 'tile_items': tile_items, 'tile_stride': stride, 'wpack_floats': floats, 'lds_bytes': lds,
               'fits': lds <= LDS_LIMIT, 'large_lds': lds > LDS_PLAIN}


def capacity_heads(fits):
    """(largest, past): the widest and deepest 128-wide head `fits(dims)` accepts, found by walking — 128 -> 128 -> ... while another
    128-wide layer fits, then the widest last hidden layer — and the first head past it (that last layer one unit wider)."""
    hidden = []
    while len(hidden) + 2 <= RANK_MAX_LAYERS and fits([128] + hidden + [128, 1]):
        hidden.append(128)                                           # [128] + hidden + [1] fits, one more 128-wide layer may not
    assert hidden and not fits([128] + hidden + [128, 1])
    widths = [w for w in range(2, 128) if fits([128] + hidden + [w, 1])]
    if not widths:
        return [128] + hidden + [1], [128] + hidden + [2, 1]
    return [128] + hidden + [widths[-1], 1], [128] + hidden + [widths[-1] + 1, 1]
