"""tests/entry_point_ref.py — the float64 reference of tests/test_entry_points_gpu.py — pinned to what the project already trusts: oracle.models /
oracle.layers / oracle.train, torch float64 autograd and the float32 Keras expression of test_training_kernels.  No GPU."""
import numpy as np
import pytest

from oracle import layers as ol
from oracle import models as om
from oracle import train as otrain
from oracle import weights as ow
from tests import entry_point_ref as ref


def _fold(head, ug, ig, ub, ib, feature_based):
    """The per-entity tables of the fused head: dense1* / dense2* applied, then the FIRST layer of dense3a / dense3b split into the halves
    of its concatenated input and applied per entity (x . W = u . W[:d] + i . W[d:]); the bias rides on the second table."""
    f = lambda t: np.asarray(t, dtype=np.float64)                                                         # noqa: E731
    net = lambda name, x: ol.dense_network(x, [(f(w), f(b)) for w, b in head[name]], 'relu')              # noqa: E731
    ug, ig, ub, ib = net('dense1a', ug), net('dense1b', ig), net('dense2a', ub), net('dense2b', ib)
    pairs = ((ug, ig), (ub, ib)) if feature_based else ((ug, ub), (ig, ib))
    A, B = [], []
    for (first, second), name in zip(pairs, ('dense3a', 'dense3b')):
        w, b = f(head[name][0][0]), f(head[name][0][1])
        d = first.shape[1]
        A.append(first @ w[:d])
        B.append(second @ w[d:] + b)
    return A, B


@pytest.mark.parametrize('feature_based', [True, False])
@pytest.mark.parametrize('n_branch,clf_units', [(0, [20]), (1, [32, 32]), (2, [32])])
def test_two_branch_head_is_the_hybrid_head_on_prefolded_tables(feature_based, n_branch, clf_units):
    rng = np.random.default_rng(3 + n_branch)
    D, nu, ni, P = 32, 50, 40, 333
    head = ow.hybrid_head(rng, 12, 20, ([16, 8], [24, 8], [D] * (n_branch + 1)), clf_units, bias_range=0.3)
    ug, ig = rng.standard_normal((nu, 12)), rng.standard_normal((ni, 12))
    ub, ib = rng.standard_normal((nu, 20)), rng.standard_normal((ni, 20))
    u, i = rng.integers(0, nu, P), rng.integers(0, ni, P)
    want = om.hybrid_cbrs(ug[u], ig[i], ub[u], ib[i], head, feature_based=feature_based)[:, 0]
    A, B = _fold(head, ug, ig, ub, ib, feature_based)
    rows_a, rows_b = ([u, u], [i, i]) if feature_based else ([u, i], [u, i])
    got, scale = ref.dual_head(A, B, rows_a, rows_b, [head['dense3a'][1:], head['dense3b'][1:]], head['clf'], 'relu', ['relu'] * n_branch,
                               ['relu'] * len(clf_units) + ['sigmoid'])
    assert np.abs(got - want).max() < 1e-12
    assert (scale > 0).all()


@pytest.mark.parametrize('D,W,n_branch,n_trunk,in_act,b_act', [(64, 64, 1, 3, 'relu', 'relu'), (16, 4, 1, 3, 'none', 'none'), (64, 4, 1, 2, 'relu', 'none'),
                                                               (48, 20, 2, 3, 'none', 'relu'), (32, 48, 0, 2, 'sigmoid', 'relu'), (16, 20, 1, 3, 'none', 'none')])
def test_float32_numpy_head_meets_the_bounds_the_kernels_are_held_to(D, W, n_branch, n_trunk, in_act, b_act):
    """The bounds of the GPU tests are satisfiable by a float32 evaluation: numpy float32 against float64 stays within 5e-6 of an element's own
    scale on a linear output (measured 8e-8 .. 2.3e-6, the largest on the all-linear 4-wide trunk, which has the two-layer scale) and within 1e-6 absolute on sigmoid scores
    (measured 3e-7)."""
    h = ref.draw_dual_head(np.random.default_rng(D + W), D, W, n_branch, n_trunk, 3000)
    rows = [np.random.default_rng(6 + k).integers(0, 3000, 100_000) for k in range(4)]
    for last in ('none', 'sigmoid'):
        args = (h['A'], h['B'], rows[:2], rows[2:], h['branch'], h['trunk'], in_act, [b_act] * n_branch, ['relu'] * (n_trunk - 1) + [last])
        want, scale = ref.dual_head(*args)
        got = ref.dual_head_f32(*args)
        if last == 'none':
            assert ref.scaled_error(got, want, scale) < 5e-6
            assert np.median(scale / np.maximum(np.abs(want), 1e-3)) < (300 if W < ref.NARROW_TRUNK else 30)   # the element's own size, not the array's
        else:
            assert np.abs(got - want).max() < 1e-6
            assert W < 64 or (want.min() < 0.3 and want.max() > 0.7)                       # the common head's scores spread over (0, 1)


def test_attention_mix_is_the_oracles_two_way_softmax():
    rng = np.random.default_rng(1)
    M, D = 200, 24
    a, b = rng.standard_normal((M, D)), rng.standard_normal((M, D))
    fw = {'att_weight': rng.standard_normal((D, D)) * 1.5}
    ta, tb = a @ fw['att_weight'], b @ fw['att_weight']
    assert np.abs(ta).max() > 8                                                             # saturated tanh among them
    assert np.abs(ref.attention_mix(a, b, ta, tb) - om.attention_fuse(a, b, fw)).max() < 1e-13
    # wa = sigmoid(tanh ta - tanh tb) against the explicit softmax over the two stacked sources
    att = np.exp(np.tanh(np.stack([ta, tb], axis=1)))
    assert np.abs(ref.attention_weight(ta, tb) - (att / att.sum(axis=1, keepdims=True))[:, 0]).max() < 1e-15


def test_attention_mix_reverse_is_autograd():
    import torch
    rng = np.random.default_rng(2)
    dout, a, b, ta, tb = (np.asarray(t, dtype=np.float64) for t in ref.draw_attention_inputs(rng, 300, 7))
    ts = [torch.tensor(t, requires_grad=True) for t in (a, b, ta, tb)]
    att = torch.softmax(torch.tanh(torch.stack([ts[2], ts[3]], dim=1)), dim=1)
    out = (att * torch.stack([ts[0], ts[1]], dim=1)).sum(dim=1)
    assert np.abs(out.detach().numpy() - ref.attention_mix(a, b, ta, tb)).max() < 1e-14
    out.backward(torch.tensor(dout))
    got = ref.attention_mix_bwd(dout, a, b, ta, tb)
    for g, t in zip(got, ts):
        assert np.abs(g - t.grad.numpy()).max() < 1e-14
    assert np.abs(got[0] + got[1] - dout).max() < 1e-15


def test_locality_scale_is_dgcf_convs_scaling_step_and_autograd():
    import torch
    from scipy import sparse
    rng = np.random.default_rng(3)
    dout, x, w = (np.asarray(t, dtype=np.float64) for t in ref.draw_locality_inputs(rng, 150, 9))
    eye = sparse.identity(150, format='csr')
    assert np.abs(ref.locality_scale(x, w) - ol.dgcf_conv(x, eye, w[:, None])).max() < 1e-15
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    (xt * torch.sigmoid(wt)[:, None]).backward(torch.tensor(dout))
    dx, dw = ref.locality_scale_bwd(dout, x, w)
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-15 and np.abs(dw - wt.grad.numpy()).max() < 1e-14
    assert dw[0] < 1e-40 and np.isfinite(dw).all()                                          # w = +-100: sigmoid' = 0


@pytest.mark.parametrize('name', ['none', 'relu', 'sigmoid'])
def test_add3_act_is_the_oracles_activation_of_the_sum(name):
    a, b, c = (np.asarray(t, dtype=np.float64) for t in ref.draw_add3_inputs(np.random.default_rng(4), 50, 5, name))
    with np.errstate(over='ignore'):
        want = ol._act(a + b + c, None if name == 'none' else name)
    assert np.array_equal(ref.add3_act(a, b, c, name), want)


def test_float32_numpy_figures_behind_the_kernel_bounds():
    """The kernels are held to KERNEL_FACTOR times ref.f32_numpy_figures(): what a numpy float32 evaluation of the same formulas leaves on
    the planted inputs.  ref.F32_NUMPY_FIGURES is the record of that measurement quoted in the GPU tests' docstrings."""
    measured = ref.f32_numpy_figures()
    assert set(measured) == set(ref.F32_NUMPY_FIGURES)
    for key, value in measured.items():
        print(key, value)
        assert abs(value - ref.F32_NUMPY_FIGURES[key]) <= 0.05 * value, (key, value)
        assert value < 8 * ref.F32_EPS                                                      # a few float32 roundings
    dout, a, b, ta, tb = ref.draw_attention_inputs(np.random.default_rng(1), 300, 8)
    assert np.abs(ref.attention_mix_t(a, b, ta, tb) - ref.attention_mix(*(t.astype(np.float64) for t in (a, b, ta, tb)))).max() < 1e-5


def test_adam_scales_are_the_term_magnitudes():
    rng = np.random.default_rng(8)
    w, m = rng.standard_normal(50), rng.standard_normal(50)
    v, parts = rng.uniform(0, 1, 50), rng.standard_normal((3, 50))
    sw, sm, sv = ref.adam_scales(w, parts, m, v, 1e-3, 0.9, 0.999, 1e-7, 0.0)
    got = ref.adam_step(w, parts.sum(0), m, v, 1e-3, 0.9, 0.999, 1e-7)
    assert (sm >= np.abs(got[1])).all() and (sv >= got[2]).all() and (sw >= np.abs(w)).all()
    assert np.allclose(sm, 0.9 * np.abs(m) + 0.1 * np.abs(parts).sum(0))


def test_adam_step_is_the_oracles_update():
    rng = np.random.default_rng(5)
    w, g, m = (rng.standard_normal(500) for _ in range(3))
    v = rng.uniform(0, 1, 500)
    for t in (1, 3, 10000):
        lr_t = ref.adam_lr_t(t, 1e-3, 0.9, 0.999)
        assert lr_t == 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for l2 in (0.0, 1e-3):
            got = ref.adam_step(w, g, m, v, lr_t, 0.9, 0.999, 1e-7, l2)
            want = otrain.adam_update(w, g + 2 * l2 * w, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7)
            for a, b in zip(got, want):
                assert np.abs(a - b).max() < 1e-15
    zero = ref.adam_step(np.ones(3), np.zeros(3), np.zeros(3), np.zeros(3), 1e-3, 0.9, 0.999, 1e-7)
    assert np.array_equal(zero[0], np.ones(3))                                              # v = 0, g = 0: the epsilon guards the division


def test_partial_gradients_are_added_in_group_order():
    parts = np.random.default_rng(6).standard_normal((17, 300)).astype(np.float32) * np.float32(1e3)
    seq = parts[0].copy()
    for k in range(1, 17):
        seq += parts[k]
    assert np.array_equal(ref.sum_groups_f32(parts), seq) and ref.sum_groups_f32(parts).dtype == np.float32


def test_bce_terms_are_the_float32_keras_expression():
    rng = np.random.default_rng(7)
    p = rng.uniform(0, 1, 500).astype(np.float32); p[:3] = [0.0, 1.0, 5e-8]
    lab = rng.integers(0, 2, 500).astype(np.float32)
    # the expression of tests/test_training_gpu.py::test_training_kernels, written out
    e32, one = np.float32(1e-7), np.float32(1)
    pc = np.clip(p, e32, one - e32)
    want_terms = -(lab * np.log(pc + e32) + (one - lab) * np.log(one - pc + e32))
    inside = (p >= e32) & (p <= one - e32)
    want_dz = -(lab / (pc + e32) - (one - lab) / (one - pc + e32)) / np.float32(500) * inside * p * (one - p)
    terms, dz = ref.bce_terms_f32(p, lab)
    assert np.array_equal(terms, want_terms) and np.array_equal(dz, want_dz) and terms.dtype == np.float32
    assert abs(terms.astype(np.float64).mean() - ref.bce_mean_loss(p, lab)) < 1e-6 * ref.bce_mean_loss(p, lab)
    # and the float64 mean is the oracle's loss expression away from the clip points (float32 puts the upper one at 1 - 1.19e-7)
    pd, yd = p[3:].astype(np.float64), lab[3:].astype(np.float64)
    pcd = np.clip(pd, otrain.EPS, 1 - otrain.EPS)
    oracle = -np.mean(yd * np.log(pcd + otrain.EPS) + (1 - yd) * np.log(1 - pcd + otrain.EPS))
    assert abs(oracle - ref.bce_mean_loss(p[3:], lab[3:])) < 1e-9
    lo, mid, hi = ref.ulp_neighbours(1e-7)
    assert lo < mid < hi and mid == np.float32(1e-7)
