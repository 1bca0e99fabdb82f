"""float64 numpy restatement of the gradient clips of include/amar_hip.h (clipvalue, clipnorm, global_clipnorm: Keras 2's OptimizerV2),
written from the header's formulas; no torch, no device.  tests/test_grad_clip_cpu.py pins it against hand-computed cases.

A slot is (w, parts [G, n], l2): its finished gradient is parts.sum(0) + 2 l2 w.  `clip` is the rule, `bounds` what float32 may do to it,
`Optimizer` is optimizer_ref.Optimizer with the clip in front of the update.

The error bounds (`bounds`), derived here and not from any output of the kernels.  u = 2^-24 is float32's unit roundoff.
  * gi: G - 1 float32 additions and one fused multiply-add, max(G, 1) roundings in all, each relative to a partial result that the sum of
    the magnitudes gs = sum |parts| + 2 l2 |w| bounds:  e_g = max(G, 1) u gs  (optimizer_ref.scales' gs, with the count written out).
  * clipvalue: the clamp is exact and 1-Lipschitz:  e = e_g.
  * a norm: the float32 sum of n squares, in any order and fused or not, is within n u of its exact value relatively (every term passes
    through at most n roundings), the root halves that and adds one rounding, and the errors of the gi move the norm by at most their
    own 2-norm:  e_norm = ||e_g||_2 + norm (n u / 2 + u).  n is the slot's size (clipnorm) or the size of all slots (global_clipnorm).
  * the scale s = c / max(norm, c): where norm + e_norm <= c both sides have s = 1 exactly and e_s = 0; else its relative error is that of
    the norm plus the division's rounding, e_s = e_norm / norm + u (this also covers a kernel that finds norm <= c, s = 1, where the
    exact norm is just above c: then 1 - s <= e_norm / norm).
  * the product gi s, one more rounding:  e = s e_g + |gi| s (e_s + u); where e_s = 0 the product is by 1 and exact:  e = e_g.
Every bound is multiplied by 1.01 for the second-order terms."""
import numpy as np

from tests import optimizer_ref as oref

MODES = ('clipvalue', 'clipnorm', 'global_clipnorm')
U = 2.0 ** -24
SLACK = 1.01


def finished(w, parts, l2=0.0):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    return np.asarray(parts, dtype=np.float64).reshape(-1, w.size).sum(0) + 2.0 * l2 * w


def _finished_all(slots):
    return [finished(w, parts, l2) for w, parts, l2 in slots]


def norms(mode, slots):
    """The measured norms: one per slot (clipnorm), one in all (global_clipnorm)."""
    sq = np.array([float(np.sum(g * g)) for g in _finished_all(slots)])
    return np.sqrt(sq) if mode == 'clipnorm' else np.sqrt(np.array([sq.sum()]))


def max_abs(slots):
    return max(float(np.abs(g).max()) for g in _finished_all(slots))


def _scales(mode, c, slots):
    nrm = norms(mode, slots)
    s = c / np.maximum(nrm, c)
    return (s if mode == 'clipnorm' else np.repeat(s, len(slots))), nrm


def clip(mode, c, slots):
    """([clipped finished gradient of every slot], measured norms or None)."""
    assert mode in MODES and c > 0
    gs = _finished_all(slots)
    if mode == 'clipvalue':
        return [np.minimum(np.maximum(g, -c), c) for g in gs], None
    s, nrm = _scales(mode, c, slots)
    return [g * sk for g, sk in zip(gs, s)], nrm


def bounds(mode, c, slots):
    """([per-element absolute error bound of every slot's clipped gradient], absolute error bounds of the norms or None): the module's
    docstring derives them."""
    gs = _finished_all(slots)
    e_g = []
    for w, parts, l2 in slots:
        w = np.abs(np.asarray(w, dtype=np.float64).reshape(-1))
        parts = np.abs(np.asarray(parts, dtype=np.float64).reshape(-1, w.size))
        e_g.append(max(parts.shape[0], 1) * U * (parts.sum(0) + 2.0 * l2 * w))
    if mode == 'clipvalue':
        return [SLACK * e for e in e_g], None
    s, nrm = _scales(mode, c, slots)
    if mode == 'clipnorm':
        n_terms = np.array([g.size for g in gs], dtype=np.float64)
        e_2 = np.array([np.sqrt(np.sum(e * e)) for e in e_g])
    else:
        n_terms = np.array([float(sum(g.size for g in gs))])
        e_2 = np.array([np.sqrt(sum(float(np.sum(e * e)) for e in e_g))])
    e_norm = e_2 + nrm * (n_terms * U / 2.0 + U)
    e_s = np.where(nrm + SLACK * e_norm <= c, 0.0, e_norm / np.where(nrm > 0, nrm, 1.0) + U)
    if mode == 'global_clipnorm':
        e_s = np.repeat(e_s, len(slots))
    out = [SLACK * (sk * e + np.abs(g) * sk * (es + U if es > 0 else 0.0)) for g, e, sk, es in zip(gs, e_g, s, e_s)]
    return out, SLACK * e_norm


class Optimizer(oref.Optimizer):
    """optimizer_ref.Optimizer with a gradient clip: `update_all` clips the gradients of ALL parameters of a step (global_clipnorm needs
    them together), then updates each.  The gradients are finished ones (the L2 part already in them), so the update runs with l2 = 0."""

    def __init__(self, rule, clip=None, **hyper):
        super().__init__(rule, **hyper)
        self.clip = clip                                             # None or (mode, c)

    def update_all(self, params):
        """params: {key: (w, g)} -> {key: new w}"""
        keys = list(params)
        grads = [np.asarray(params[k][1], dtype=np.float64) for k in keys]
        if self.clip is not None:
            flat, _ = clip(self.clip[0], self.clip[1], [(np.zeros(g.size), g.reshape(1, -1), 0.0) for g in grads])
            grads = [f.reshape(g.shape) for f, g in zip(flat, grads)]
        return {k: self.update(k, params[k][0], g) for k, g in zip(keys, grads)}
