"""float64 numpy restatement of the optimizer rules of include/amar_hip.h (SGD, RMSprop, Adagrad, Adamax, Nadam, AMSGrad), written from the
header's formulas; no torch, no device.  tests/test_optimizers_cpu.py pins it against torch.optim where the two are algebraically identical
and against hand-computed steps elsewhere.

`Optimizer` is stateful over steps (the step count, Nadam's running product, one list of state arrays per parameter key); `scalars`,
`step` and `scales` are its stateless parts, which the kernel tests call directly."""
import numpy as np

DEFAULTS = {
    'SGD': dict(learning_rate=0.01, momentum=0.0, nesterov=False),
    'RMSprop': dict(learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False),
    'Adagrad': dict(learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7),
    'Adamax': dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7),
    'Nadam': dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7),
    'AMSGrad': dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7),
}


def hyper_of(rule, **hyper):
    """Keras' constructor defaults of `rule` overridden by `hyper`, as Python floats / bools."""
    h = dict(DEFAULTS[rule])
    assert set(hyper) <= set(h), set(hyper) - set(h)
    h.update(hyper)
    return {k: (bool(v) if isinstance(DEFAULTS[rule][k], bool) else float(v)) for k, v in h.items()}


def as_float32(h):
    """The hyper-parameters as the kernels receive them: rounded to float32 (then computed with in float64)."""
    return {k: (v if isinstance(v, bool) else float(np.float32(v))) for k, v in h.items()}


def state_names(rule, h):
    """The state arrays of a parameter, in the header's order s0, s1, s2."""
    if rule == 'SGD':
        return ['a'] if h['momentum'] > 0 else []
    if rule == 'RMSprop':
        return ['rms'] + (['mg'] if h['centered'] else []) + (['mom'] if h['momentum'] > 0 else [])
    return {'Adagrad': ['acc'], 'Adamax': ['m', 'u'], 'Nadam': ['m', 'v'], 'AMSGrad': ['m', 'v', 'vhat']}[rule]


def initial_arrays(rule, h, like):
    fill = h.get('initial_accumulator_value', 0.0)
    return [np.full(np.shape(like), fill, dtype=np.float64) for _ in state_names(rule, h)]


def scalars(rule, h, t, p_prev=1.0):
    """The step-dependent scalars of step t (t = 1 for the first step).  Nadam: p_prev = P_{t-1} (P_0 = 1); the result's 'P' is P_t."""
    lr = h['learning_rate']
    if rule == 'Adamax':
        return {'step': lr / (1.0 - h['beta_1'] ** t)}
    if rule == 'AMSGrad':
        return {'step': lr * np.sqrt(1.0 - h['beta_2'] ** t) / (1.0 - h['beta_1'] ** t)}
    if rule == 'Nadam':
        mu = h['beta_1'] * (1.0 - 0.5 * 0.96 ** (0.004 * t))
        mu_next = h['beta_1'] * (1.0 - 0.5 * 0.96 ** (0.004 * (t + 1)))
        return {'step': lr, 'mu': mu, 'mu_next': mu_next, 'P': p_prev * mu, 'omb2': 1.0 - h['beta_2'] ** t}
    return {'step': lr}


def step(rule, h, sc, w, g, arrays, l2=0.0):
    """(w, [state arrays]) after one update of the header's rule; sc = scalars(rule, h, t, ...)."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s = [np.asarray(a, dtype=np.float64) for a in arrays]
    g = g + 2.0 * l2 * w
    lr = sc['step']
    if rule == 'SGD':
        if h['momentum'] == 0:
            return w - lr * g, []
        a = h['momentum'] * s[0] - lr * g
        return (w + h['momentum'] * a - lr * g, [a]) if h['nesterov'] else (w + a, [a])
    if rule == 'RMSprop':
        rho, eps = h['rho'], h['epsilon']
        rms = rho * s[0] + (1.0 - rho) * g * g
        out, d = [rms], rms
        if h['centered']:
            mg = rho * s[1] + (1.0 - rho) * g
            out.append(mg)
            d = np.maximum(rms - mg * mg, 0.0)
        if h['momentum'] == 0:
            return w - lr * g / (np.sqrt(d) + eps), out
        mom = h['momentum'] * s[-1] + lr * g / np.sqrt(d + eps)
        return w - mom, out + [mom]
    if rule == 'Adagrad':
        acc = s[0] + g * g
        return w - lr * g / (np.sqrt(acc) + h['epsilon']), [acc]
    b1, b2, eps = h['beta_1'], h['beta_2'], h['epsilon']
    m = b1 * s[0] + (1.0 - b1) * g
    if rule == 'Adamax':
        u = np.maximum(b2 * s[1], np.abs(g))
        return w - lr * m / (u + eps), [m, u]
    v = b2 * s[1] + (1.0 - b2) * g * g
    if rule == 'Nadam':
        g_hat = g / (1.0 - sc['P'])
        m_hat = m / (1.0 - sc['P'] * sc['mu_next'])
        v_hat = v / sc['omb2']
        return w - h['learning_rate'] * ((1.0 - sc['mu']) * g_hat + sc['mu_next'] * m_hat) / (np.sqrt(v_hat) + eps), [m, v]
    assert rule == 'AMSGrad', rule
    vhat = np.maximum(s[2], v)
    return w - lr * m / (np.sqrt(vhat) + eps), [m, v, vhat]


def scales(rule, h, sc, w, parts, arrays, l2=0.0):
    """Per-element scales (w, [state arrays]) of one step whose gradient is the sum of `parts` [G, n]: every state array against the sum of
    the magnitudes of its terms (a maximum: against the larger magnitude), the weight against the update those magnitudes would give over
    the TRUE denominator, plus |w| (the stored result carries its rounding) — entry_point_ref.adam_scales for the other rules.  Centered
    RMSprop's denominator is a difference, rms - mg^2: the update's scale grows by (rms_s + mg_s^2) / (rms - mg^2), the factor by which
    the difference amplifies the relative error of its terms."""
    w64 = np.asarray(w, dtype=np.float64)
    parts = np.asarray(parts, dtype=np.float64).reshape(-1, w64.size)
    s = [np.abs(np.asarray(a, dtype=np.float64)) for a in arrays]
    gs = np.abs(parts).sum(0) + 2.0 * l2 * np.abs(w64)
    _, true = step(rule, h, sc, w64, parts.sum(0), arrays, l2)
    lr, aw = sc['step'], np.abs(w64)
    if rule == 'SGD':
        if h['momentum'] == 0:
            return aw + lr * gs, []
        a_s = h['momentum'] * s[0] + lr * gs
        return aw + (h['momentum'] * a_s + lr * gs if h['nesterov'] else a_s), [a_s]
    if rule == 'RMSprop':
        rho, eps = h['rho'], h['epsilon']
        rms_s = rho * s[0] + (1.0 - rho) * gs * gs
        out, d, amp = [rms_s], true[0], 1.0
        if h['centered']:
            mg_s = rho * s[1] + (1.0 - rho) * gs
            out.append(mg_s)
            d = np.maximum(true[0] - true[1] ** 2, 0.0)
            amp = np.maximum((rms_s + mg_s ** 2) / np.maximum(d, 1e-300), 1.0)
        if h['momentum'] == 0:
            return aw + amp * lr * gs / (np.sqrt(d) + eps), out
        mom_s = h['momentum'] * s[-1] + amp * lr * gs / np.sqrt(d + eps)
        return aw + mom_s, out + [mom_s]
    if rule == 'Adagrad':
        return aw + lr * gs / (np.sqrt(true[0]) + h['epsilon']), [s[0] + gs * gs]
    b1, b2, eps = h['beta_1'], h['beta_2'], h['epsilon']
    m_s = b1 * s[0] + (1.0 - b1) * gs
    if rule == 'Adamax':
        return aw + lr * m_s / (true[1] + eps), [m_s, np.maximum(b2 * s[1], gs)]
    v_s = b2 * s[1] + (1.0 - b2) * gs * gs
    if rule == 'Nadam':
        num = h['learning_rate'] * ((1.0 - sc['mu']) * gs / (1.0 - sc['P']) + sc['mu_next'] * m_s / (1.0 - sc['P'] * sc['mu_next']))
        return aw + num / (np.sqrt(true[1] / sc['omb2']) + eps), [m_s, v_s]
    return aw + lr * m_s / (np.sqrt(true[2]) + eps), [m_s, v_s, np.maximum(s[2], v_s)]


class Optimizer:
    """One rule over steps: `advance()` once per step, then `update(key, w, g)` for every parameter of that step."""

    def __init__(self, rule, **hyper):
        self.rule, self.h = rule, hyper_of(rule, **hyper)
        self.t, self.p, self.state, self.sc = 0, 1.0, {}, None

    def advance(self):
        self.t += 1
        self.sc = scalars(self.rule, self.h, self.t, self.p)
        self.p = self.sc.get('P', 1.0)

    def update(self, key, w, g, l2=0.0):
        arrays = self.state.get(key)
        if arrays is None:
            arrays = initial_arrays(self.rule, self.h, w)
        w, self.state[key] = step(self.rule, self.h, self.sc, w, g, arrays, l2)
        return w
