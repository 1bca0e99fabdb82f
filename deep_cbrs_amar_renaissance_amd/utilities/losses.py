"""Losses named by `parameters.loss` in the configs (`/root/reference/src/utilities/losses.py:5-25`).

The experiment looks a name up here first (``hasattr(losses, name)`` -> an instance, `experiment.py:155-157` of the reference);
any other value — a Keras loss name, a Keras class name, or a mapping ``{name: ..., <hyper-parameters>}`` — goes through
`resolve_loss`, which names the pointwise losses the device computes (include/amar_hip.h: amar_loss_grad_f32) and refuses every other
name: ``binary_crossentropy`` is the default.  ``fit()`` and ``evaluate()`` read the compiled loss through `resolve_loss`
(`loss_kind` tells BPR from the pointwise losses).  `loss_terms` / `loss_dp` restate every pointwise loss in float64 numpy, with
the weights of ``fit(class_weight=...)`` and of a weighted Sequence where given (`pair_weights`, `resolve_class_weight`).

Beside BPRLoss stand three listwise losses on the groups the triplet sampler draws (one positive and ``n_negatives`` negatives of one
user): SampledSoftmaxLoss, HardestNegativeBPRLoss, MarginRankingLoss (include/amar_hip.h: amar_group_loss_grad_f32).  They route
wherever BPR routes (`loss_kind` says 'bpr'); `group_loss_terms` / `group_loss_dp` restate them in float64 numpy.
"""
from collections.abc import Mapping


import numpy as np


class BPRLoss:
    """Bayesian Personalized Ranking on the model's sigmoid outputs: the batch holds the observed items' scores in its first half
    and the sampled negatives' in its second.  An odd batch drops its last element; with h = B // 2,
    ``loss = -mean_j log sigmoid(p[j] - p[h + j])``, j < h (on probabilities, not logits).  Keras adds the L2 losses."""

    def __init__(self, name="BPR_loss"):
        self.name = name

    def __call__(self, y_true, y_pred):
        """float64 value of the loss for one batch (y_true is not read).  A batch without a pair (B < 2) counts 0."""
        p = np.asarray(y_pred, dtype=np.float64).reshape(-1)
        h = len(p) // 2
        if h == 0:
            return 0.0
        x = p[:h] - p[h:2 * h]
        return float(np.mean(np.logaddexp(0.0, -x)))          # -log sigmoid(x)


class _GroupLoss:
    """A listwise loss on the groups of data/datasets.py:UserItemGraphTriplets, on the model's sigmoid outputs as BPRLoss: a batch of
    B = 2h rows (an odd B drops its last) holds G = h / n_negatives groups; group g has the positive ``p[g K]`` and the negatives
    ``p[h + g K + k]``, k < K = n_negatives (rows g K + 1 .. g K + K - 1 repeat the positive's pair and carry nothing).  The batch
    loss is the mean of the group losses (include/amar_hip.h: amar_group_loss_grad_f32)."""
    code, hyper_name = None, None

    def hyper(self):
        """The kernel's four floats: (temperature | margin, 0, 0, 0)."""
        return (float(getattr(self, self.hyper_name)) if self.hyper_name else 0.0, 0.0, 0.0, 0.0)

    def __call__(self, y_true, y_pred, n_negatives=1):
        """float64 value of the loss for one batch (y_true is not read).  A batch without a pair (B < 2) counts 0."""
        p = np.asarray(y_pred, dtype=np.float64).reshape(-1)
        return float(np.sum(group_loss_terms(self.code, self.hyper(), p, n_negatives)) / len(p)) if len(p) else 0.0


class SampledSoftmaxLoss(_GroupLoss):
    """Sampled softmax over one positive and K negatives: ``l_g = -p+/t + log(exp(p+/t) + sum_k exp(p-_k/t))``, temperature t > 0,
    evaluated with the group's maximum subtracted.  K = 1, t = 1 is BPRLoss's value."""
    code, hyper_name = -2, 'temperature'

    def __init__(self, temperature=1.0, name="sampled_softmax_loss"):
        self.temperature, self.name = _positive(temperature, 'temperature', strict=True), name


class HardestNegativeBPRLoss(_GroupLoss):
    """BPR against the hardest of K sampled negatives (dynamic negative sampling): ``l_g = -log sigmoid(p+ - max_k p-_k)``; the
    negative side's gradient goes to the lowest k that attains the maximum."""
    code = -3

    def __init__(self, name="hardest_negative_BPR_loss"):
        self.name = name


class MarginRankingLoss(_GroupLoss):
    """Margin ranking hinge: ``l_g = (1 / K) sum_k max(0, m - p+ + p-_k)``, margin m >= 0; the subgradient is 0 where the hinge
    argument is not strictly positive."""
    code, hyper_name = -4, 'margin'

    def __init__(self, margin=0.5, name="margin_ranking_loss"):
        self.margin, self.name = _positive(margin, 'margin', strict=False), name


def _positive(value, what, strict):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("{} must be a number (got {!r})".format(what, value))
    if isinstance(value, bool) or not np.isfinite(v) or v < 0.0 or (strict and v == 0.0):
        raise ValueError("{} must be finite and {} (got {!r})".format(what, 'positive' if strict else 'not negative', value))
    return v


def loss_kind(loss):
    """'bpr' for a BPRLoss (instance or name) and for the listwise losses on its batches (SampledSoftmaxLoss, HardestNegativeBPRLoss,
    MarginRankingLoss: instance, name or mapping), 'bce' for anything else (the reference's default binary cross-entropy)."""
    if isinstance(loss, (BPRLoss, _GroupLoss)) or loss == 'BPRLoss':
        return 'bpr'
    if isinstance(loss, Mapping):
        loss = loss.get('name', loss.get('class_name'))
    if isinstance(loss, str) and loss in _GROUP_CLASSES:
        return 'bpr'
    return 'bce'


# ---- Keras 2's pointwise losses on one sigmoid output (include/amar_hip.h: AMAR_LOSS_*) ---------------------------------------------
BCE, MSE, MAE, HINGE, SQUARED_HINGE, HUBER, LOG_COSH, POISSON, FOCAL = range(9)
BPR = -1                                                              # (no code of amar_loss_grad_f32: amar_bpr_grad_f32's loss)
# the listwise losses on BPR's batches, and their kinds in amar_group_loss_grad_f32 (include/amar_hip.h: AMAR_GROUP_*)
SAMPLED_SOFTMAX, HARDEST_NEGATIVE, MARGIN_RANKING = SampledSoftmaxLoss.code, HardestNegativeBPRLoss.code, MarginRankingLoss.code
GROUP_KINDS = {SAMPLED_SOFTMAX: 0, HARDEST_NEGATIVE: 1, MARGIN_RANKING: 2}
_GROUP_CLASSES = {'SampledSoftmaxLoss': SampledSoftmaxLoss, 'HardestNegativeBPRLoss': HardestNegativeBPRLoss,
                  'MarginRankingLoss': MarginRankingLoss}

LOSS_NAMES = {BCE: 'binary_crossentropy', MSE: 'mean_squared_error', MAE: 'mean_absolute_error', HINGE: 'hinge',
              SQUARED_HINGE: 'squared_hinge', HUBER: 'huber', LOG_COSH: 'log_cosh', POISSON: 'poisson',
              FOCAL: 'binary_focal_crossentropy', BPR: 'BPRLoss', SAMPLED_SOFTMAX: 'SampledSoftmaxLoss',
              HARDEST_NEGATIVE: 'HardestNegativeBPRLoss', MARGIN_RANKING: 'MarginRankingLoss'}
_ALIASES = {
    'binary_crossentropy': BCE, 'BinaryCrossentropy': BCE,
    'mean_squared_error': MSE, 'mse': MSE, 'MSE': MSE, 'MeanSquaredError': MSE,
    'mean_absolute_error': MAE, 'mae': MAE, 'MAE': MAE, 'MeanAbsoluteError': MAE,
    'hinge': HINGE, 'Hinge': HINGE,
    'squared_hinge': SQUARED_HINGE, 'SquaredHinge': SQUARED_HINGE,
    'huber': HUBER, 'huber_loss': HUBER, 'Huber': HUBER,
    'log_cosh': LOG_COSH, 'logcosh': LOG_COSH, 'LogCosh': LOG_COSH,
    'poisson': POISSON, 'Poisson': POISSON,
    'binary_focal_crossentropy': FOCAL, 'BinaryFocalCrossentropy': FOCAL,
    'BPRLoss': BPR,
    'SampledSoftmaxLoss': SAMPLED_SOFTMAX, 'HardestNegativeBPRLoss': HARDEST_NEGATIVE, 'MarginRankingLoss': MARGIN_RANKING,
}
# what tf.keras.losses.get resolves and no kernel here computes (multi-class, distribution and similarity losses)
_KERAS_WITHOUT_KERNEL = {
    'categorical_crossentropy', 'CategoricalCrossentropy', 'sparse_categorical_crossentropy', 'SparseCategoricalCrossentropy',
    'categorical_hinge', 'CategoricalHinge', 'kl_divergence', 'kld', 'KLD', 'kullback_leibler_divergence', 'KLDivergence',
    'cosine_similarity', 'CosineSimilarity', 'mean_absolute_percentage_error', 'mape', 'MAPE', 'MeanAbsolutePercentageError',
    'mean_squared_logarithmic_error', 'msle', 'MSLE', 'MeanSquaredLogarithmicError',
}
# hyper-parameters a mapping may carry, with Keras' defaults; the kernel's array is (label_smoothing, delta | gamma, alpha, balancing)
_HYPER_DEFAULTS = {BCE: {'label_smoothing': 0.0}, HUBER: {'delta': 1.0},
                   FOCAL: {'gamma': 2.0, 'apply_class_balancing': False, 'alpha': 0.25, 'label_smoothing': 0.0},
                   SAMPLED_SOFTMAX: {'temperature': 1.0}, MARGIN_RANKING: {'margin': 0.5}}


def supported_losses():
    """Every name `resolve_loss` accepts, sorted."""
    return sorted(_ALIASES)


def resolve_loss(loss):
    """(code, hyper, name) of a compiled loss: `code` one of the AMAR_LOSS_* codes (or BPR), `hyper` the kernel's four floats
    (label_smoothing, delta or gamma, alpha, apply_class_balancing as 0 / 1) as a tuple, `name` Keras' function name.
    Accepts None (binary cross-entropy), a Keras loss or class name, a BPRLoss, or a mapping {name: ..., <hyper-parameters>}.
    The listwise losses (instance, class name, or a mapping such as {name: SampledSoftmaxLoss, temperature: 0.2}) have the codes
    SAMPLED_SOFTMAX / HARDEST_NEGATIVE / MARGIN_RANKING and hyper = (temperature | margin, 0, 0, 0).
    NotImplementedError: a loss Keras knows and no kernel here computes; ValueError: any other name or hyper-parameter."""
    values = {}
    if isinstance(loss, BPRLoss):
        return BPR, (0.0, 0.0, 0.0, 0.0), LOSS_NAMES[BPR]
    if isinstance(loss, _GroupLoss):
        if loss.hyper_name:                                          # (an attribute set after the constructor is checked again)
            _positive(getattr(loss, loss.hyper_name), loss.hyper_name, strict=loss.code == SAMPLED_SOFTMAX)
        return loss.code, loss.hyper(), LOSS_NAMES[loss.code]
    if isinstance(loss, Mapping):
        values = {k: v for k, v in loss.items() if k not in ('name', 'class_name')}
        loss = loss.get('name', loss.get('class_name'))
    if loss is None:
        loss = 'binary_crossentropy'
    if not isinstance(loss, str):
        raise ValueError("loss must be a name, a mapping with a name, a BPRLoss or None (got {!r})".format(loss))
    if loss not in _ALIASES:
        if loss in _KERAS_WITHOUT_KERNEL:
            raise NotImplementedError("loss '{}' has no kernel here; supported: {}".format(loss, ', '.join(supported_losses())))
        raise ValueError("unknown loss '{}'; supported: {}".format(loss, ', '.join(supported_losses())))
    code = _ALIASES[loss]
    known = dict(_HYPER_DEFAULTS.get(code, {}))
    unknown = sorted(set(values) - set(known))
    if unknown:
        raise ValueError("loss '{}' takes no hyper-parameter {} (it takes: {})".format(loss, unknown, sorted(known) or 'none'))
    known.update(values)
    if code in GROUP_KINDS:                                          # (the classes check the temperature and the margin)
        return code, _GROUP_CLASSES[loss](**known).hyper(), LOSS_NAMES[code]
    ls = float(known.get('label_smoothing', 0.0))
    shape = float(known.get('delta', known.get('gamma', 0.0)))
    if not 0.0 <= ls <= 1.0 or shape < 0.0:
        raise ValueError("loss '{}': label_smoothing must lie in [0, 1], delta / gamma must not be negative".format(loss))
    hyper = (ls, shape, float(known.get('alpha', 0.0)), 1.0 if known.get('apply_class_balancing', False) else 0.0)
    return code, hyper, LOSS_NAMES[code]


def _f32(x):
    return float(np.float32(x))


def _bce_parts(p, y, f32_constants):
    """Keras' backend binary_crossentropy on probabilities: (term, d term / dp).  f32_constants: the clip points float32 arithmetic
    produces (epsilon = float32(1e-7), upper clip 1 - epsilon rounded to float32), as the device and Keras itself compute them."""
    eps = _f32(1e-7) if f32_constants else 1e-7
    hi = _f32(np.float32(1) - np.float32(1e-7)) if f32_constants else 1.0 - eps
    pc = np.clip(p, eps, hi)
    term = -(y * np.log(pc + eps) + (1.0 - y) * np.log(1.0 - pc + eps))
    inside = (p >= eps) & (p <= hi)
    return term, np.where(inside, -(y / (pc + eps) - (1.0 - y) / (1.0 - pc + eps)), 0.0)


def _pair_parts(code, hyper, y_true, y_pred, f32_constants=False):
    y = np.asarray(y_true, dtype=np.float64).reshape(-1)
    p = np.asarray(y_pred, dtype=np.float64).reshape(-1)
    ls, shape, alpha, balance = (float(v) for v in hyper)
    e, s = p - y, 2.0 * y - 1.0
    if code == BCE:
        return _bce_parts(p, y * (1.0 - ls) + 0.5 * ls, f32_constants)
    if code == MSE:
        return e * e, 2.0 * e
    if code == MAE:
        return np.abs(e), np.sign(e)
    if code == HINGE:
        m = np.maximum(1.0 - s * p, 0.0)
        return m, np.where(m > 0.0, -s, 0.0)
    if code == SQUARED_HINGE:
        m = np.maximum(1.0 - s * p, 0.0)
        return m * m, -2.0 * s * m
    if code == HUBER:
        quad = np.abs(e) <= shape
        return np.where(quad, 0.5 * e * e, shape * np.abs(e) - 0.5 * shape * shape), np.where(quad, e, shape * np.sign(e))
    if code == LOG_COSH:
        return e + np.logaddexp(0.0, -2.0 * e) - np.log(2.0), np.tanh(e)
    if code == POISSON:
        q = p + (_f32(1e-7) if f32_constants else 1e-7)
        return p - y * np.log(q), 1.0 - y / q
    if code == FOCAL:
        ys = y * (1.0 - ls) + 0.5 * ls
        bce, dbce = _bce_parts(p, ys, f32_constants)
        q = np.maximum(1.0 - (ys * p + (1.0 - ys) * (1.0 - p)), 0.0)
        w = ys * alpha + (1.0 - ys) * (1.0 - alpha) if balance else 1.0
        with np.errstate(divide='ignore', invalid='ignore'):
            ff = np.power(q, shape)
            dff = shape * np.power(q, shape - 1.0) * (1.0 - 2.0 * ys) if shape else np.zeros_like(q)
        return w * ff * bce, w * (dff * bce + ff * dbce)
    raise ValueError("no pointwise loss with code {}".format(code))


def pair_weights(y_true, sample_weight=None, class_weight=None):
    """float64 weight of every pair under Keras' fit(): w_j = sample_weight_j * class_weight[label_j], a missing factor 1, the class
    read from the 0/1 label itself (y > 0.5, before any smoothing).  class_weight: a pair (class 0, class 1) or a mapping with keys
    0 and 1.  None when neither is given."""
    if sample_weight is None and class_weight is None:
        return None
    y = np.asarray(y_true, dtype=np.float64).reshape(-1)
    w = np.ones(len(y))
    if sample_weight is not None:
        sw = np.asarray(sample_weight, dtype=np.float64).reshape(-1)
        if len(sw) != len(y):
            raise ValueError("sample_weight holds {} weights for {} pairs".format(len(sw), len(y)))
        w = w * sw
    if class_weight is not None:
        pair = (class_weight[0], class_weight[1])
        w = w * np.where(y > 0.5, float(pair[1]), float(pair[0]))
    return w


def loss_terms(code, hyper, y_true, y_pred, f32_constants=False, sample_weight=None, class_weight=None):
    """float64 per-pair terms of pointwise loss `code` (their sum over the batch size is the batch loss): what amar_loss_grad_f32
    writes to loss_terms; with weights (`pair_weights`) w_j x the term, what amar_loss_grad_weighted_f32 writes."""
    terms = _pair_parts(code, hyper, y_true, y_pred, f32_constants)[0]
    w = pair_weights(y_true, sample_weight, class_weight)
    return terms if w is None else w * terms


def loss_dp(code, hyper, y_true, y_pred, f32_constants=False, sample_weight=None, class_weight=None):
    """float64 d(term_i)/d(p_i) of pointwise loss `code`: 0 where the loss is flat or clipped, TensorFlow's choice (0) at MAE's kink;
    with weights w_i x that."""
    dp = _pair_parts(code, hyper, y_true, y_pred, f32_constants)[1]
    w = pair_weights(y_true, sample_weight, class_weight)
    return dp if w is None else w * dp


def _group_parts(code, hyper, y_pred, n_negatives):
    """(terms [B], d(batch loss)/dp [B]) of listwise loss `code` in float64, group by group in vector form."""
    if code not in GROUP_KINDS:
        raise ValueError("no listwise loss with code {}".format(code))
    p = np.asarray(y_pred, dtype=np.float64).reshape(-1)
    B, h, K = len(p), len(p) // 2, int(n_negatives)
    if K < 1 or h % K:
        raise ValueError("{} triples do not split into groups of n_negatives = {}".format(h, n_negatives))
    terms, dp = np.zeros(B), np.zeros(B)
    G = h // K
    if G == 0:
        return terms, dp
    a, b = p[:h:K], p[h:2 * h].reshape(G, K)                          # the positives [G], the negatives [G, K]
    da, db = dp[:h:K], dp[h:2 * h].reshape(G, K)                      # (views: written in place)
    if code == SAMPLED_SOFTMAX:
        t = float(hyper[0])
        if not t > 0.0:
            raise ValueError("temperature must be positive (got {!r})".format(hyper[0]))
        m = np.maximum(a, b.max(axis=1))
        ea, eb = np.exp((a - m) / t), np.exp((b - m[:, None]) / t)
        s = ea + eb.sum(axis=1)
        loss = -(a - m) / t + np.log(s)
        da[:] = (ea / s - 1.0) / t
        db[:] = eb / s[:, None] / t
    elif code == HARDEST_NEGATIVE:
        k = np.argmax(b, axis=1)                                      # (the first k that attains the maximum)
        x = a - b[np.arange(G), k]
        loss = np.logaddexp(0.0, -x)
        g = 1.0 / (1.0 + np.exp(x))                                   # 1 - sigmoid(x)
        da[:] = -g
        db[np.arange(G), k] = g
    else:
        mgn = float(hyper[0])
        if not mgn >= 0.0:
            raise ValueError("margin must not be negative (got {!r})".format(hyper[0]))
        v = (mgn - a)[:, None] + b
        on = v > 0.0
        loss = np.where(on, v, 0.0).sum(axis=1) / K
        da[:] = -on.sum(axis=1) / K
        db[:] = on / K
    terms[:h:K] = (B / G) * loss
    dp /= G
    return terms, dp


def group_loss_terms(code, hyper, y_pred, n_negatives=1):
    """float64 terms of listwise loss `code` (SAMPLED_SOFTMAX, HARDEST_NEGATIVE, MARGIN_RANKING) on one batch of probabilities in
    UserItemGraphTriplets' layout: terms[g K] = (B / G) l_g, every other element 0, so their sum over B is the batch loss — what
    amar_group_loss_grad_f32 writes to loss_terms.  hyper: `resolve_loss`'s tuple, [0] the temperature or the margin."""
    return _group_parts(code, hyper, y_pred, n_negatives)[0]


def group_loss_dp(code, hyper, y_pred, n_negatives=1):
    """float64 d(batch loss)/d(p_i) of listwise loss `code`: (1 / G) dl_g/dp_i, the positive's whole gradient on row g K and 0 on
    its copies and on the trailing element of an odd batch; the hardest negative's share goes to the lowest k at the maximum, a
    hinge that is not strictly positive gives 0.  amar_group_loss_grad_f32's dz is this times p (1 - p)."""
    return _group_parts(code, hyper, y_pred, n_negatives)[1]


def loss_value(loss, y_true, y_pred, sample_weight=None, class_weight=None, n_negatives=1):
    """float64 batch value of a compiled loss (anything `resolve_loss` accepts) on labels and probabilities: the sum of the per-pair
    terms over the batch size B — weighted terms too (Keras' SUM_OVER_BATCH_SIZE: the divisor is B, not the sum of the weights);
    BPRLoss's own value for BPR, which takes no weights; the mean over the groups of `n_negatives` triples for the listwise losses,
    which take none either (every other loss ignores n_negatives); an empty batch counts 0."""
    code, hyper, name = resolve_loss(loss)
    if code in GROUP_KINDS:
        if sample_weight is not None or class_weight is not None:
            raise ValueError("{} has no per-pair label or term: it takes no class_weight and no sample_weight".format(name))
        terms = group_loss_terms(code, hyper, y_pred, n_negatives)
        return float(np.sum(terms) / len(terms)) if len(terms) else 0.0
    if code == BPR:
        if sample_weight is not None or class_weight is not None:
            raise ValueError("BPRLoss has no per-pair label or term: it takes no class_weight and no sample_weight")
        return BPRLoss()(y_true, y_pred)
    terms = loss_terms(code, hyper, y_true, y_pred, sample_weight=sample_weight, class_weight=class_weight)
    return float(np.sum(terms) / len(terms)) if len(terms) else 0.0


def resolve_class_weight(value, labels=None):
    """Keras' fit(class_weight=...) for 0/1 labels as the pair (weight of class 0, weight of class 1) of Python floats; None stays None.
    `value`: a mapping whose keys are 0 and 1, as ints or as the strings YAML gives ('0', '1') — a class it leaves out weighs 1 unless
    `labels` holds that class — or 'balanced': N / (2 * count_c) over `labels` (scikit-learn's compute_class_weight).
    ValueError: another key, a negative or non-finite weight, a class of `labels` absent from the mapping, 'balanced' without labels
    or with an empty class, anything else."""
    if value is None:
        return None
    present = None
    if labels is not None:
        lab = np.asarray(labels, dtype=np.float64).reshape(-1) > 0.5
        present = (int((~lab).sum()), int(lab.sum()))
    if isinstance(value, str):
        if value != 'balanced':
            raise ValueError("class_weight must be a mapping over the classes 0 and 1 or 'balanced' (got {!r})".format(value))
        if present is None:
            raise ValueError("class_weight='balanced' needs the labels it balances")
        if min(present) == 0:
            raise ValueError("class_weight='balanced': class {} has no label".format(0 if present[0] == 0 else 1))
        n = float(sum(present))
        return n / (2.0 * present[0]), n / (2.0 * present[1])
    if not isinstance(value, Mapping):
        raise ValueError("class_weight must be a mapping over the classes 0 and 1 or 'balanced' (got {!r})".format(value))
    pair = [None, None]
    for key, weight in value.items():
        if isinstance(key, bool) or key not in (0, 1, '0', '1'):
            raise ValueError("class_weight has the classes 0 and 1 (got the key {!r})".format(key))
        c = int(key)
        if pair[c] is not None:
            raise ValueError("class_weight names class {} twice".format(c))
        try:
            weight = float(weight)
        except (TypeError, ValueError):
            raise ValueError("class_weight[{}] must be a number (got {!r})".format(c, weight))
        if not np.isfinite(weight) or weight < 0.0 or weight > float(np.finfo(np.float32).max):     # (the device holds float32)
            raise ValueError("class_weight[{}] must be finite and not negative (got {!r})".format(c, weight))
        pair[c] = weight
    for c in (0, 1):
        if pair[c] is None:
            if present is not None and present[c]:
                raise ValueError("class {} occurs in the labels and has no weight in class_weight".format(c))
            pair[c] = 1.0
    return pair[0], pair[1]
