"""CPU: the compiled losses and metrics on the host — the float64 restatements of Keras' pointwise losses against Keras' documented
values, their analytic gradients against central differences, name resolution and its two errors, and the metric values that come
out of a counter block."""
import os
import re

import numpy as np
import pytest

from deep_cbrs_amar_renaissance_amd.utilities import losses as L
from deep_cbrs_amar_renaissance_amd.utilities import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y4, P4 = [0, 1, 0, 0], [.6, .4, .4, .6]                               # Keras' docstring example, flattened


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


@pytest.mark.parametrize('name,want', [('hinge', 1.3), ('squared_hinge', 1.86), ('huber', 0.155), ('mse', 0.31), ('mae', 0.55)])
def test_documented_values(name, want):
    assert abs(L.loss_value(name, Y4, P4) - want) < 1e-12


def test_documented_values_log_cosh_poisson():
    p = [1, 1, 0, 0]
    assert abs(L.loss_value('log_cosh', Y4, p) - 0.108445) < 1e-6
    assert abs(L.loss_value('poisson', Y4, p) - 0.5) < 1e-6


def test_documented_values_focal():
    p = _sigmoid([-18.6, 0.51, 2.94, -12.8])
    assert abs(L.loss_value('binary_focal_crossentropy', Y4, p) - 0.691212) < 1e-6
    assert abs(L.loss_value({'name': 'binary_focal_crossentropy', 'gamma': 3}, Y4, p) - 0.646995) < 1e-6
    assert abs(L.loss_value({'name': 'binary_focal_crossentropy', 'apply_class_balancing': True, 'alpha': .25}, Y4, p) - 0.510133) < 1e-6


def test_cross_entropy_matches_keras_backend_form_and_smoothing():
    p, y = np.array([.6, .4, .4, .6]), np.array([0., 1., 0., 0.])
    want = -np.mean(y * np.log(p + 1e-7) + (1 - y) * np.log(1 - p + 1e-7))
    assert abs(L.loss_value(None, y, p) - want) < 1e-15 and abs(L.loss_value('BinaryCrossentropy', y, p) - want) < 1e-15
    ys = y * 0.8 + 0.1
    want_s = -np.mean(ys * np.log(p + 1e-7) + (1 - ys) * np.log(1 - p + 1e-7))
    assert abs(L.loss_value({'name': 'binary_crossentropy', 'label_smoothing': 0.2}, y, p) - want_s) < 1e-15


GRAD_CASES = ['binary_crossentropy', {'name': 'binary_crossentropy', 'label_smoothing': 0.1}, 'mse', 'mae', 'hinge', 'squared_hinge',
              {'name': 'huber', 'delta': 0.25}, 'log_cosh', 'poisson', 'binary_focal_crossentropy',
              {'name': 'binary_focal_crossentropy', 'gamma': 3.0, 'apply_class_balancing': True, 'alpha': 0.4, 'label_smoothing': 0.1}]


@pytest.mark.parametrize('loss', GRAD_CASES, ids=lambda v: v if isinstance(v, str) else '-'.join(str(x) for x in v.values()))
def test_analytic_gradient_against_central_difference(loss):
    code, hyper, _ = L.resolve_loss(loss)
    rng = np.random.default_rng(7)
    p = rng.uniform(0.02, 0.98, 400)
    y = rng.integers(0, 2, 400).astype(np.float64)
    h = 1e-6
    away = np.abs(np.abs(p - y) - 0.25) > 1e-3                       # Huber's kink at |e| = delta (the other kinks lie at p = y or outside)
    num = (L.loss_terms(code, hyper, y, p + h) - L.loss_terms(code, hyper, y, p - h)) / (2 * h)
    got = L.loss_dp(code, hyper, y, p)
    assert away.sum() > 300
    np.testing.assert_allclose(got[away], num[away], rtol=1e-6, atol=1e-8)


def test_flat_and_clipped_gradients_are_zero():
    hinge = L.resolve_loss('hinge')
    assert L.loss_dp(hinge[0], hinge[1], [1.0], [1.0])[0] == 0 and L.loss_terms(hinge[0], hinge[1], [1.0], [1.0])[0] == 0
    bce = L.resolve_loss(None)
    assert np.all(L.loss_dp(bce[0], bce[1], [0, 1, 1, 0], [0.0, 1.0, 1e-9, 1 - 1e-9]) == 0)
    mae = L.resolve_loss('mae')
    assert L.loss_dp(mae[0], mae[1], [1.0], [1.0])[0] == 0


ALIASES = {
    L.BCE: ['binary_crossentropy', 'BinaryCrossentropy', None], L.MSE: ['mean_squared_error', 'mse', 'MSE', 'MeanSquaredError'],
    L.MAE: ['mean_absolute_error', 'mae', 'MAE', 'MeanAbsoluteError'], L.HINGE: ['hinge', 'Hinge'],
    L.SQUARED_HINGE: ['squared_hinge', 'SquaredHinge'], L.HUBER: ['huber', 'huber_loss', 'Huber'],
    L.LOG_COSH: ['log_cosh', 'logcosh', 'LogCosh'], L.POISSON: ['poisson', 'Poisson'],
    L.FOCAL: ['binary_focal_crossentropy', 'BinaryFocalCrossentropy'], L.BPR: ['BPRLoss', L.BPRLoss()],
}


def test_every_alias_and_class_name_resolves():
    for code, names in ALIASES.items():
        for name in names:
            assert L.resolve_loss(name)[0] == code, name
            if not isinstance(name, L.BPRLoss):
                assert L.resolve_loss({'name': name})[0] == code, name
    assert {L.resolve_loss(n)[2] for n in ALIASES[L.MSE]} == {'mean_squared_error'}


def test_mean_squared_error_is_not_cross_entropy():
    """Fails before this feature: every name but BPRLoss trained binary cross-entropy."""
    assert L.resolve_loss('mean_squared_error')[0] != L.resolve_loss('binary_crossentropy')[0]
    assert L.loss_kind('mean_squared_error') == 'bce' and L.loss_kind(L.BPRLoss()) == 'bpr'     # (loss_kind keeps telling BPR from the rest)


def test_mapping_form_carries_hyper_parameters():
    assert L.resolve_loss('huber')[1] == (0.0, 1.0, 0.0, 0.0)
    assert L.resolve_loss({'name': 'huber', 'delta': 0.5})[1] == (0.0, 0.5, 0.0, 0.0)
    assert L.resolve_loss('binary_focal_crossentropy')[1] == (0.0, 2.0, 0.25, 0.0)
    focal = {'name': 'BinaryFocalCrossentropy', 'gamma': 3, 'alpha': 0.4, 'apply_class_balancing': True, 'label_smoothing': 0.1}
    assert L.resolve_loss(focal)[1] == (0.1, 3.0, 0.4, 1.0)
    assert L.resolve_loss({'name': 'binary_crossentropy', 'label_smoothing': 0.2})[1][0] == 0.2
    with pytest.raises(ValueError):
        L.resolve_loss({'name': 'mse', 'delta': 1.0})
    with pytest.raises(ValueError):
        L.resolve_loss({'name': 'binary_crossentropy', 'label_smoothing': 1.5})
    with pytest.raises(ValueError):
        L.resolve_loss({'delta': 1.0})


def test_unknown_and_unsupported_names():
    with pytest.raises(ValueError, match='no_such_loss'):
        L.resolve_loss('no_such_loss')
    for name in ('categorical_crossentropy', 'kl_divergence', 'cosine_similarity'):
        with pytest.raises(NotImplementedError, match='mean_squared_error'):      # (the message names the supported set)
            L.resolve_loss(name)
    with pytest.raises(NotImplementedError):
        M.resolve_metrics(['TopKCategoricalAccuracy'])
    with pytest.raises(ValueError):
        M.resolve_metrics(['no_such_metric'])


def test_metric_names_resolve_in_compile_order():
    assert M.resolve_metrics(['AUC', 'acc', 'Recall', 'precision']) == ['auc', 'accuracy', 'recall', 'precision']
    for names, want in ((['accuracy', 'acc', 'binary_accuracy', 'BinaryAccuracy'], ['accuracy']), (['Precision', 'precision'], ['precision']),
                        (['Recall', 'recall'], ['recall']), (['AUC', 'auc'], ['auc']), (None, [])):
        assert M.resolve_metrics(names) == want


def test_compile_raises_both_errors_and_bpr_takes_only_accuracy():
    from deep_cbrs_amar_renaissance_amd import engine
    model = engine.Model()
    with pytest.raises(ValueError):
        model.compile(loss='no_such_loss')
    with pytest.raises(NotImplementedError):
        model.compile(loss='categorical_crossentropy')
    with pytest.raises(NotImplementedError):
        model.compile(loss='mse', metrics=['TopKCategoricalAccuracy'])
    model.compile(loss=L.BPRLoss(), metrics=['accuracy'])
    assert M.resolve_compiled(model.loss, model.metrics)[2] == []
    with pytest.raises(NotImplementedError):
        model.compile(loss=L.BPRLoss(), metrics=['accuracy', 'AUC'])
    model.compile(loss={'name': 'huber', 'delta': 0.5}, metrics=['accuracy', 'AUC'])
    assert M.resolve_compiled(model.loss, model.metrics) == (L.HUBER, (0.0, 0.5, 0.0, 0.0), ['accuracy', 'auc'])


def test_auc_precision_recall_values():
    c = M.metric_counters([0, .5, .3, .9], [0, 0, 1, 1])
    assert c.dtype == np.int64 and len(c) == M.N_COUNTERS == 402 and c[:4].tolist() == [1, 0, 2, 1] and c[4:].sum() == 4
    v = M.metric_values(c, ['auc', 'accuracy', 'precision', 'recall'])
    assert list(v) == ['auc', 'accuracy', 'precision', 'recall']
    assert abs(v['auc'] - 0.75) < 1e-12 and v['accuracy'] == 0.75 and v['precision'] == 1.0 and v['recall'] == 0.5
    empty = M.metric_values(M.metric_counters([0.2, 0.3], [0, 0]), ['precision', 'recall'])
    assert empty == {'precision': 0.0, 'recall': 0.0}                # div_no_nan: no predicted / no actual positive
    assert M.metric_values(np.zeros(402, dtype=np.int64), ['accuracy', 'auc']) == {'accuracy': 0.0, 'auc': 0.0}


def test_auc_matches_the_threshold_definition():
    """Keras' AUC from its definition — confusion counts at each of the 200 thresholds, trapezoid rule — on random scores that
    include exact thresholds and their float neighbours."""
    rng = np.random.default_rng(11)
    p = rng.uniform(0, 1, 500).astype(np.float32)
    thr = M.auc_thresholds()
    assert thr.dtype == np.float32 and len(thr) == 198 and thr[0] == np.float32(1 / 199.0) and thr[-1] == np.float32(198 / 199.0)
    p[:198] = thr
    p[198:300] = np.nextafter(thr[:102], np.float32(1))
    p[300:400] = np.nextafter(thr[50:150], np.float32(0))
    y = rng.integers(0, 2, 500)
    full = np.concatenate([[-1e-7], thr.astype(np.float64), [1 + 1e-7]])
    above = p.astype(np.float64)[None, :] > full[:, None]
    tp, fp = (above & (y == 1)).sum(1), (above & (y == 0)).sum(1)
    rec, fpr = tp / (y == 1).sum(), fp / (y == 0).sum()
    want = float(np.sum((fpr[:-1] - fpr[1:]) * (rec[:-1] + rec[1:]) / 2))
    assert abs(M.metric_values(M.metric_counters(p, y), ['auc'])['auc'] - want) < 1e-12


def test_binding_and_header_declare_the_entry_points():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    for sym in ('amar_loss_grad_f32', 'amar_loss_counters'):
        assert sym in capi.SIGNATURES and re.search(r'\b' + sym + r'\s*\(', header)
    codes = {name: int(value) for name, value in re.findall(r'#define AMAR_LOSS_([A-Z_]+)\s+(\d+)\s', header)}
    assert codes == {'BCE': L.BCE, 'MSE': L.MSE, 'MAE': L.MAE, 'HINGE': L.HINGE, 'SQUARED_HINGE': L.SQUARED_HINGE, 'HUBER': L.HUBER,
                     'LOG_COSH': L.LOG_COSH, 'POISSON': L.POISSON, 'FOCAL': L.FOCAL, 'HYPER_FLOATS': capi.LOSS_HYPER_FLOATS}
    assert (capi.LOSS_BCE, capi.LOSS_FOCAL) == (L.BCE, L.FOCAL) and capi.LOSS_COUNTERS == M.N_COUNTERS == capi.loss_counters()
