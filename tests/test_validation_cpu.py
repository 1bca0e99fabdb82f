"""Host: validation during fit() — EarlyStopping's rule on scripted logs, holdout_split, the binding of amar_rank_metrics_f64 and
the argument checks of its wrapper (pytest -m "not gpu")."""
import logging
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeModel:
    """stop_training and a weight store, no GPU: the 'weights' are the epoch that produced them."""

    def __init__(self):
        self.stop_training, self.weights, self.restored = False, None, None

    def get_weights(self):
        return self.weights

    def set_weights(self, weights):
        self.restored = weights


def _run(values, key='val_loss', **kwargs):
    from deep_cbrs_amar_renaissance_amd.utilities.keras import EarlyStopping
    model = _FakeModel()
    stop = EarlyStopping(**kwargs)
    stop.set_model(model)
    stop.on_train_begin()
    ran = 0
    for epoch, value in enumerate(values):
        model.weights = epoch
        stop.on_epoch_end(epoch, {'loss': 0.0, key: value})
        ran += 1
        if model.stop_training:
            break
    return stop, model, ran


def test_early_stopping_patience_two():
    stop, model, ran = _run([1.0, 0.9, 0.95, 0.97, 0.5], patience=2, restore_best_weights=True)
    assert model.stop_training and ran == 4 and stop.stopped_epoch == 3 and stop.best_epoch == 1 and stop.best == 0.9
    assert model.restored == 1                                               # the weights of the best epoch were put back


def test_early_stopping_patience_zero_never_stops_at_epoch_zero():
    stop, model, ran = _run([1.0, 1.1, 0.2], patience=0)
    assert ran == 2 and stop.stopped_epoch == 1 and stop.best_epoch == 0 and model.restored is None
    stop, model, ran = _run([1.0], patience=0)
    assert ran == 1 and not model.stop_training                             # wait >= patience at epoch 0 already: epoch > 0 is required


def test_early_stopping_min_delta():
    stop, _, ran = _run([1.0, 0.9, 0.85], patience=2, min_delta=0.2)
    assert ran == 3 and stop.best_epoch == 0 and stop.best == 1.0 and stop.stopped_epoch == 2       # 0.9 is no improvement on 1.0
    stop, _, ran = _run([1.0, 0.9, 0.85], patience=2, min_delta=-0.2)                                   # |min_delta|
    assert stop.best_epoch == 0


def test_early_stopping_auto_mode_is_max_for_auc():
    from deep_cbrs_amar_renaissance_amd.utilities.keras import monitor_mode
    stop, model, ran = _run([0.5, 0.6, 0.55, 0.58, 0.9], key='val_auc', monitor='val_auc', patience=2)
    assert stop.mode == 'max' and ran == 4 and stop.best_epoch == 1 and stop.best == 0.6 and stop.stopped_epoch == 3
    for name in ('val_acc', 'val_accuracy', 'auc', 'val_precision', 'val_recall', 'val_ndcg_at_10', 'val_hit_at_5'):
        assert monitor_mode(name) == 'max', name
    for name in ('val_loss', 'loss', 'scripted', 'val_ndcg_at_k'):
        assert monitor_mode(name) == 'min', name
    assert monitor_mode('val_auc', 'min') == 'min'
    with pytest.raises(ValueError):
        monitor_mode('val_loss', 'best')


def test_early_stopping_start_from_epoch():
    stop, _, ran = _run([0.1, 0.2, 0.3, 0.4, 0.5], patience=1, start_from_epoch=2)
    # epochs 0 and 1 are not looked at: 0.3 at epoch 2 is the first (and best) value, 0.4 at epoch 3 uses up the patience
    assert ran == 4 and stop.best_epoch == 2 and stop.best == 0.3 and stop.stopped_epoch == 3


def test_early_stopping_baseline():
    # improvements that do not beat the baseline do not reset the wait
    stop, _, ran = _run([1.0, 0.9, 0.8, 0.7], patience=2, baseline=0.5)
    assert ran == 2 and stop.stopped_epoch == 1 and stop.best == 0.9
    stop, _, ran = _run([1.0, 0.4, 0.45, 0.47], patience=2, baseline=0.5)
    assert ran == 4 and stop.best_epoch == 1 and stop.stopped_epoch == 3


def test_early_stopping_warns_once_on_a_missing_key(caplog):
    with caplog.at_level(logging.WARNING):
        stop, model, ran = _run([1.0, 2.0, 3.0], key='other', monitor='val_loss', patience=0)
    assert ran == 3 and not model.stop_training and stop.wait == 0
    assert len([r for r in caplog.records if 'val_loss' in r.getMessage()]) == 1


def _split_input(seed=0):
    """900 rows over 40 users x 60 items, no pair twice, plus a user and an item with a single row each."""
    rng = np.random.default_rng(seed)
    keys = rng.choice(40 * 60, size=898, replace=False)
    r = np.stack([keys // 60 + 100, keys % 60 + 1000, rng.integers(0, 2, size=898)], axis=1)
    return np.concatenate([r, [[999, 1000, 1], [100, 9999, 0]]])


def test_holdout_split():
    from deep_cbrs_amar_renaissance_amd.data.datasets import holdout_split
    r, fraction = _split_input(), 0.1
    n, n_users, n_items = len(r), len(np.unique(r[:, 0])), len(np.unique(r[:, 1]))
    # a maximal set of movable rows leaves every kept row as the last one of its user or of its item: n - |U| - |I| rows can always move
    assert n - n_users - n_items >= 0.8 * fraction * n
    kept, held = holdout_split(r, fraction, 7)
    as_set = lambda a: set(map(tuple, a.tolist()))
    assert len(kept) + len(held) == n and as_set(kept) | as_set(held) == as_set(r) and not as_set(kept) & as_set(held)
    assert set(kept[:, 0]) == set(r[:, 0]) and set(kept[:, 1]) == set(r[:, 1])
    assert 0.8 * fraction * n <= len(held) <= round(fraction * n)
    assert 999 not in held[:, 0] and 9999 not in held[:, 1]
    again = holdout_split(r, fraction, 7)
    assert np.array_equal(again[0], kept) and np.array_equal(again[1], held)
    other = holdout_split(r, fraction, 8)
    assert not np.array_equal(other[1], held)
    kept0, held0 = holdout_split(r, 0.0, 7)
    assert len(held0) == 0 and np.array_equal(kept0, r)
    # nothing may move where every row is the only one of its user: the rule wins over the fraction
    lonely = np.stack([np.arange(20), np.zeros(20, dtype=np.int64) + 500, np.ones(20, dtype=np.int64)], axis=1)
    assert len(holdout_split(lonely, 0.5, 1)[1]) == 0
    with pytest.raises(ValueError):
        holdout_split(r, 1.0, 1)


def test_rank_metrics_symbol_is_bound_and_declared():
    from deep_cbrs_amar_renaissance_amd import capi
    header = open(os.path.join(ROOT, 'include', 'amar_hip.h')).read()
    assert 'amar_rank_metrics_f64' in capi.SIGNATURES
    assert re.search(r'\bint\s+amar_rank_metrics_f64\s*\(', header)
    assert len(capi.SIGNATURES['amar_rank_metrics_f64'][1]) == 14
    assert 'amar_rank_metrics.hip' in open(os.path.join(ROOT, 'deep_cbrs_amar_renaissance_amd', 'csrc', 'Makefile')).read()
    assert int(re.search(r'#define\s+AMAR_RANK_METRICS_MAX_KS\s+(\d+)', header).group(1)) == capi.RANK_METRICS_MAX_KS
    assert int(re.search(r'#define\s+AMAR_RANK_METRICS_MAX_BLOCKS\s+(\d+)', header).group(1)) == capi.RANK_METRICS_MAX_BLOCKS


def test_rank_metrics_wrapper_refuses_bad_cutoffs():
    from deep_cbrs_amar_renaissance_amd import capi
    ks, cum = capi.rank_metrics_args(64, [1, 5, 64])
    assert ks == [1, 5, 64] and cum.dtype == np.float64 and cum.shape == (65,) and cum[0] == 0.0 and cum[1] == 1.0
    assert abs(cum[3] - (1.0 + 1.0 / np.log2(3.0) + 0.5)) < 1e-15
    for K, bad in ((65, [1]), (0, [1]), (10, []), (10, list(range(1, 10))), (10, [0]), (10, [11]), (1, [2])):
        with pytest.raises(ValueError):
            capi.rank_metrics_args(K, bad)


def test_fit_hooks_skip_inherited_batch_hooks():
    """A callback deriving from Callback without overriding the batch hooks is not called per batch."""
    from deep_cbrs_amar_renaissance_amd import training
    from deep_cbrs_amar_renaissance_amd.utilities.keras import Callback

    class Plain(Callback):
        def on_epoch_end(self, epoch, logs=None):
            logs['seen'] = epoch

    class PerBatch(Callback):
        def on_train_batch_end(self, batch, logs=None):
            pass

    class History:
        values = {'loss': [0.5]}
        trainer = type('T', (), {'_compiled': staticmethod(lambda: (0, (0.0,), []))})()

    model = type('M', (), {'stop_training': False})()
    assert training._fit_hooks(model, History(), None, None, 1, None) is None
    hooks = training._fit_hooks(model, History(), [Plain(), PerBatch()], None, 1, None)
    assert len(hooks.batch_begin) == 0 and len(hooks.batch_end) == 1 and len(hooks.hooks['on_epoch_end']) == 1
    assert hooks.epoch_end(0, False) is False
    with pytest.raises(NotImplementedError):
        training._fit_hooks(model, History(), None, None, 1, {'trainset': None, 'ratings': None, 'ks': [5]})
