"""Parameter counting used by the driver — mirrors `/root/reference/src/utilities/keras.py:10-22` — and the callbacks of
``fit(callbacks=[...])``: `Callback` (no-op hooks), `EarlyStopping`, `ModelCheckpoint`, `LearningRateScheduler` and `ReduceLROnPlateau`
after Keras 2's classes of the same names.  The two that move the learning rate go through training.set_learning_rate: the rate lives
in device memory, so the captured training graph replays under the new rate as it is."""
import logging
import re

import numpy as np
import torch

logger = logging.getLogger(__name__)


def get_total_parameters(model):
    """(trainable, non-trainable) parameter counts of a model."""
    trainable = sum(int(p.numel()) for p in model.trainable_weights)
    non_trainable = sum(int(p.numel()) for p in model.non_trainable_weights)
    return trainable, non_trainable


class Callback:
    """Base class of fit()'s callbacks: every hook does nothing.  fit() duck-types, so deriving from this class is optional; the
    batch hooks are called only where a callback overrides them, with logs = {} (training.py:_FitHooks)."""

    model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_train_batch_begin(self, batch, logs=None):
        pass

    def on_train_batch_end(self, batch, logs=None):
        pass


_MAX_SUFFIXES = ('acc', 'accuracy', 'auc', 'precision', 'recall')


def monitor_mode(monitor, mode='auto'):
    """'min' or 'max' for a monitored history name.  mode='auto': 'max' for names ending in acc, accuracy or auc (Keras' rule) and,
    here, in precision or recall and for the ranking names *_at_<k>; 'min' for every other name."""
    if mode in ('min', 'max'):
        return mode
    if mode != 'auto':
        raise ValueError("mode must be 'auto', 'min' or 'max' (got {!r})".format(mode))
    name = str(monitor)
    return 'max' if name.endswith(_MAX_SUFFIXES) or re.search(r'_at_\d+$', name) else 'min'


def get_weights_device(model):
    """Clones of every parameter of `model`, where the parameters live (the device)."""
    return [prm.detach().clone() for prm in model.parameters()]


def set_weights_device(model, weights):
    """Copy `weights` (as get_weights_device returned them) into the model's parameters in place.  The in-place copy moves every
    parameter's version counter, so whatever is keyed on Model.weights_version — the hoisted propagation, the towers, packed Dense
    blobs, the captured predict graph — is rebuilt on next use, while the captured training graph, which holds the parameters'
    addresses, stays valid.  Optimizer state is left alone."""
    params = list(model.parameters())
    if len(params) != len(weights):
        raise ValueError("set_weights_device: {} tensors for {} parameters".format(len(weights), len(params)))
    with torch.no_grad():
        for prm, value in zip(params, weights):
            prm.copy_(value)


class EarlyStopping(Callback):
    """Keras 2's EarlyStopping.  On every on_epoch_end whose logs hold `monitor`, from epoch `start_from_epoch` on:
    the current weights are stored if restore_best_weights is set and none are stored yet; wait += 1; the value improves when it
    beats `best` (starting at +-inf) by more than |min_delta|; an improvement sets best / best_epoch, stores the weights if asked and
    sets wait = 0 unless a `baseline` is given that the value does not beat; with wait >= patience and epoch > 0 training stops
    (stopped_epoch = epoch, model.stop_training = True) and the stored weights are put back if asked.  A missing monitor key warns once.
    Stored weights are device clones (`get_weights_device`); `get_weights` / `set_weights` may be overridden (the tests do, with a
    model that has no parameters)."""

    def __init__(self, monitor='val_loss', min_delta=0, patience=0, mode='auto', baseline=None, restore_best_weights=False,
                 start_from_epoch=0):
        self.monitor, self.min_delta, self.patience = monitor, abs(float(min_delta)), int(patience)
        self.mode = monitor_mode(monitor, mode)
        self.baseline, self.restore_best_weights, self.start_from_epoch = baseline, bool(restore_best_weights), int(start_from_epoch)
        self._warned = False
        self.on_train_begin()

    def get_weights(self):
        fn = getattr(self.model, 'get_weights', None)
        return fn() if callable(fn) else get_weights_device(self.model)

    def set_weights(self, weights):
        fn = getattr(self.model, 'set_weights', None)
        return fn(weights) if callable(fn) else set_weights_device(self.model, weights)

    def _better(self, value, reference):
        return value + self.min_delta < reference if self.mode == 'min' else value - self.min_delta > reference

    def on_train_begin(self, logs=None):
        self.wait, self.stopped_epoch, self.best_epoch = 0, 0, 0
        self.best = np.inf if self.mode == 'min' else -np.inf
        self.best_weights = None

    def on_epoch_end(self, epoch, logs=None):
        value = (logs or {}).get(self.monitor)
        if value is None:
            if not self._warned:
                logger.warning("EarlyStopping: the monitored value '%s' is not in the epoch's logs (%s)", self.monitor,
                               ', '.join(sorted(logs or {})))
                self._warned = True
            return
        if epoch < self.start_from_epoch:
            return
        value = float(value)
        if self.restore_best_weights and self.best_weights is None:
            self.best_weights = self.get_weights()
        self.wait += 1
        if self._better(value, self.best):
            self.best, self.best_epoch = value, epoch
            if self.restore_best_weights:
                self.best_weights = self.get_weights()
            if self.baseline is None or self._better(value, float(self.baseline)):
                self.wait = 0
        if self.wait >= self.patience and epoch > 0:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.restore_best_weights and self.best_weights is not None:
                self.set_weights(self.best_weights)


class ModelCheckpoint(Callback):
    """Keras 2's ModelCheckpoint on Model.save_weights: after every epoch (save_best_only=False) or after every epoch whose `monitor`
    improved on the best so far, the weights go to `filepath.format(epoch=epoch + 1, **logs)`."""

    def __init__(self, filepath, monitor='val_loss', save_best_only=False, mode='auto'):
        self.filepath, self.monitor, self.save_best_only = str(filepath), monitor, bool(save_best_only)
        self.mode = monitor_mode(monitor, mode)
        self.best = np.inf if self.mode == 'min' else -np.inf
        self._warned = False
        self.saved = []

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        if self.save_best_only:
            value = logs.get(self.monitor)
            if value is None:
                if not self._warned:
                    logger.warning("ModelCheckpoint: the monitored value '%s' is not in the epoch's logs", self.monitor)
                    self._warned = True
                return
            value = float(value)
            if not (value < self.best if self.mode == 'min' else value > self.best):
                return
            self.best = value
        path = self.filepath.format(epoch=epoch + 1, **logs)
        self.model.save_weights(path)
        self.saved.append(path)


def _get_lr(model):
    fn = getattr(model, 'get_learning_rate', None)
    if callable(fn):
        return float(fn())
    from deep_cbrs_amar_renaissance_amd import training
    return training.get_learning_rate(model)


def _set_lr(model, value):
    fn = getattr(model, 'set_learning_rate', None)
    if callable(fn):
        return fn(value)
    from deep_cbrs_amar_renaissance_amd import training
    return training.set_learning_rate(model, value)


class LearningRateScheduler(Callback):
    """Keras 2's LearningRateScheduler: at every on_epoch_begin the rate becomes schedule(epoch, current rate) — schedule(epoch) for a
    function of one argument (a TypeError of the first call) — which must be a float; on_epoch_end puts the rate in force into
    logs['lr'].  A model may bring its own get_learning_rate() / set_learning_rate(value) (the tests do); otherwise the rate is the
    trainer's (training.get_learning_rate / set_learning_rate)."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, int(verbose)

    def on_epoch_begin(self, epoch, logs=None):
        try:
            value = self.schedule(epoch, _get_lr(self.model))
        except TypeError:                                            # the older form: a function of the epoch alone
            value = self.schedule(epoch)
        if not isinstance(value, (float, np.float32, np.float64)):
            raise ValueError('The output of the "schedule" function should be float (got {!r})'.format(value))
        _set_lr(self.model, float(value))
        if self.verbose:
            print("Epoch {}: LearningRateScheduler setting learning rate to {}.".format(epoch + 1, float(value)))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs['lr'] = _get_lr(self.model)


class ReduceLROnPlateau(Callback):
    """Keras 2's ReduceLROnPlateau.  on_train_begin resets best (+-inf), wait and cooldown_counter.  On every on_epoch_end: logs['lr'] =
    the rate in force; a missing monitor key warns once and ends the call; in cooldown the counter goes down and wait = 0; a value
    better than best by more than min_delta (value < best - min_delta for 'min', value > best + min_delta for 'max') becomes best and
    sets wait = 0; otherwise, outside cooldown, wait += 1, and with wait >= patience and rate > min_lr the rate becomes
    max(rate * factor, min_lr), the cooldown starts and wait = 0."""

    def __init__(self, monitor='val_loss', factor=0.1, patience=10, verbose=0, mode='auto', min_delta=1e-4, cooldown=0, min_lr=0):
        if float(factor) >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0 (got {})".format(factor))
        self.monitor, self.factor, self.patience, self.verbose = monitor, float(factor), int(patience), int(verbose)
        self.min_delta, self.cooldown, self.min_lr = float(min_delta), int(cooldown), float(min_lr)
        self.mode = monitor_mode(monitor, mode)
        self._warned = False
        self.on_train_begin()

    def _better(self, value, reference):
        return value < reference - self.min_delta if self.mode == 'min' else value > reference + self.min_delta

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_train_begin(self, logs=None):
        self.best = np.inf if self.mode == 'min' else -np.inf
        self.wait, self.cooldown_counter = 0, 0
        if self.model is not None and not callable(getattr(self.model, 'set_learning_rate', None)):
            from deep_cbrs_amar_renaissance_amd import training
            training.make_learning_rate_dynamic(self.model)          # the rate on the device from the first epoch on: one capture, `lr` in every epoch

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs['lr'] = _get_lr(self.model)
        value = logs.get(self.monitor)
        if value is None:
            if not self._warned:
                logger.warning("ReduceLROnPlateau: the monitored value '%s' is not in the epoch's logs (%s)", self.monitor,
                               ', '.join(sorted(logs)))
                self._warned = True
            return
        value = float(value)
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self._better(value, self.best):
            self.best, self.wait = value, 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old = _get_lr(self.model)
                if old > np.float32(self.min_lr):
                    new = max(old * self.factor, self.min_lr)
                    _set_lr(self.model, new)
                    if self.verbose:
                        print("Epoch {}: ReduceLROnPlateau reducing learning rate to {}.".format(epoch + 1, new))
                    self.cooldown_counter, self.wait = self.cooldown, 0
