"""Parameter counting used by the driver — mirrors `/root/reference/src/utilities/keras.py:10-22` — and the callbacks of
``fit(callbacks=[...])``: `Callback` (no-op hooks), `EarlyStopping` and `ModelCheckpoint` after Keras 2's classes of the same names.
ReduceLROnPlateau and the like are not offered: the learning rate is baked into the captured training graph."""
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
