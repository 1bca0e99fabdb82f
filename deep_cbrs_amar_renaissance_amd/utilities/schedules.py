"""Learning-rate schedules after tf.keras.optimizers.schedules: ExponentialDecay, InverseTimeDecay, PolynomialDecay, CosineDecay and
PiecewiseConstantDecay, with Keras' constructor signatures and defaults.  An optimizer takes one as its `learning_rate`; training.py
hands it to the device (capi.lr_schedule -> amar_lr_schedule), where the kernel that advances the optimizer state evaluates it at the
step counter, so a replayed training batch follows it without being captured again.

`schedule(step)` here is the host restatement of that device function (include/amar_hip.h states the formulas): the parameters rounded
to float32, as the device receives them and as Keras holds them, the arithmetic in float64 without fused products, one rounding to
float32 at the end.  `step` is zero-based: the first training step runs at schedule(0)."""
import math

import numpy as np

MAX_BOUNDARIES = 16


def _f32(value):
    return float(np.float32(value))


class LearningRateSchedule:
    """Base class: `kind` names the device formula, `_fields` the constructor arguments in order (get_config, key)."""
    kind = None
    _fields = ()

    def get_config(self):
        return {name: getattr(self, name) for name in self._fields}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    @property
    def key(self):
        """Hashable; equal for schedules that give the same rates (part of training.OptimizerSpec.key)."""
        return (type(self).__name__,) + tuple(tuple(v) if isinstance(v, list) else v for v in (getattr(self, n) for n in self._fields))

    def __eq__(self, other):
        return isinstance(other, LearningRateSchedule) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return "{}({})".format(type(self).__name__, ', '.join("{}={!r}".format(k, v) for k, v in self.get_config().items()))

    def _decay_steps(self, decay_steps):
        if not float(decay_steps) > 0.0:
            raise ValueError("{}: decay_steps must be positive (got {!r})".format(type(self).__name__, decay_steps))
        return decay_steps

    def __call__(self, step):
        s = float(step)
        if not 0.0 <= s < float(1 << 24):
            raise ValueError("a schedule is defined for steps 0 .. 2^24 - 1 (got {!r})".format(step))
        return np.float32(self._rate(s))


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ^ (step / decay_steps); staircase: floor(step / decay_steps)."""
    kind = 'exponential'
    _fields = ('initial_learning_rate', 'decay_steps', 'decay_rate', 'staircase')

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate, self.decay_steps = float(initial_learning_rate), self._decay_steps(decay_steps)
        self.decay_rate, self.staircase, self.name = float(decay_rate), bool(staircase), name

    def _progress(self, s):
        p = s / _f32(self.decay_steps)
        return math.floor(p) if self.staircase else p

    def _rate(self, s):
        return _f32(self.initial_learning_rate) * _f32(self.decay_rate) ** self._progress(s)

    def device_args(self):
        return dict(kind=self.kind, staircase=self.staircase, initial_learning_rate=self.initial_learning_rate,
                    decay_steps=self.decay_steps, decay_rate=self.decay_rate)


class InverseTimeDecay(ExponentialDecay):
    """initial_learning_rate / (1 + decay_rate * step / decay_steps); staircase: floor(step / decay_steps).  Keras 2's optimizer
    argument `decay` is InverseTimeDecay(learning_rate, 1, decay)."""
    kind = 'inverse_time'

    def _rate(self, s):
        return _f32(self.initial_learning_rate) / (1.0 + _f32(self.decay_rate) * self._progress(s))


class PolynomialDecay(LearningRateSchedule):
    """(initial - end) * (1 - min(step, decay_steps) / decay_steps) ^ power + end; cycle: decay_steps grows to the next multiple that
    holds the step, and there is no min."""
    kind = 'polynomial'
    _fields = ('initial_learning_rate', 'decay_steps', 'end_learning_rate', 'power', 'cycle')

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False, name=None):
        self.initial_learning_rate, self.decay_steps = float(initial_learning_rate), self._decay_steps(decay_steps)
        self.end_learning_rate, self.power, self.cycle, self.name = float(end_learning_rate), float(power), bool(cycle), name

    def _rate(self, s):
        lr0, d, end = _f32(self.initial_learning_rate), _f32(self.decay_steps), _f32(self.end_learning_rate)
        if self.cycle:
            p = s / (d * (1.0 if s == 0.0 else math.ceil(s / d)))
        else:
            p = min(s, d) / d
        return (lr0 - end) * (1.0 - p) ** _f32(self.power) + end

    def device_args(self):
        return dict(kind=self.kind, cycle=self.cycle, initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    end_learning_rate=self.end_learning_rate, power=self.power)


class CosineDecay(LearningRateSchedule):
    """initial * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)."""
    kind = 'cosine'
    _fields = ('initial_learning_rate', 'decay_steps', 'alpha')

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        self.initial_learning_rate, self.decay_steps = float(initial_learning_rate), self._decay_steps(decay_steps)
        self.alpha, self.name = float(alpha), name

    def _rate(self, s):
        lr0, d, alpha = _f32(self.initial_learning_rate), _f32(self.decay_steps), _f32(self.alpha)
        c = 0.5 * (1.0 + math.cos(math.pi * (min(s, d) / d)))
        return lr0 * ((1.0 - alpha) * c + alpha)

    def device_args(self):
        return dict(kind=self.kind, initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps, alpha=self.alpha)


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] up to and including step boundaries[0], values[i] for boundaries[i-1] < step <= boundaries[i], values[-1] beyond."""
    kind = 'piecewise'
    _fields = ('boundaries', 'values')

    def __init__(self, boundaries, values, name=None):
        self.boundaries, self.values, self.name = [float(b) for b in boundaries], [float(v) for v in values], name
        if not 1 <= len(self.boundaries) <= MAX_BOUNDARIES:
            raise ValueError("PiecewiseConstantDecay: 1 .. {} boundaries (got {})".format(MAX_BOUNDARIES, len(self.boundaries)))
        if len(self.values) != len(self.boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay: {} boundaries need {} values (got {})".format(
                len(self.boundaries), len(self.boundaries) + 1, len(self.values)))

    def _rate(self, s):
        for b, v in zip(self.boundaries, self.values):
            if s <= _f32(b):
                return v
        return self.values[-1]

    def device_args(self):
        return dict(kind=self.kind, boundaries=self.boundaries, values=self.values)


class CosineDecayRestarts(LearningRateSchedule):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            "CosineDecayRestarts is not offered: the index of the running restart is the floor of a quotient of logarithms, and a device "
            "libm and a host libm can round that quotient to different sides of an integer at every restart step — the rate a replayed "
            "batch trains with could then differ from the rate the host reports by a whole restart period's worth")


SCHEDULES = {cls.__name__: cls for cls in (ExponentialDecay, InverseTimeDecay, PolynomialDecay, CosineDecay, PiecewiseConstantDecay,
                                           CosineDecayRestarts)}


def resolve(value):
    """What an optimizer's `learning_rate` may be -> a float (a fixed rate) or a LearningRateSchedule: a number; a schedule object;
    a mapping {name: ExponentialDecay, initial_learning_rate: ..., ...} (experiment files); Keras' {class_name: ..., config: {...}}."""
    if isinstance(value, LearningRateSchedule):
        return value
    if isinstance(value, dict):
        config = dict(value)
        if 'class_name' in config:
            name, config = config['class_name'], dict(config.get('config') or {})
        elif 'name' in config:
            name = config.pop('name')
        else:
            raise ValueError("a learning-rate mapping names its schedule: {{name: ..., <arguments>}} or {{class_name: ..., config: {{...}}}} (got {!r})".format(value))
        if name not in SCHEDULES:
            raise ValueError("no learning-rate schedule '{}': choose one of {}".format(
                name, ', '.join(sorted(n for n in SCHEDULES if n != 'CosineDecayRestarts'))))
        return SCHEDULES[name](**config)
    try:                                                             # (a number, or its text: '1e-4' out of a YAML 1.1 reader)
        if isinstance(value, bool):
            raise TypeError
        return float(value)
    except (TypeError, ValueError):
        raise ValueError("learning_rate must be a number, a LearningRateSchedule or a mapping that names one (got {!r})".format(value)) from None
