"""float64 numpy restatement of the learning-rate schedules of include/amar_hip.h, written from the header's formulas; no torch, no
device, and nothing of deep_cbrs_amar_renaissance_amd/utilities/schedules.py.  tests/test_lr_schedules_cpu.py pins it by hand.

Every function takes the zero-based steps as an array and returns float64; `as_float32` rounds parameters the way the device receives
them (the kernels compute in double from float32 members), `rate32` rounds a result once to float32 as the kernels do."""
import numpy as np


def as_float32(*values):
    out = tuple(float(np.float32(v)) if np.ndim(v) == 0 else [float(np.float32(x)) for x in v] for v in values)
    return out[0] if len(out) == 1 else out


def rate32(rates):
    return np.asarray(rates, dtype=np.float64).astype(np.float32)


def _steps(steps):
    return np.atleast_1d(np.asarray(steps, dtype=np.float64))


def exponential(steps, lr0, decay_steps, decay_rate, staircase=False):
    p = _steps(steps) / decay_steps
    if staircase:
        p = np.floor(p)
    return lr0 * np.power(decay_rate, p)


def inverse_time(steps, lr0, decay_steps, decay_rate, staircase=False):
    p = _steps(steps) / decay_steps
    if staircase:
        p = np.floor(p)
    return lr0 / (1.0 + decay_rate * p)


def polynomial(steps, lr0, decay_steps, end=1e-4, power=1.0, cycle=False):
    s = _steps(steps)
    if cycle:
        p = s / (decay_steps * np.where(s == 0, 1.0, np.ceil(s / decay_steps)))
    else:
        p = np.minimum(s, decay_steps) / decay_steps
    return (lr0 - end) * np.power(1.0 - p, power) + end


def cosine(steps, lr0, decay_steps, alpha=0.0):
    s = _steps(steps)
    return lr0 * ((1.0 - alpha) * 0.5 * (1.0 + np.cos(np.pi * (np.minimum(s, decay_steps) / decay_steps))) + alpha)


def piecewise(steps, boundaries, values):
    s = _steps(steps)
    index = np.searchsorted(np.asarray(boundaries, dtype=np.float64), s, side='left')   # the first i with s <= b[i], or len(b)
    return np.asarray(values, dtype=np.float64)[index]


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at want (both float32 arrays)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
