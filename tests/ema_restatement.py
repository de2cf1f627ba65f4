"""Float64 restatement of the weight average (fastvision_amd.ModelEMA / fva_ema_update), for tests/test_ema_cpu.py and
tests/test_gpu_ema.py: the ramp, one update, the recurrence over several updates, and the error bound of the fp32 kernel.

The kernel computes, per fp32 element,  e' = fmaf(w, p - e, e)  with w = (float)(1 - d): one fp32 subtraction (rounded once, relative
error <= 2^-24) and one fused multiply-add (rounded once, error <= half an ulp of the result).  Against the float64 value
ref = w * (p - e) + e of the same fp32 inputs and the same fp32 weight that gives

    |gpu - ref| <= 0.5 * ulp32(ref) + w * 2^-24 * |p - e|

(the float64 arithmetic itself errs by ~2^-53 relative: nothing beside 2^-25).  Over several updates the error obeys
err' <= (1 - w) * err + bound, so with 0 <= w <= 1 it is at most the sum of the per-step bounds."""
import math

import numpy as np

DECAY, TAU = 0.9999, 2000.0


def weight(k, decay=DECAY, tau=TAU):
    """w = 1 - d of update number k (1-based): d = decay * (1 - exp(-k / tau)), the ramp that lets a young average follow the model;
    d = decay when tau == 0."""
    d = decay * (1.0 - math.exp(-k / tau)) if tau > 0 else decay
    return 1.0 - d


def w32(w):
    """The weight as the chunk kernel reads it: the double rounded to fp32 (returned as a float64 number)."""
    return float(np.float32(w))


def step(e, p, w):
    """One update in float64 from fp32 (or float64) operands; ``w`` is used as given (pass w32(...) for the kernel's weight)."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return w * (p - e) + e


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (2^-149 below the normal range; 0 at 0: an exact zero must come out exact)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    ex = np.frexp(a)[1].astype(np.int64) - 1            # a = m * 2^(ex + 1), m in [0.5, 1): floor(log2 a), exactly
    u = np.ldexp(1.0, np.maximum(ex - 23, -149))
    return np.where(a > 0, u, 0.0)


def step_bound(ref, e, p, w):
    """Bound on |fp32 kernel result - ref| for one update (see the module docstring)."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return 0.5 * ulp32(ref) + w * 2.0 ** -24 * np.abs(p - e)


def follow(e0, ps, ws):
    """The recurrence in float64: yields (ref_t, bound_t) after each update t, from the fp32 start e0, the fp32 model values ps[t]
    (a callable ps[t](ref) may derive p from the current reference, e.g. p = e) and the weights ws[t]."""
    ref = np.asarray(e0, dtype=np.float64)
    for p, w in zip(ps, ws):
        p = np.asarray(p, dtype=np.float64)
        new = step(ref, p, w)
        yield new, step_bound(new, ref, p, w)
        ref = new
