"""numpy restatement of the guarded optimizer step (pointwise_amd/optim.py, csrc/conv3p_optim_guarded.hpp): the scale of
tf.clip_by_global_norm and both forms of TensorFlow's ApplyMomentum, in the parameter's dtype.  Every operation is a
numpy statement of its own, so every product and sum is rounded separately -- the contract of the device kernels.

    scale  = dtype(clip_norm / max(sqrt(sumsq), clip_norm))      sqrt and division in float64, one rounding to dtype;
                                                                  0 when sumsq is not finite, 1 without clipping
    g'     = g * scale
    plain     accum = accum * m + g';  param = param - accum * lr
    nesterov  accum = accum * m + g';  param = param - (g' * lr + (accum * m) * lr)
"""
import math

import numpy as np


def clip_scale_ref(sumsq, clip_norm, dtype):
    """The factor every gradient is multiplied with, a scalar of `dtype`.  sumsq: the float64 sum of squares; clip_norm
    None (or <= 0): no clipping."""
    dt = np.dtype(dtype).type
    if clip_norm is None or not clip_norm > 0:
        return dt(1)
    sumsq = np.float64(sumsq)
    if not np.isfinite(sumsq):
        return dt(0)
    c = np.float64(dt(clip_norm))                  # the kernel receives clip_norm in the parameter's dtype
    norm = np.sqrt(sumsq)
    den = norm if norm > c else c
    q = c / den
    return dt(q)


def guarded_step_ref(param, grad, accum, lr, momentum, nesterov=False, scale=None):
    """-> (new param, new accum).  scale: clip_scale_ref's value, None for a step without clipping (no multiply)."""
    dt = param.dtype.type
    assert grad.dtype == param.dtype and accum.dtype == param.dtype
    lr, m = dt(lr), dt(momentum)
    with np.errstate(all="ignore"):
        g = grad
        if scale is not None:
            g = grad * dt(scale)
        am = accum * m
        a = am + g
        if nesterov:
            glr = g * lr
            am2 = a * m
            amlr = am2 * lr
            upd = glr + amlr
            w = param - upd
        else:
            alr = a * lr
            w = param - alr
    assert a.dtype == param.dtype and w.dtype == param.dtype
    return w, a


def sumsq_ref(arrays):
    """(exact sum of the finite elements' float64 squares, rounded once; number of non-finite elements).  The squares
    of float32 values are exact in float64; those of float64 values carry one rounding each."""
    terms, bad = [], 0
    for a in arrays:
        a = np.asarray(a).reshape(-1)
        ok = np.isfinite(a)
        bad += int((~ok).sum())
        d = a[ok].astype(np.float64)
        terms.append(d * d)
    return math.fsum(np.concatenate(terms).tolist()) if terms else 0.0, bad
