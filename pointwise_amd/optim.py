"""The optimizer of the reference's three training drivers, on fused HIP kernels.

train_modelnet40_acsd.py:78-82 (scene_seg/train_scene_seg_s3dis.py:80-83, train_scene_seg_scenenn.py:83-86)
    learning_rate = tf.train.exponential_decay(start_learning_rate, global_step, decay_steps, decay_rate, staircase=True)
    optimizer     = tf.train.MomentumOptimizer(learning_rate, momentum)
    train_op      = optimizer.minimize(loss, global_step=global_step)
with param.json's 0.001, 0.9, 100000, 0.96.  MomentumOptimizer is TensorFlow's non-Nesterov ApplyMomentum, in place:

    accum = accum * momentum + grad
    param = param - accum * lr

conv3p_momentum_step_f32 / _f64 (include/conv3p.h, csrc/conv3p_optim.hpp) apply it to up to 16 tensors per launch, each
statement as two separately rounded operations: bit-equal to numpy's `a * m + g` and `w - a * lr` in the parameter's
dtype.  conv3p_fc_backward_step_f32 folds the update of the classification head's fc1 (151 MB) into the pass that
produces its gradient.  The schedule is a host computation in float32, as the TF1 op.  Nothing here synchronises.

The rest of the call: use_nesterov (TensorFlow's ApplyMomentum with use_nesterov), clip_norm (the tf.clip_by_global_norm
a TF1 driver puts between compute_gradients and apply_gradients) and skip_nonfinite (a step whose gradients hold a NaN
or an Inf changes nothing).  grad_sumsq finds {sum of squares, non-finite elements} of the gradients on the device
(conv3p_grad_norm_*), conv3p_momentum_step_guarded_* reads them on the device: a bad batch costs one step and the host
never waits to learn of it (csrc/conv3p_optim_guarded.hpp).  Only last_grad_norm() synchronises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, distributed
from ._host import _HEADS, _SFX, Conv3pInvalidArgument, _call, _check_device, _require, _workspace

MAX_TENSORS = _lib.OPT_MAX_TENSORS


def exponential_decay(start, global_step, decay_steps, decay_rate, staircase=True):
    """tf.train.exponential_decay on the host, in float32 as the TF1 op (its inputs are cast to the learning rate's
    dtype): start * decay_rate ** (global_step / decay_steps), the exponent floored when staircase.  Returns a Python
    float holding the float32 value."""
    _require(decay_steps > 0, "exponential_decay: decay_steps must be positive")
    _require(global_step >= 0, "exponential_decay: global_step must not be negative")
    if staircase:
        p = np.float32(int(global_step) // int(decay_steps))
    else:
        p = np.float32(global_step) / np.float32(decay_steps)
    return float(np.float32(start) * np.power(np.float32(decay_rate), p, dtype=np.float32))


def _check_tensor(t, what):
    _require(isinstance(t, torch.Tensor), "MomentumOptimizer: %s must be a tensor" % what)
    if t.dtype not in _SFX:
        raise Conv3pInvalidArgument("MomentumOptimizer: %s must be float32 or float64" % what)
    _require(t.is_contiguous(), "MomentumOptimizer: %s must be contiguous" % what)


def _check_clip_norm(clip_norm):
    if clip_norm is None:
        return None
    _require(isinstance(clip_norm, (int, float, np.floating, np.integer)) and not isinstance(clip_norm, bool) and
             math.isfinite(clip_norm) and clip_norm > 0,
             "MomentumOptimizer: clip_norm must be a positive finite number or None")
    return float(clip_norm)


def _check_stats(stats, dev):
    _require(isinstance(stats, torch.Tensor) and stats.dtype == torch.float64 and stats.dim() == 1 and stats.numel() == 2
             and stats.is_contiguous(), "MomentumOptimizer: stats must be a contiguous float64 tensor of two values")
    _require(dev is None or stats.device == dev, "MomentumOptimizer: stats must be on the parameters' device")


def _tables(part, cols):
    """The host arrays of one launch: a pointer table per column of `part` and the element counts."""
    n = len(part)
    tabs = [(ctypes.c_void_p * n)(*[t[j].data_ptr() for t in part]) for j in range(cols)]
    return tabs, (ctypes.c_size_t * n)(*[t[0].numel() for t in part])


def _vp(array):
    return ctypes.cast(array, ctypes.c_void_p)


def grad_sumsq(grads, out=None, accumulate=False):
    """-> a device float64 tensor of two values, {sum of every gradient element squared, number of elements that are NaN
    or +-Inf} (such an element adds nothing to the sum): what clip_norm and skip_nonfinite decide from.  One launch pair
    per dtype per 16 tensors on the current stream, chained in stream order; None entries are skipped.  Does not
    synchronise.  out: where to write; accumulate=True adds to what `out` holds (several calls, or the ranks of a
    data-parallel run after an all-reduce of the two values, make one norm).  Equal arguments give equal bits."""
    todo = [(g,) for g in grads if g is not None]
    for (g,) in todo:
        _check_tensor(g, "gradient")
    for (g,) in todo:
        _require(g.device.type == "cuda", "MomentumOptimizer: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        _require(g.device == todo[0][0].device, "MomentumOptimizer: all tensors must be on the same device")
    _require(out is not None or not accumulate, "MomentumOptimizer: grad_sumsq(accumulate=True) needs out=")
    _require(out is not None or todo, "MomentumOptimizer: grad_sumsq needs a gradient or out= to know the device")
    if out is not None:
        _check_stats(out, todo[0][0].device if todo else None)
        _require(out.device.type == "cuda", "MomentumOptimizer: tensors must live on a HIP device (no CPU path in pointwise_amd)")
    lib = _lib.load()
    dev = out.device if out is not None else todo[0][0].device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    need = lib.conv3p_grad_norm_workspace_bytes()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = _workspace(dev, need, _HEADS)
        acc = 1 if accumulate else 0
        calls = 0
        for dt, (sfx, _, _) in _SFX.items():
            group = [t for t in todo if t[0].dtype == dt]
            for o in range(0, len(group), MAX_TENSORS):
                part = group[o:o + MAX_TENSORS]
                tabs, numels = _tables(part, 1)
                _call(getattr(lib, "conv3p_grad_norm_" + sfx), len(part), _vp(tabs[0]), _vp(numels), out.data_ptr(), acc,
                      ws.data_ptr(), ws.numel(), stream)
                acc = 1
                calls += 1
        if calls == 0 and not accumulate:
            _call(lib.conv3p_grad_norm_f32, 0, None, None, out.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
    return out


def momentum_step(params, grads, accums, lr, momentum=0.9, use_nesterov=False, clip_norm=None, skip_nonfinite=False,
                  stats=None):
    """One ApplyMomentum on every (param, grad, accum) triple, in place: one launch per dtype per 16 tensors on the
    current stream.  Tensors are contiguous (a slice of a flat buffer is), float32 or float64, on one HIP device; an
    entry of `grads` may be None: that parameter is left alone (it is updated elsewhere).

    use_nesterov: TensorFlow's rule, accum = accum * m + g; param -= g * lr + accum * m * lr.  clip_norm: every gradient
    is multiplied by clip_norm / max(global norm, clip_norm) first (tf.clip_by_global_norm).  skip_nonfinite: nothing is
    changed when a gradient holds a NaN or an Inf.  Both read `stats` (grad_sumsq's two values) on the device; None
    computes them here over the gradients being applied.  Returns the stats that were used (None when none were).
    With the defaults this launches exactly what it launched before these arguments existed."""
    clip_norm = _check_clip_norm(clip_norm)
    guarded = clip_norm is not None or bool(skip_nonfinite)
    params, grads, accums = list(params), list(grads), list(accums)
    _require(len(grads) == len(params) and len(accums) == len(params),
             "MomentumOptimizer expects one gradient per parameter (%d parameters, %d gradients)" % (len(params), len(grads)))
    todo = [(p, g, a) for p, g, a in zip(params, grads, accums) if g is not None]
    for i, (p, g, a) in enumerate(todo):
        _check_tensor(p, "parameter")
        _check_tensor(g, "gradient")
        _check_tensor(a, "accumulator")
        _require(g.dtype == p.dtype and a.dtype == p.dtype,
                 "MomentumOptimizer expects a parameter, its gradient and its accumulator to have the same dtype")
        _require(tuple(g.shape) == tuple(p.shape) and a.numel() == p.numel(),
                 "MomentumOptimizer expects a parameter and its gradient to have the same shape")
    for p, g, a in todo:
        _require(p.device.type == "cuda" and g.device.type == "cuda" and a.device.type == "cuda",
                 "MomentumOptimizer: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        _require(g.device == p.device and a.device == p.device and p.device == todo[0][0].device,
                 "MomentumOptimizer: all tensors must be on the same device")
    if stats is not None:
        _check_stats(stats, todo[0][0].device if todo else None)
    if clip_norm is not None:
        for p, _, _ in todo:
            c = _SFX[p.dtype][1](clip_norm).value
            _require(math.isfinite(c) and c > 0, "MomentumOptimizer: clip_norm must be a positive finite number in the "
                     "parameters' dtype")
    if not todo:
        return stats if guarded else None
    if guarded and stats is None:
        stats = grad_sumsq([t[1] for t in todo])
    lib = _lib.load()
    dev = todo[0][0].device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for dt, (sfx, real, _) in _SFX.items():
            group = [t for t in todo if t[0].dtype == dt]
            for o in range(0, len(group), MAX_TENSORS):
                part = group[o:o + MAX_TENSORS]
                tabs, numels = _tables(part, 3)
                if guarded or use_nesterov:
                    _call(getattr(lib, "conv3p_momentum_step_guarded_" + sfx), len(part), _vp(tabs[0]), _vp(tabs[1]), _vp(tabs[2]), _vp(numels),
                          real(lr), real(momentum), 1 if use_nesterov else 0, real(clip_norm or 0.0),
                          1 if skip_nonfinite else 0, stats.data_ptr() if guarded else None, stream)
                else:
                    _call(getattr(lib, "conv3p_momentum_step_" + sfx), len(part), _vp(tabs[0]), _vp(tabs[1]), _vp(tabs[2]), _vp(numels),
                          real(lr), real(momentum), stream)
    return stats if guarded else None


class MomentumOptimizer:
    """tf.train.MomentumOptimizer(learning_rate, momentum) over a list of contiguous HIP tensors.

    learning_rate: a float, or a callable of the global step (e.g. lambda s: exponential_decay(0.001, s, 100000, 0.96)).
    Accumulators are zero-initialised, one per parameter (the reference's "Momentum" slots).

    use_nesterov, clip_norm (a positive number: tf.clip_by_global_norm over the gradients of a step) and skip_nonfinite
    (a step whose gradients hold a NaN or an Inf changes no parameter and no accumulator) are decided on the device
    from grad_sumsq's two values; the host does not learn what happened unless it asks (last_grad_norm(),
    skipped_steps).  An optimizer with any of them is not `fusable`: the global norm exists only once every gradient
    does, so fused_fc_step and the classification tail's _step form -- which update inside the pass that produces the
    gradient -- refuse it, and ClassificationHead writes its gradients for step() instead."""

    def __init__(self, params, learning_rate, momentum=0.9, use_nesterov=False, clip_norm=None, skip_nonfinite=False):
        self.clip_norm = _check_clip_norm(clip_norm)
        self.use_nesterov = bool(use_nesterov)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.params = list(params)
        for p in self.params:
            _check_tensor(p, "parameter")
        for p in self.params:
            _require(p.device.type == "cuda",
                     "MomentumOptimizer: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        _require(callable(learning_rate) or isinstance(learning_rate, (int, float)),
                 "MomentumOptimizer: learning_rate must be a number or a callable of the global step")
        self._lr = learning_rate
        self.momentum = float(momentum)
        self.accums = [torch.zeros_like(p) for p in self.params]
        self._shards = {}              # parameter index -> (lo, hi, accumulator of this rank's slice), sharded_step()
        self.global_step = 0
        self.grad_stats = None         # the last step's {sum of squares, non-finite elements}: a device float64[2]
        # steps the device skipped: a device int64 scalar, advanced on the stream (reading it synchronises)
        self.skipped_steps = torch.zeros((), dtype=torch.int64, device=self.params[0].device if self.params else "cpu")

    # ------------------------------------------------------------------ helpers
    @property
    def fusable(self):
        """True when the update may run inside the pass that produces a gradient (fused_fc_step, the tail's _step
        form): the plain rule, no clipping, no skipping."""
        return not (self.use_nesterov or self.clip_norm is not None or self.skip_nonfinite)

    def _guarded(self):
        return self.clip_norm is not None or self.skip_nonfinite

    def _settings(self):
        return dict(use_nesterov=self.use_nesterov, clip_norm=self.clip_norm, skip_nonfinite=self.skip_nonfinite)

    def learning_rate(self, step=None):
        """The learning rate of `step` (default: the current global step), a float32 value as a Python float."""
        s = self.global_step if step is None else step
        lr = self._lr(s) if callable(self._lr) else self._lr
        return float(np.float32(lr))

    def _index(self, t, what):
        for i, p in enumerate(self.params):
            if p is t:
                return i
        raise Conv3pInvalidArgument("MomentumOptimizer: %s is not one of this optimizer's parameters" % what)

    def owns(self, *tensors):
        return all(any(p is t for p in self.params) for t in tensors)

    # ------------------------------------------------------------------ public
    def step(self, grads, stats=None):
        """minimize()'s update with the gradients in the parameters' order (None: skip that parameter, it was updated
        by fused_fc_step / sharded_step).  The learning rate is the schedule at the step count BEFORE the increment.

        With clip_norm or skip_nonfinite the norm is that of exactly the gradients given here (grad_sumsq), unless
        `stats` is given: a data-parallel caller computes grad_sumsq itself, all-reduces the two values (SUM) and hands
        them in, as SegmentationHead.weight_total() / denominator=.  The stats used stay in .grad_stats; skipped_steps
        is advanced on the device.  global_step advances whether or not the device skipped: the host does not know."""
        used = momentum_step(self.params, grads, self.accums, self.learning_rate(), self.momentum, stats=stats,
                             **self._settings())
        if used is not None:
            self.grad_stats = used
            if self.skip_nonfinite:
                self.skipped_steps += (used[1] > 0).to(self.skipped_steps.device)
        self.global_step += 1

    def last_grad_norm(self):
        """SYNCHRONISES (a device-to-host copy of .grad_stats): -> (global norm of the last step's finite gradient
        elements, number of non-finite elements).  For logging every so often, not for every step."""
        _require(self.grad_stats is not None, "MomentumOptimizer: no step with clip_norm / skip_nonfinite yet")
        sumsq, bad = self.grad_stats.cpu().tolist()
        return math.sqrt(sumsq) if sumsq >= 0 else float("nan"), int(bad)

    def sharded_step(self, param, grad, group=None, stats=None):
        """Data-parallel update of one LARGE parameter (the head's fc1): distributed.reduce_scatter_grad, the kernel on
        this rank's [lo, hi) slice -- its accumulator holds that slice only, 1/world of the parameter -- then
        distributed.all_gather_param.  Without a process group the slice is the whole tensor and the accumulator is
        the one step() uses.  Uses the current global step's learning rate and does not advance it: call step()
        (with None for this parameter) once per training step.

        With clip_norm or skip_nonfinite: `stats` as in step(); None takes grad_sumsq of this rank's reduced slice alone,
        which is the global norm only without a process group.  skipped_steps is step()'s to count."""
        i = self._index(param, "param")
        _check_tensor(grad, "gradient")
        _require(grad.dtype == param.dtype and tuple(grad.shape) == tuple(param.shape),
                 "MomentumOptimizer expects a parameter and its gradient to have the same shape")
        g, lo, hi = distributed.reduce_scatter_grad(grad, group)
        flat = param.reshape(-1)
        if lo == 0 and hi == flat.numel():
            acc = self.accums[i].reshape(-1)
        else:
            sh = self._shards.get(i)
            if sh is None or sh[0] != lo or sh[1] != hi:
                sh = (lo, hi, torch.zeros(hi - lo, dtype=param.dtype, device=param.device))
                self._shards[i] = sh
                self.accums[i] = self.accums[i].new_empty(0)       # the full-size accumulator is not kept
            acc = sh[2]
        mine = flat[lo:hi]
        used = momentum_step([mine], [g.contiguous()], [acc], self.learning_rate(), self.momentum, stats=stats,
                             **self._settings())
        if used is not None:
            self.grad_stats = used
        return distributed.all_gather_param(param, mine, group)

    def fused_fc_step(self, x, W, b, y, dy, selu=True, need_dx=True):
        """fully_connected_grad and this optimizer's update of W (and b) as one pass (conv3p_fc_backward_step_f32): W, b
        and their accumulators are updated in place, dW and db are never written; returns dx (from the OLD W) or None.
        Bit-equal to head.fully_connected_grad followed by step().  Does not advance the global step."""
        from .head import _check_fc
        _require(self.fusable, "MomentumOptimizer: fused_fc_step applies the plain rule inside the gradient pass; with "
                 "use_nesterov, clip_norm or skip_nonfinite use fully_connected_grad and step()")
        lib = _lib.load()
        _check_fc(x, W, b)
        iw = self._index(W, "W")
        ib = self._index(b, "b") if b is not None else None
        _require(x.is_contiguous() and y.is_contiguous() and dy.is_contiguous(),
                 "MomentumOptimizer: fused_fc_step expects contiguous tensors")
        _require(self.accums[iw].numel() == W.numel(), "MomentumOptimizer: W's accumulator is sharded")
        dev = _check_device(x, W, y, dy)
        M, K = x.shape
        N = W.shape[1]
        dx = torch.empty_like(x) if need_dx else None
        need = lib.conv3p_fc_workspace_bytes(M, K, N)
        with torch.cuda.device(dev):
            ws = _workspace(dev, need, _HEADS)
            _call(lib.conv3p_fc_backward_step_f32, x.data_ptr(), W.data_ptr(), b.data_ptr() if b is not None else None,
                  y.data_ptr(), dy.data_ptr(), M, K, N, 1 if selu else 0, dx.data_ptr() if dx is not None else None,
                  self.accums[iw].data_ptr(), self.accums[ib].data_ptr() if ib is not None else None,
                  ctypes.c_float(self.learning_rate()), ctypes.c_float(self.momentum), ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream(dev).cuda_stream)
        return dx

    def state_dict(self):
        """What the reference's Saver snapshots of the optimizer: the Momentum slots and the global step; and the three
        settings of the guarded step with the count of skipped steps."""
        return {"global_step": int(self.global_step), "momentum": self.momentum, "use_nesterov": self.use_nesterov,
                "clip_norm": self.clip_norm, "skip_nonfinite": self.skip_nonfinite,
                "skipped_steps": self.skipped_steps.clone(),
                "accumulators": [a.clone() for a in self.accums],
                "shards": {i: (lo, hi, a.clone()) for i, (lo, hi, a) in self._shards.items()}}

    def load_state_dict(self, state):
        accs = state["accumulators"]
        _require(len(accs) == len(self.params),
                 "MomentumOptimizer expects one accumulator per parameter (%d parameters, %d accumulators)"
                 % (len(self.params), len(accs)))
        shards = state.get("shards", {})
        for i, (p, a) in enumerate(zip(self.params, accs)):
            _require(a.dtype == p.dtype and (a.numel() == p.numel() or (a.numel() == 0 and i in shards)),
                     "MomentumOptimizer expects a parameter and its accumulator to have the same dtype and size")
        self.accums = [a.to(p.device).reshape(p.shape).clone() if a.numel() else a.to(p.device).clone()
                       for p, a in zip(self.params, accs)]
        self._shards = {int(i): (int(lo), int(hi), a.to(self.params[int(i)].device).clone())
                        for i, (lo, hi, a) in shards.items()}
        self.momentum = float(state.get("momentum", self.momentum))
        # a dictionary written before these settings existed leaves them as constructed and has skipped nothing
        clip = _check_clip_norm(state.get("clip_norm", self.clip_norm))
        self.use_nesterov = bool(state.get("use_nesterov", self.use_nesterov))
        self.clip_norm = clip
        self.skip_nonfinite = bool(state.get("skip_nonfinite", self.skip_nonfinite))
        skipped = state.get("skipped_steps", 0)
        self.skipped_steps = torch.as_tensor(skipped, dtype=torch.int64).reshape(()).to(self.skipped_steps.device).clone()
        self.global_step = int(state["global_step"])
