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
"""
import ctypes

import numpy as np
import torch

from . import _lib, distributed
from .conv3p_op import _SFX, Conv3pInvalidArgument, _call, _require

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


def momentum_step(params, grads, accums, lr, momentum=0.9):
    """One ApplyMomentum on every (param, grad, accum) triple, in place: one launch per dtype per 16 tensors on the
    current stream.  Tensors are contiguous (a slice of a flat buffer is), float32 or float64, on one HIP device; an
    entry of `grads` may be None: that parameter is left alone (it is updated elsewhere)."""
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
    if not todo:
        return
    lib = _lib.load()
    dev = todo[0][0].device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for dt, (sfx, real, _) in _SFX.items():
            group = [t for t in todo if t[0].dtype == dt]
            for o in range(0, len(group), MAX_TENSORS):
                part = group[o:o + MAX_TENSORS]
                n = len(part)
                tab = [(ctypes.c_void_p * n)(*[t[j].data_ptr() for t in part]) for j in range(3)]
                numels = (ctypes.c_size_t * n)(*[t[0].numel() for t in part])
                _call(getattr(lib, "conv3p_momentum_step_" + sfx), n, ctypes.cast(tab[0], ctypes.c_void_p),
                      ctypes.cast(tab[1], ctypes.c_void_p), ctypes.cast(tab[2], ctypes.c_void_p),
                      ctypes.cast(numels, ctypes.c_void_p), real(lr), real(momentum), stream)


class MomentumOptimizer:
    """tf.train.MomentumOptimizer(learning_rate, momentum) over a list of contiguous HIP tensors.

    learning_rate: a float, or a callable of the global step (e.g. lambda s: exponential_decay(0.001, s, 100000, 0.96)).
    Accumulators are zero-initialised, one per parameter (the reference's "Momentum" slots)."""

    def __init__(self, params, learning_rate, momentum=0.9):
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

    # ------------------------------------------------------------------ helpers
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
    def step(self, grads):
        """minimize()'s update with the gradients in the parameters' order (None: skip that parameter, it was updated
        by fused_fc_step / sharded_step).  The learning rate is the schedule at the step count BEFORE the increment."""
        momentum_step(self.params, grads, self.accums, self.learning_rate(), self.momentum)
        self.global_step += 1

    def sharded_step(self, param, grad, group=None):
        """Data-parallel update of one LARGE parameter (the head's fc1): distributed.reduce_scatter_grad, the kernel on
        this rank's [lo, hi) slice -- its accumulator holds that slice only, 1/world of the parameter -- then
        distributed.all_gather_param.  Without a process group the slice is the whole tensor and the accumulator is
        the one step() uses.  Uses the current global step's learning rate and does not advance it: call step()
        (with None for this parameter) once per training step."""
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
        momentum_step([mine], [g.contiguous()], [acc], self.learning_rate(), self.momentum)
        return distributed.all_gather_param(param, mine, group)

    def fused_fc_step(self, x, W, b, y, dy, selu=True, need_dx=True):
        """fully_connected_grad and this optimizer's update of W (and b) as one pass (conv3p_fc_backward_step_f32): W, b
        and their accumulators are updated in place, dW and db are never written; returns dx (from the OLD W) or None.
        Bit-equal to head.fully_connected_grad followed by step().  Does not advance the global step."""
        from .head import _check_fc, _workspace
        from .conv3p_op import _check_device
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
            ws = _workspace(dev, need)
            _call(lib.conv3p_fc_backward_step_f32, x.data_ptr(), W.data_ptr(), b.data_ptr() if b is not None else None,
                  y.data_ptr(), dy.data_ptr(), M, K, N, 1 if selu else 0, dx.data_ptr() if dx is not None else None,
                  self.accums[iw].data_ptr(), self.accums[ib].data_ptr() if ib is not None else None,
                  ctypes.c_float(self.learning_rate()), ctypes.c_float(self.momentum), ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream(dev).cuda_stream)
        return dx

    def state_dict(self):
        """What the reference's Saver snapshots of the optimizer: the Momentum slots and the global step."""
        return {"global_step": int(self.global_step), "momentum": self.momentum,
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
        self.global_step = int(state["global_step"])
