"""numpy restatement of the optimizer the reference's drivers use (train_modelnet40_acsd.py:78-82):
tf.train.MomentumOptimizer under a staircase tf.train.exponential_decay.

ApplyMomentum, non-Nesterov, both statements in the parameter's dtype -- numpy rounds every operation of an expression
separately, which is the contract of the device kernels (no fused multiply-add):

    accum = accum * momentum + grad
    param = param - accum * lr

The schedule is float32 arithmetic on float32 inputs, as the TF1 op computes it.
"""
import numpy as np


def momentum_step_ref(param, grad, accum, lr, momentum):
    """-> (new param, new accum); inputs are arrays of one dtype, lr / momentum are rounded to it first."""
    dt = param.dtype.type
    assert grad.dtype == param.dtype and accum.dtype == param.dtype
    with np.errstate(all="ignore"):
        a = accum * dt(momentum) + grad
        w = param - a * dt(lr)
    assert a.dtype == param.dtype and w.dtype == param.dtype
    return w, a


def exponential_decay_ref(start, global_step, decay_steps, decay_rate, staircase=True):
    f = np.float32
    p = f(global_step // decay_steps) if staircase else f(global_step) / f(decay_steps)
    return float(f(start) * np.power(f(decay_rate), p, dtype=np.float32))


class MomentumRef:
    """The optimizer object on numpy arrays: the same step count / schedule rule as optim.MomentumOptimizer."""

    def __init__(self, params, learning_rate, momentum=0.9):
        self.params = [p.copy() for p in params]
        self.accums = [np.zeros_like(p) for p in params]
        self.lr, self.momentum, self.global_step = learning_rate, momentum, 0

    def step(self, grads):
        lr = self.lr(self.global_step) if callable(self.lr) else self.lr
        lr = float(np.float32(lr))
        for i, g in enumerate(grads):
            if g is not None:
                self.params[i], self.accums[i] = momentum_step_ref(self.params[i], g, self.accums[i], lr, self.momentum)
        self.global_step += 1
