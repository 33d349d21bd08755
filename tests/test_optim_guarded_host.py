"""Host-side tests of the guarded optimizer step (no GPU): the exported symbols and their status codes, argument
validation, the state dictionary, and the numpy restatement's own consistency."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op, optim
from tests.optim_guarded_ref import clip_scale_ref, guarded_step_ref, sumsq_ref
from tests.optim_ref import momentum_step_ref

NEW = ("conv3p_grad_norm_workspace_bytes", "conv3p_grad_norm_f32", "conv3p_grad_norm_f64",
       "conv3p_momentum_step_guarded_f32", "conv3p_momentum_step_guarded_f64")


def test_library_exports_the_new_symbols():
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    assert lib.conv3p_abi_version() == _lib.ABI_VERSION == 5               # additions do not move the version
    assert lib.conv3p_profile_kinds() == 20                                 # ... nor the table of profile kinds
    assert lib.conv3p_grad_norm_workspace_bytes() >= 2048 * 16             # one record per workgroup of the largest grid
    import pointwise_amd
    assert optim.grad_sumsq is not None and pointwise_amd.MomentumOptimizer is optim.MomentumOptimizer


def test_grad_norm_status_codes_before_any_launch():
    """Decided before a HIP call: bogus (never dereferenced) device pointers are fine."""
    lib = _lib.load()
    need = lib.conv3p_grad_norm_workspace_bytes()
    p = ctypes.c_void_p(256)
    for fn, esz in ((lib.conv3p_grad_norm_f32, 4), (lib.conv3p_grad_norm_f64, 8)):
        def call(n, grads, numels, stats=p, acc=0, ws=p, wsb=need, arrays=(True, True)):
            tab = (ctypes.c_void_p * max(len(grads), 1))(*grads)
            ne = (ctypes.c_size_t * max(len(numels), 1))(*numels)
            a = [ctypes.cast(t, ctypes.c_void_p) if keep else None for t, keep in zip((tab, ne), arrays)]
            return fn(n, a[0], a[1], stats, acc, ws, wsb, None)
        assert call(-1, [256], [1]) == _lib.ERR_INVALID_ARGUMENT
        assert call(17, [256] * 17, [0] * 17) == _lib.ERR_INVALID_ARGUMENT
        assert call(1, [256], [0], stats=None) == _lib.ERR_INVALID_ARGUMENT
        assert call(2, [256, 512], [0, 0], arrays=(False, True)) == _lib.ERR_INVALID_ARGUMENT
        assert call(2, [256, 512], [0, 0], arrays=(True, False)) == _lib.ERR_INVALID_ARGUMENT
        assert call(2, [256, None], [0, 5]) == _lib.ERR_INVALID_ARGUMENT            # a NULL entry with a count
        for bad in (1, 2, esz // 2, esz - 1):
            assert call(2, [256, 512 + bad], [0, 5]) == _lib.ERR_INVALID_ARGUMENT, bad
        assert call(1, [256], [5], ws=None) == _lib.ERR_WORKSPACE
        assert call(1, [256], [5], wsb=need - 1) == _lib.ERR_WORKSPACE
        assert call(1, [256], [5], ws=ctypes.c_void_p(264)) == _lib.ERR_WORKSPACE
        # nothing to read and accumulate: nothing is launched, so this is safe without a device
        assert call(0, [], [], acc=1, arrays=(False, False)) == _lib.OK
        assert call(3, [None] * 3, [0] * 3, acc=1, ws=None, wsb=0) == _lib.OK


def test_guarded_step_status_codes_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    for fn, plain, real in ((lib.conv3p_momentum_step_guarded_f32, lib.conv3p_momentum_step_f32, ctypes.c_float),
                            (lib.conv3p_momentum_step_guarded_f64, lib.conv3p_momentum_step_f64, ctypes.c_double)):
        def call(n, ptrs, numels, nesterov=0, clip=0.0, skip=0, stats=None, arrays=True):
            tabs = [ctypes.cast((ctypes.c_void_p * max(len(ptrs), 1))(*ptrs), ctypes.c_void_p) for _ in range(3)]
            ne = ctypes.cast((ctypes.c_size_t * max(len(numels), 1))(*numels), ctypes.c_void_p)
            if not arrays:
                tabs, ne = [None] * 3, None
            return fn(n, tabs[0], tabs[1], tabs[2], ne, real(0.001), real(0.9), nesterov, real(clip), skip, stats, None)
        zero3 = ([256, 512, 1024], [0, 0, 0])
        # stats == NULL with clipping or skipping
        assert call(3, *zero3, clip=1.0) == _lib.ERR_INVALID_ARGUMENT
        assert call(3, *zero3, skip=1) == _lib.ERR_INVALID_ARGUMENT
        assert call(0, [], [], clip=1.0) == _lib.ERR_INVALID_ARGUMENT
        assert call(3, *zero3, clip=float("inf"), stats=p) == _lib.ERR_INVALID_ARGUMENT
        assert call(3, *zero3, clip=float("nan"), stats=p) == _lib.ERR_INVALID_ARGUMENT
        # ... and every combination that is fine, with all counts zero so that nothing is launched
        for kw in (dict(), dict(nesterov=1), dict(clip=1.0, stats=p), dict(skip=1, stats=p), dict(clip=-1.0),
                   dict(nesterov=1, clip=2.0, skip=1, stats=p), dict(stats=p)):
            assert call(3, *zero3, **kw) == _lib.OK, kw
            assert call(0, [], [], arrays=False, **kw) == _lib.OK, kw
            assert call(-1, *zero3, **kw) == _lib.ERR_INVALID_ARGUMENT and call(17, [256] * 17, [0] * 17, **kw) == \
                _lib.ERR_INVALID_ARGUMENT, kw
            assert call(3, *zero3, arrays=False, **kw) == _lib.ERR_INVALID_ARGUMENT, kw
            assert call(3, [256, None, 1024], [0, 5, 0], **kw) == _lib.ERR_INVALID_ARGUMENT, kw
            assert call(3, [256, 513, 1024], [0, 5, 0], **kw) == _lib.ERR_INVALID_ARGUMENT, kw


def test_optimizer_argument_validation():
    from pointwise_amd.optim import MomentumOptimizer, grad_sumsq, momentum_step
    w, g, a = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3)
    for bad in (0, -1.0, float("inf"), float("nan"), "1", True, [1.0]):
        with pytest.raises(op.Conv3pInvalidArgument, match="clip_norm must be a positive finite number or None"):
            MomentumOptimizer([], 0.1, clip_norm=bad)
        with pytest.raises(op.Conv3pInvalidArgument, match="clip_norm must be a positive finite number or None"):
            momentum_step([w], [g], [a], 0.1, 0.9, clip_norm=bad)
    opt = MomentumOptimizer([], 0.1, 0.9, True, 2, True)                      # the documented positional order
    assert opt.use_nesterov is True and opt.clip_norm == 2.0 and opt.skip_nonfinite is True and opt.fusable is False
    plain = MomentumOptimizer([], 0.1)
    assert plain.fusable is True and plain.use_nesterov is False and plain.clip_norm is None and plain.skip_nonfinite is False
    assert plain.grad_stats is None and plain.skipped_steps.dtype == torch.int64 and int(plain.skipped_steps) == 0
    for kw in (dict(use_nesterov=True), dict(clip_norm=1.0), dict(skip_nonfinite=True)):
        assert MomentumOptimizer([], 0.1, **kw).fusable is False, kw
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        MomentumOptimizer([w], 0.1, clip_norm=1.0)                            # the existing checks still come
    # stats: a contiguous float64 tensor of two values
    for bad in (torch.zeros(2), torch.zeros(3, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)[::2],
                torch.zeros(2, 1, dtype=torch.float64), [0.0, 0.0]):
        with pytest.raises(op.Conv3pInvalidArgument, match="stats must be a contiguous float64 tensor of two values"):
            opt.step([], stats=bad)
        with pytest.raises(op.Conv3pInvalidArgument, match="stats must be a contiguous float64 tensor of two values"):
            momentum_step([], [], [], 0.1, 0.9, skip_nonfinite=True, stats=bad)
        with pytest.raises(op.Conv3pInvalidArgument, match="stats must be a contiguous float64 tensor of two values"):
            grad_sumsq([], out=bad)
    assert opt.global_step == 0                                               # a refused step does not count
    opt.step([], stats=torch.zeros(2, dtype=torch.float64))                   # nothing to update: nothing launched
    opt.step([])
    assert opt.global_step == 2 and int(opt.skipped_steps) == 0
    with pytest.raises(op.Conv3pInvalidArgument, match="no step with clip_norm / skip_nonfinite yet"):
        plain.last_grad_norm()
    # grad_sumsq
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        grad_sumsq([g])
    with pytest.raises(op.Conv3pInvalidArgument, match="float32 or float64"):
        grad_sumsq([g.half()])
    with pytest.raises(op.Conv3pInvalidArgument, match="gradient must be contiguous"):
        grad_sumsq([g.t()])
    with pytest.raises(op.Conv3pInvalidArgument, match="must be a tensor"):
        grad_sumsq([np.zeros(3)])
    with pytest.raises(op.Conv3pInvalidArgument, match="needs out="):
        grad_sumsq([], accumulate=True)
    with pytest.raises(op.Conv3pInvalidArgument, match="needs a gradient or out="):
        grad_sumsq([None, None])
    # the fused epilogue refuses an optimizer that has to see every gradient first
    with pytest.raises(op.Conv3pInvalidArgument, match="fused_fc_step applies the plain rule"):
        opt.fused_fc_step(torch.zeros(2, 4), torch.zeros(4, 8), None, torch.zeros(2, 8), torch.zeros(2, 8))


def test_state_dict_round_trip_and_the_earlier_format():
    from pointwise_amd.optim import MomentumOptimizer
    opt = MomentumOptimizer([], 0.1, momentum=0.8, use_nesterov=True, clip_norm=2.5, skip_nonfinite=True)
    opt.step([])
    opt.skipped_steps += 3
    sd = opt.state_dict()
    assert sd["use_nesterov"] is True and sd["clip_norm"] == 2.5 and sd["skip_nonfinite"] is True
    assert int(sd["skipped_steps"]) == 3 and sd["global_step"] == 1 and sd["momentum"] == 0.8
    opt.skipped_steps += 1
    assert int(sd["skipped_steps"]) == 3                                      # a copy, not the live counter
    other = MomentumOptimizer([], 0.1)
    other.load_state_dict(sd)
    assert (other.use_nesterov, other.clip_norm, other.skip_nonfinite) == (True, 2.5, True) and not other.fusable
    assert int(other.skipped_steps) == 3 and other.skipped_steps.dtype == torch.int64 and other.global_step == 1
    # a dictionary as written before these settings existed: exactly these four keys
    old = {"global_step": 7, "momentum": 0.7, "accumulators": [], "shards": {}}
    other.load_state_dict(old)
    assert other.global_step == 7 and other.momentum == 0.7
    assert (other.use_nesterov, other.clip_norm, other.skip_nonfinite) == (True, 2.5, True)   # left as they were
    assert int(other.skipped_steps) == 0
    fresh = MomentumOptimizer([], 0.1)
    fresh.load_state_dict(old)
    assert fresh.fusable and fresh.global_step == 7
    with pytest.raises(op.Conv3pInvalidArgument, match="clip_norm must be a positive finite number or None"):
        fresh.load_state_dict(dict(old, clip_norm=-1.0))


# --------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_ref_nesterov_without_momentum_is_gradient_descent(dt):
    rng = np.random.default_rng(5)
    w, g, a = (rng.standard_normal(500).astype(dt) for _ in range(3))
    lr = float(np.float32(0.01))
    w1, a1 = guarded_step_ref(w, g, a, lr, 0.0, nesterov=True)
    assert np.array_equal(a1, g + dt(0) * a) and np.array_equal(w1, w - g * dt(lr))
    # ... and the plain rule of this file is the one of tests/optim_ref.py
    for m in (0.0, 0.9):
        w2, a2 = guarded_step_ref(w, g, a, lr, m, nesterov=False)
        w3, a3 = momentum_step_ref(w, g, a, lr, m)
        assert np.array_equal(w2, w3) and np.array_equal(a2, a3)
    # Nesterov differs from the plain rule by the look-ahead: same accumulator, another parameter
    w4, a4 = guarded_step_ref(w, g, a, lr, 0.9, nesterov=True)
    assert np.array_equal(a4, a2) and not np.array_equal(w4, w2)
    assert np.allclose(w4, w - lr * (g + 0.9 * a4), rtol=0, atol=1e-5)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_ref_scale(dt):
    one = dt(1)
    for sumsq, clip in ((0.0, 1.0), (4.0, 2.0), (3.999, 2.0), (1e-30, 1e-3), (1.0, 1e30)):
        s = clip_scale_ref(sumsq, clip, dt)
        assert type(s) is dt and s == one, (sumsq, clip)                      # norm <= clip_norm: exactly 1
    assert clip_scale_ref(16.0, 2.0, dt) == dt(0.5) and clip_scale_ref(16.0, 1.0, dt) == dt(0.25)
    s = clip_scale_ref(10.0, 1.0, dt)
    assert 0 < s < 1 and s == dt(1.0 / np.sqrt(np.float64(10.0)))
    assert clip_scale_ref(np.inf, 1.0, dt) == 0 and clip_scale_ref(np.nan, 1.0, dt) == 0
    assert clip_scale_ref(16.0, None, dt) == one and clip_scale_ref(16.0, 0.0, dt) == one
    # a scale of exactly 1 changes no bit of a step, and a scale rescales the gradient and nothing else
    rng = np.random.default_rng(6)
    w, g, a = (rng.standard_normal(300).astype(dt) for _ in range(3))
    for nest in (False, True):
        w0, a0 = guarded_step_ref(w, g, a, 0.01, 0.9, nesterov=nest)
        w1, a1 = guarded_step_ref(w, g, a, 0.01, 0.9, nesterov=nest, scale=one)
        assert np.array_equal(w0, w1) and np.array_equal(a0, a1)
        w2, a2 = guarded_step_ref(w, g, a, 0.01, 0.9, nesterov=nest, scale=dt(0.5))
        w3, a3 = guarded_step_ref(w, g * dt(0.5), a, 0.01, 0.9, nesterov=nest)
        assert np.array_equal(w2, w3) and np.array_equal(a2, a3)


def test_ref_sumsq():
    a = np.array([3.0, np.inf, -4.0, np.nan, -np.inf], dtype=np.float32)
    assert sumsq_ref([a, a.astype(np.float64)]) == (50.0, 6)
    assert sumsq_ref([]) == (0.0, 0) and sumsq_ref([np.zeros(0, np.float32)]) == (0.0, 0)
