"""CPU tests (not gpu) of the optimizer's host side: the module imports, the C ABI exports and binds the three symbols
without moving the ABI version or the profile-kind table, the status codes that are decided before any HIP call, the
Python argument checks, the learning-rate schedule, the host-only part of state_dict, and the numpy restatement
against a per-element Python loop."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op

from tests.optim_ref import exponential_decay_ref, momentum_step_ref

PARAM_JSON = dict(start=0.001, decay_steps=100000, decay_rate=0.96)       # the reference's param.json; momentum 0.9


def test_module_imports_and_is_exported():
    import pointwise_amd
    from pointwise_amd import optim
    assert pointwise_amd.MomentumOptimizer is optim.MomentumOptimizer
    assert pointwise_amd.exponential_decay is optim.exponential_decay
    assert pointwise_amd.momentum_step is optim.momentum_step
    assert {"MomentumOptimizer", "exponential_decay", "momentum_step"} <= set(pointwise_amd.__all__)
    assert optim.MAX_TENSORS == _lib.OPT_MAX_TENSORS == 16


def test_symbols_are_bound_and_nothing_pinned_moved():
    lib = _lib.load()
    for n in ("conv3p_momentum_step_f32", "conv3p_momentum_step_f64", "conv3p_fc_backward_step_f32"):
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    assert lib.conv3p_abi_version() == _lib.ABI_VERSION == 5
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert names[-1] == "seg_head_kernel" and len(names) == 20               # no profile kind was added
    assert names.index("fc_dw_kernel") == 14 and names.index("fc_dx_kernel") == 13


def test_momentum_step_status_codes_before_any_launch():
    """Everything here is decided before a HIP call: bogus (never dereferenced) device pointers are fine."""
    lib = _lib.load()
    for fn, real, esz in ((lib.conv3p_momentum_step_f32, ctypes.c_float, 4), (lib.conv3p_momentum_step_f64, ctypes.c_double, 8)):
        def call(n, params, grads, accums, numels, arrays=(True, True, True, True)):
            tabs = [(ctypes.c_void_p * max(len(v), 1))(*v) for v in (params, grads, accums)]
            ne = (ctypes.c_size_t * max(len(numels), 1))(*numels)
            args = [ctypes.cast(t, ctypes.c_void_p) if keep else None for t, keep in zip(tabs + [ne], arrays)]
            return fn(n, args[0], args[1], args[2], args[3], real(0.001), real(0.9), None)
        ok3 = ([256, 512, 1024], [2048, 4096, 8192], [256 + 65536, 512 + 65536, 1024 + 65536])
        assert call(-1, *ok3, [1, 1, 1]) == _lib.ERR_INVALID_ARGUMENT
        assert call(17, [256] * 17, [256] * 17, [256] * 17, [0] * 17) == _lib.ERR_INVALID_ARGUMENT
        assert call(0, [], [], [], []) == _lib.OK
        assert call(0, [], [], [], [], arrays=(False, False, False, False)) == _lib.OK
        assert call(3, *ok3, [0, 0, 0]) == _lib.OK                            # all counts zero: nothing launched
        assert call(3, [None] * 3, [None] * 3, [None] * 3, [0, 0, 0]) == _lib.OK   # ... and empty tensors may be NULL
        assert call(16, [None] * 16, [None] * 16, [None] * 16, [0] * 16) == _lib.OK
        for drop in range(4):                                                  # a NULL array
            arrays = tuple(i != drop for i in range(4))
            assert call(3, *ok3, [0, 0, 0], arrays=arrays) == _lib.ERR_INVALID_ARGUMENT
        for which in range(3):                                                 # a NULL entry with a non-zero count
            tabs = [list(v) for v in ok3]
            tabs[which][1] = None
            assert call(3, *tabs, [0, 5, 0]) == _lib.ERR_INVALID_ARGUMENT
            assert call(3, *tabs, [0, 0, 0]) == _lib.OK
        for which in range(3):                                                 # not aligned to the element size
            for bad in (1, 2, esz // 2, esz - 1):
                tabs = [list(v) for v in ok3]
                tabs[which][2] += bad
                assert call(3, *tabs, [0, 0, 7]) == _lib.ERR_INVALID_ARGUMENT, (which, bad)
                assert call(3, *tabs, [0, 0, 0]) == _lib.OK


def test_fc_backward_step_status_codes_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    need = lib.conv3p_fc_workspace_bytes(32, 4096, 512)
    assert need > 0

    def call(x=p, W=p, b=p, y=p, dy=p, M=32, K=4096, N=512, act=1, dx=p, aW=p, ab=p, ws=p, wsb=need):
        return lib.conv3p_fc_backward_step_f32(x, W, b, y, dy, M, K, N, act, dx, aW, ab, ctypes.c_float(0.001),
                                               ctypes.c_float(0.9), ws, wsb, None)
    assert call(M=-1) == _lib.ERR_INVALID_ARGUMENT and call(act=2) == _lib.ERR_INVALID_ARGUMENT
    for name in ("x", "W", "dy", "aW", "y"):
        assert call(**{name: None}) == _lib.ERR_INVALID_ARGUMENT, name
    assert call(b=None) == _lib.ERR_INVALID_ARGUMENT and call(ab=None) == _lib.ERR_INVALID_ARGUMENT   # one without the other
    assert call(M=0) == _lib.ERR_INVALID_ARGUMENT                              # no batch: no gradient to step with
    assert call(K=0) == _lib.OK and call(N=0) == _lib.OK                       # nothing to update
    assert call(N=516) == _lib.ERR_UNSUPPORTED and call(N=1032) == _lib.ERR_UNSUPPORTED and call(M=129) == _lib.ERR_UNSUPPORTED
    assert call(ws=None) == _lib.ERR_WORKSPACE and call(wsb=8) == _lib.ERR_WORKSPACE
    # the codes of conv3p_fc_backward_f32 for the same arguments
    def plain(M=32, K=4096, N=512, act=1, ws=p, wsb=need, x=p):
        return lib.conv3p_fc_backward_f32(x, p, p, p, M, K, N, act, p, p, p, ws, wsb, None)
    for kw in (dict(M=-1), dict(act=2), dict(x=None), dict(K=0), dict(N=516), dict(M=129), dict(ws=None), dict(wsb=8)):
        assert call(**kw) == plain(**kw), kw


def test_argument_checks():
    from pointwise_amd.optim import MomentumOptimizer, momentum_step
    w, g, a = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        MomentumOptimizer([w], 0.001)
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        momentum_step([w], [g], [a], 0.001, 0.9)
    with pytest.raises(op.Conv3pInvalidArgument, match=r"one gradient per parameter \(2 parameters, 1 gradients\)"):
        momentum_step([w, w], [g], [a, a], 0.001, 0.9)
    with pytest.raises(op.Conv3pInvalidArgument, match="the same dtype"):
        momentum_step([w], [g.double()], [a], 0.001, 0.9)
    with pytest.raises(op.Conv3pInvalidArgument, match="the same shape"):
        momentum_step([w], [torch.zeros(3, 4)], [a], 0.001, 0.9)
    with pytest.raises(op.Conv3pInvalidArgument, match="gradient must be contiguous"):
        momentum_step([w], [torch.zeros(3, 4).t()], [a], 0.001, 0.9)
    with pytest.raises(op.Conv3pInvalidArgument, match="parameter must be contiguous"):
        MomentumOptimizer([torch.zeros(3, 4).t()], 0.001)
    with pytest.raises(op.Conv3pInvalidArgument, match="float32 or float64"):
        MomentumOptimizer([w.half()], 0.001)
    with pytest.raises(op.Conv3pInvalidArgument, match="must be a tensor"):
        MomentumOptimizer([np.zeros(3)], 0.001)
    with pytest.raises(op.Conv3pInvalidArgument, match="learning_rate must be a number or a callable"):
        MomentumOptimizer([], "fast")
    opt = MomentumOptimizer([], 0.001)
    with pytest.raises(op.Conv3pInvalidArgument, match=r"one gradient per parameter \(0 parameters, 1 gradients\)"):
        opt.step([g])
    assert opt.global_step == 0                                               # a refused step does not count
    with pytest.raises(op.Conv3pInvalidArgument, match="not one of this optimizer's parameters"):
        opt.sharded_step(w, g)
    with pytest.raises(op.Conv3pInvalidArgument, match="not one of this optimizer's parameters"):
        opt.fused_fc_step(torch.zeros(2, 4), torch.zeros(4, 8), None, torch.zeros(2, 8), torch.zeros(2, 8))
    assert not opt.owns(w) and opt.owns()


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at `want` (a float64 number)."""
    return abs(float(np.float32(got)) - want) / float(np.spacing(np.float32(want)))


def test_exponential_decay_schedule():
    """The TF1 op casts its inputs to the learning rate's dtype and works in float32; the float64 closed form it is held
    against is therefore evaluated on those float32 inputs: float32(0.001) * float32(0.96) ** k.  (Against the form on
    the decimal literals the op itself is off by the rounding of its inputs: 0.41 ulp of float32(0.001), plus k times the
    2.2e-8 relative error of float32(0.96) -- 2.5 ulps at k = 12, whatever the arithmetic; printed below.)"""
    from pointwise_amd.optim import exponential_decay
    sched = lambda s, **kw: exponential_decay(PARAM_JSON["start"], s, PARAM_JSON["decay_steps"], PARAM_JSON["decay_rate"], **kw)
    start32 = float(np.float32(0.001))
    for s in (0, 1, 500, 99999):
        assert sched(s) == start32                                             # exactly `start` below decay_steps
    for lo in (100000, 1200000):
        vals = {sched(s) for s in (lo, lo + 1, lo + 34567, lo + 99999)}
        assert len(vals) == 1                                                  # constant inside a staircase interval
    assert sched(100000) < sched(99999) and sched(200000) < sched(199999)
    for s in (0, 99999, 100000, 1234567):
        k = s // 100000
        got = sched(s)
        assert isinstance(got, float) and float(np.float32(got)) == got        # a Python float holding a float32 value
        want = start32 * float(np.float32(0.96)) ** k
        print("step %d: %.9e, %.3f ulp of the closed form on the op's float32 inputs, %.3f ulp of the one on the literals"
              % (s, got, ulps32(got, want), ulps32(got, 0.001 * 0.96 ** k)))
        assert ulps32(got, want) <= 2.0
        assert got == exponential_decay_ref(0.001, s, 100000, 0.96)
    # the continuous form: a float exponent
    got = sched(150000, staircase=False)
    assert ulps32(got, start32 * float(np.float32(0.96)) ** 1.5) <= 2.0
    assert sched(150000) == sched(100000) and got < sched(150000)
    with pytest.raises(op.Conv3pInvalidArgument):
        exponential_decay(0.001, 5, 0, 0.96)


def test_learning_rate_is_the_schedule_before_the_increment_and_state_dict_round_trip():
    from pointwise_amd.optim import MomentumOptimizer, exponential_decay
    seen = []
    def lr(step):
        seen.append(step)
        return exponential_decay(0.001, step, 2, 0.5)
    opt = MomentumOptimizer([], lr, momentum=0.8)
    rates = []
    for _ in range(5):
        rates.append(opt.learning_rate())
        opt.step([])
    assert opt.global_step == 5 and seen == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]     # asked once here, once by step(): same step
    f = lambda v: float(np.float32(v))
    assert rates == [f(0.001), f(0.001), f(0.001) * 0.5, f(0.001) * 0.5, f(0.001) * 0.25]
    sd = opt.state_dict()
    assert sd["global_step"] == 5 and sd["momentum"] == 0.8 and sd["accumulators"] == [] and sd["shards"] == {}
    other = MomentumOptimizer([], lr)
    other.load_state_dict(sd)
    assert other.global_step == 5 and other.momentum == 0.8 and other.learning_rate() == f(0.001) * 0.25
    with pytest.raises(op.Conv3pInvalidArgument, match="one accumulator per parameter"):
        other.load_state_dict({"global_step": 1, "accumulators": [torch.zeros(2)]})
    assert MomentumOptimizer([], 0.1).learning_rate() == f(0.1)                # a constant rate is rounded to float32 too


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_ref_agrees_with_a_per_element_loop(dt):
    """momentum_step_ref against ApplyMomentum written out per element with every operation rounded on its own."""
    rng = np.random.default_rng(11)
    n = 300
    w, g, a = (rng.standard_normal(n).astype(dt) for _ in range(3))
    g[5], g[6], a[7] = np.nan, np.inf, dt(0)
    lr, m = float(np.float32(0.001)), 0.9
    w1, a1 = momentum_step_ref(w, g, a, lr, m)
    for i in range(n):
        with np.errstate(all="ignore"):
            t = dt(a[i] * dt(m))
            ai = dt(t + g[i])
            u = dt(ai * dt(lr))
            wi = dt(w[i] - u)
        assert np.array_equal(a1[i:i + 1], np.array([ai], dtype=dt), equal_nan=True)
        assert np.array_equal(w1[i:i + 1], np.array([wi], dtype=dt), equal_nan=True)
    assert np.isnan(a1[5]) and np.isnan(w1[5]) and np.isinf(a1[6]) and np.isinf(w1[6])
    assert np.isfinite(np.delete(w1, [5, 6])).all() and a1[7] == g[7]
