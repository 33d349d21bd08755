"""GPU tests of the guarded optimizer step (pointwise_amd/optim.py, csrc/conv3p_optim_guarded.hpp): the device-side
global norm, Nesterov's rule, clipping by the global norm and the step that is skipped on a non-finite gradient.

Norm: stats[0] against math.fsum of the float64 squares, relative error <= 1e-12.  All addends are non-negative and
summation is in double, so a dependent chain of L additions errs by at most L * 2^-53 relatively; float64 inputs add
one rounding per square.  The kernels keep L below 10^3 (per-lane partials, a butterfly, fixed runs in the finish), so
the bound is about 1e-13 and 1e-12 leaves a factor of ten.
Update: bit-equality with tests/optim_guarded_ref.py, which is given the device's own stats[0] so that the scale is
formed from the same double."""
import ctypes

import numpy as np
import pytest

from tests.optim_guarded_ref import clip_scale_ref, guarded_step_ref, sumsq_ref

LR, MOM = float(np.float32(0.01)), 0.9
SIZES = (0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5)
OFFSETS = (0, 1, 729)                                   # element offsets of a view inside its flat buffer
NORM_TOL = 1e-12
SLOT = 1024                                             # views start at a multiple of SLOT elements plus their offset


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from pointwise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tdt(dt):
    import torch
    return torch.float32 if dt == np.float32 else torch.float64


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


class Packed:
    """Arrays as views into ONE flat device buffer (as the stack's gradients are): array i starts at a multiple of SLOT
    elements plus offs[i], so offs[i] is its element offset inside a 16-byte line and beyond.  `flat` is the host copy
    of the whole buffer, gaps included: comparing it catches a write outside a view."""

    def __init__(self, dev, dt, arrays, offs):
        import torch
        starts, cur = [], 0
        for a, o in zip(arrays, offs):
            starts.append(cur + o)
            cur = (cur + o + a.size + SLOT - 1) // SLOT * SLOT + SLOT
        self.flat = np.zeros(cur, dtype=dt)
        self.spans = [(s, s + a.size) for s, a in zip(starts, arrays)]
        for (lo, hi), a in zip(self.spans, arrays):
            self.flat[lo:hi] = a
        self.buf = torch.from_numpy(self.flat).to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[lo:hi] for lo, hi in self.spans]

    def set(self, arrays):
        import torch
        for (lo, hi), a in zip(self.spans, arrays):
            self.flat[lo:hi] = a
        self.buf.copy_(torch.from_numpy(self.flat))

    def host(self):
        return [self.flat[lo:hi] for lo, hi in self.spans]


def check_norm(stats, arrays, bad=0):
    want, nbad = sumsq_ref(arrays)
    got = stats.cpu().numpy()
    assert nbad == bad and got[1] == bad, (got, nbad, bad)
    err = abs(got[0] - want) / want if want > 0 else abs(got[0])
    print("sumsq %.17g ref %.17g rel %.3e" % (got[0], want, err))
    assert err <= NORM_TOL, (got[0], want, err)


# --------------------------------------------------------------------------- 1 + 2: addressing and the norm
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_norm_over_sizes_and_offsets(dev, dt):
    import torch
    from pointwise_amd.optim import grad_sumsq
    rng = np.random.default_rng(300)
    every, every_host = [], []
    for n in SIZES:
        flat = rng.standard_normal(n + max(OFFSETS)).astype(dt)
        buf = torch.from_numpy(flat).to(dev)
        views = [buf[o:o + n] for o in OFFSETS]                               # read only: they may overlap
        host = [flat[o:o + n] for o in OFFSETS]
        for v, h in zip(views, host):
            st = grad_sumsq([v])
            assert st.dtype == torch.float64 and tuple(st.shape) == (2,) and st.device == buf.device
            check_norm(st, [h])
            assert torch.equal(st, grad_sumsq([v]))                           # identical calls, identical bits
        check_norm(grad_sumsq(views), host)
        every += views
        every_host += host
        assert torch.equal(buf.cpu(), torch.from_numpy(flat))                # gradients are read only
    assert len(every) == 21                                                   # two launches and the accumulate chain
    st = grad_sumsq(every + [None])
    check_norm(st, every_host)
    assert torch.equal(st, grad_sumsq([None] + every))
    # nothing to read: zeros when not accumulating, untouched when accumulating
    empty = torch.zeros(0, dtype=tdt(dt), device=dev)
    out = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    assert grad_sumsq([empty, None], out=out) is out and out.cpu().tolist() == [0.0, 0.0]
    out.fill_(7.0)
    grad_sumsq([empty], out=out, accumulate=True)
    assert out.cpu().tolist() == [7.0, 7.0]
    grad_sumsq([], out=out)
    assert out.cpu().tolist() == [0.0, 0.0]


@pytest.mark.gpu
def test_norm_of_17_tensors_and_of_mixed_dtypes(dev):
    import torch
    from pointwise_amd.optim import grad_sumsq
    rng = np.random.default_rng(301)
    sizes = [3000 + 731 * i for i in range(16)] + [9001]
    for dt in (np.float32, np.float64):
        pk = Packed(dev, dt, [rng.standard_normal(n).astype(dt) for n in sizes], [OFFSETS[i % 3] for i in range(17)])
        st = grad_sumsq(pk.views)
        check_norm(st, pk.host())
        assert torch.equal(st, grad_sumsq(pk.views))
    a32 = [rng.standard_normal(n).astype(np.float32) for n in (4097, 5, 12000)]
    a64 = [rng.standard_normal(n).astype(np.float64) for n in (729, 8197)]
    p32, p64 = Packed(dev, np.float32, a32, (1, 0, 729)), Packed(dev, np.float64, a64, (729, 1))
    mixed = [p32.views[0], p64.views[0], p32.views[1], p64.views[1], p32.views[2]]
    st = grad_sumsq(mixed)
    check_norm(st, a32 + a64)
    assert torch.equal(st, grad_sumsq(mixed))
    # the same through out= / accumulate=: one dtype after the other, by hand
    out = torch.empty(2, dtype=torch.float64, device=dev)
    grad_sumsq(p32.views, out=out)
    grad_sumsq(p64.views, out=out, accumulate=True)
    assert torch.equal(out, st)


@pytest.mark.gpu
def test_norm_where_the_grid_stride_loop_runs_twice(dev):
    """2048 * 4096 + 4096 + 7 elements: 2050 chunks for a grid of 2048."""
    import torch
    from pointwise_amd.optim import grad_sumsq
    n = 2048 * 4096 + 4096 + 7
    g = np.random.default_rng(302).standard_normal(n, dtype=np.float32)
    G = torch.from_numpy(g).to(dev)
    st = grad_sumsq([G])
    check_norm(st, [g])
    assert torch.equal(st, grad_sumsq([G]))
    g[[0, 4096 * 2048 + 1, n - 1]] = [np.inf, np.nan, -np.inf]                # first chunk, second round, tail
    G = torch.from_numpy(g).to(dev)
    check_norm(grad_sumsq([G]), [g], bad=3)


@pytest.mark.gpu
def test_norm_that_overflows_counts_as_non_finite(dev):
    import torch
    from pointwise_amd.optim import grad_sumsq
    G = torch.full((100,), 1e200, dtype=torch.float64, device=dev)
    st = grad_sumsq([G]).cpu().numpy()
    assert np.isinf(st[0]) and st[1] == 1.0


# --------------------------------------------------------------------------- 3: the update, bit for bit
TRIPLES = [(n, (o, o, o)) for n in SIZES for o in OFFSETS] + [(4097, (0, 1, 2)), (2 * 4096 + 5, (3, 2, 0)), (3, (1, 0, 0))]
TOTAL = sum(n for n, _ in TRIPLES)
MODES = {"plain": (False, None), "nesterov": (True, None), "clipped": (False, 0.4), "clipped_nesterov": (True, 0.4),
         "below_clip_norm": (False, 10.0), "below_clip_norm_nesterov": (True, 10.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_update_is_bit_equal_to_the_numpy_rule(dev, dt, mode):
    """Three consecutive steps over 24 tensors (two launches): every size and offset, and three triples whose pointers
    differ in their offset inside a 16-byte line.  clip_norm is a fraction of sqrt(TOTAL), the expected norm of that
    many standard normal values: 0.4 of it clips (scale about 0.4), 10 times it does not (scale exactly 1)."""
    import torch
    from pointwise_amd.optim import momentum_step
    nesterov, frac = MODES[mode]
    clip = None if frac is None else frac * float(np.sqrt(TOTAL))
    rng = np.random.default_rng(400)
    mk = lambda: [rng.standard_normal(n).astype(dt) for n, _ in TRIPLES]
    W = Packed(dev, dt, mk(), [o[0] for _, o in TRIPLES])
    G = Packed(dev, dt, mk(), [o[1] for _, o in TRIPLES])
    A = Packed(dev, dt, mk(), [o[2] for _, o in TRIPLES])
    for (_, o), w, g, a in zip(TRIPLES, W.views, G.views, A.views):
        assert [t.data_ptr() % 16 for t in (w, g, a)] == [(k * w.element_size()) % 16 for k in o] or w.numel() == 0
    ref_w, ref_a = [x.copy() for x in W.host()], [x.copy() for x in A.host()]
    if frac == 10.0:
        W2, A2 = W.buf.clone(), A.buf.clone()
        views2 = lambda b, pk: [b[lo:hi] for lo, hi in pk.spans]
    for step in range(3):
        G.set(mk())
        used = momentum_step(W.views, G.views, A.views, LR, MOM, use_nesterov=nesterov, clip_norm=clip)
        scale = None
        if clip is None:
            assert used is None
        else:
            check_norm(used, G.host())
            scale = clip_scale_ref(used.cpu().numpy()[0], clip, dt)
            print(mode, "scale", scale)
            if frac == 0.4:
                assert 0.1 < scale < 0.9
            else:
                assert scale == 1
                momentum_step(views2(W2, W), G.views, views2(A2, A), LR, MOM, use_nesterov=nesterov)   # the unclipped step
        for i, g in enumerate(G.host()):
            ref_w[i], ref_a[i] = guarded_step_ref(ref_w[i], g, ref_a[i], LR, MOM, nesterov=nesterov, scale=scale)
        for i, ((lo, hi), so) in enumerate(zip(W.spans, TRIPLES)):
            W.flat[lo:hi], A.flat[A.spans[i][0]:A.spans[i][1]] = ref_w[i], ref_a[i]
        assert same(A.buf.cpu().numpy(), A.flat), ("accum", step)             # whole buffers: nothing outside a view moved
        assert same(W.buf.cpu().numpy(), W.flat), ("param", step)
        assert same(G.buf.cpu().numpy(), G.flat)
        if frac == 10.0:
            assert torch.equal(W2, W.buf) and torch.equal(A2, A.buf)


# --------------------------------------------------------------------------- 4: the defaults are the plain entry
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_guarded_entry_with_defaults_equals_the_plain_entry(dev, dt):
    import torch
    from pointwise_amd import _lib
    lib = _lib.load()
    sfx, real = ("f32", ctypes.c_float) if dt == np.float32 else ("f64", ctypes.c_double)
    rng = np.random.default_rng(500)
    trip = TRIPLES[:16]
    mk = lambda k: Packed(dev, dt, [rng.standard_normal(n).astype(dt) for n, _ in trip], [o[k] for _, o in trip])
    W, G, A = mk(0), mk(1), mk(2)
    W2, A2 = mk(0), mk(2)
    W2.set(W.host())
    A2.set(A.host())
    stream = torch.cuda.current_stream(dev).cuda_stream

    def tables(w, a):
        cols = [(ctypes.c_void_p * 16)(*[v.data_ptr() for v in pk.views]) for pk in (w, G, a)]
        ne = (ctypes.c_size_t * 16)(*[n for n, _ in trip])
        return cols, ne
    for _ in range(2):
        cols, ne = tables(W, A)
        vp = lambda x: ctypes.cast(x, ctypes.c_void_p)
        assert getattr(lib, "conv3p_momentum_step_" + sfx)(16, vp(cols[0]), vp(cols[1]), vp(cols[2]), vp(ne), real(LR),
                                                           real(MOM), stream) == _lib.OK
        cols2, ne2 = tables(W2, A2)
        assert getattr(lib, "conv3p_momentum_step_guarded_" + sfx)(16, vp(cols2[0]), vp(cols2[1]), vp(cols2[2]), vp(ne2),
                                                                   real(LR), real(MOM), 0, real(-1.0), 0, None,
                                                                   stream) == _lib.OK
        torch.cuda.synchronize(dev)
        assert torch.equal(W.buf, W2.buf) and torch.equal(A.buf, A2.buf)
    assert not torch.equal(W.buf, torch.from_numpy(W.flat).to(dev))          # ... and something was updated


# --------------------------------------------------------------------------- 5: the skipped step
def seventeen(dev, dt, rng):
    sizes = [3000 + 731 * i for i in range(16)] + [9001]
    offs = [OFFSETS[i % 3] for i in range(17)]
    mk = lambda: [rng.standard_normal(n).astype(dt) for n in sizes]
    return Packed(dev, dt, mk(), offs), Packed(dev, dt, mk(), offs), mk


PLANTS = {"inf": [(5, 17, np.inf)], "nan": [(16, 9000, np.nan)], "both": [(0, 0, -np.inf), (11, 4096, np.nan)]}


@pytest.mark.gpu
@pytest.mark.parametrize("plant", list(PLANTS))
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_a_non_finite_gradient_skips_the_step(dev, dt, plant):
    import torch
    from pointwise_amd.optim import MomentumOptimizer
    rng = np.random.default_rng(600)
    W, G, mk = seventeen(dev, dt, rng)
    opt = MomentumOptimizer(W.views, LR, MOM, skip_nonfinite=True)
    assert opt.fusable is False
    ref_w, ref_a = [x.copy() for x in W.host()], [np.zeros_like(x) for x in W.host()]

    def clean_step():
        G.set(mk())
        opt.step(G.views)
        for i, g in enumerate(G.host()):
            ref_w[i], ref_a[i] = guarded_step_ref(ref_w[i], g, ref_a[i], LR, MOM)
        for i in range(17):
            assert same(opt.accums[i].cpu().numpy(), ref_a[i]) and same(W.views[i].cpu().numpy(), ref_w[i]), i
        assert opt.grad_stats.cpu().numpy()[1] == 0
    clean_step()                                                              # accumulators are no longer zero
    assert int(opt.skipped_steps) == 0
    g = mk()
    for t, e, v in PLANTS[plant]:
        g[t][e] = v
    G.set(g)
    before_w, before_a = W.buf.clone(), [a.clone() for a in opt.accums]
    opt.step(G.views)
    assert torch.equal(W.buf, before_w) and all(torch.equal(a, b) for a, b in zip(opt.accums, before_a))
    assert opt.grad_stats.cpu().numpy()[1] == len(PLANTS[plant])
    check_norm(opt.grad_stats, G.host(), bad=len(PLANTS[plant]))             # the norm is that of the finite elements
    assert int(opt.skipped_steps) == 1 and opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.device == W.buf.device
    assert opt.global_step == 2                                               # the host does not know: it counts on
    clean_step()
    assert int(opt.skipped_steps) == 1 and opt.global_step == 3
    norm, bad = opt.last_grad_norm()
    assert bad == 0 and norm == float(np.sqrt(opt.grad_stats.cpu().numpy()[0]))
    # the count and the settings travel in the state dictionary
    other = MomentumOptimizer(W.views, LR, MOM)
    other.load_state_dict(opt.state_dict())
    assert int(other.skipped_steps) == 1 and other.skip_nonfinite and other.skipped_steps.device == W.buf.device


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_without_skipping_the_norm_excludes_the_element_and_the_step_proceeds(dev, dt):
    from pointwise_amd.optim import MomentumOptimizer
    rng = np.random.default_rng(601)
    W, G, mk = seventeen(dev, dt, rng)
    total = sum(v.numel() for v in W.views)
    clip = 0.4 * float(np.sqrt(total))
    opt = MomentumOptimizer(W.views, LR, MOM, clip_norm=clip, use_nesterov=True)
    g = mk()
    g[5][17], g[16][9000] = np.inf, np.nan
    G.set(g)
    before = [x.copy() for x in W.host()]
    opt.step(G.views)
    check_norm(opt.grad_stats, G.host(), bad=2)
    assert int(opt.skipped_steps) == 0
    scale = clip_scale_ref(opt.grad_stats.cpu().numpy()[0], clip, dt)
    assert 0.1 < scale < 0.9
    for i in range(17):
        w, a = guarded_step_ref(before[i], g[i], np.zeros_like(before[i]), LR, MOM, nesterov=True, scale=scale)
        assert same(W.views[i].cpu().numpy(), w) and same(opt.accums[i].cpu().numpy(), a), i
    got = W.views[5].cpu().numpy()
    assert not np.isfinite(got[17]) and np.isfinite(np.delete(got, 17)).all()          # exactly its element


# --------------------------------------------------------------------------- 6: stats from outside
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_externally_supplied_stats_are_used_as_they_are(dev, dt):
    """What a data-parallel caller does after all-reducing the two values: here twice this process's own."""
    import torch
    from pointwise_amd.optim import MomentumOptimizer, grad_sumsq
    rng = np.random.default_rng(602)
    W, G, mk = seventeen(dev, dt, rng)
    total = sum(v.numel() for v in W.views)
    clip = 0.4 * float(np.sqrt(total))
    opt = MomentumOptimizer(W.views, LR, MOM, clip_norm=clip, skip_nonfinite=True)
    before = [x.copy() for x in W.host()]
    own = grad_sumsq(G.views)
    ext = own * 2
    opt.step(G.views, stats=ext)
    assert opt.grad_stats is ext and torch.equal(own * 2, ext)               # used, not recomputed, not written
    s_own = clip_scale_ref(own.cpu().numpy()[0], clip, dt)
    scale = clip_scale_ref(ext.cpu().numpy()[0], clip, dt)
    assert 0.1 < scale < s_own < 0.9
    for i, g in enumerate(G.host()):
        w, a = guarded_step_ref(before[i], g, np.zeros_like(before[i]), LR, MOM, scale=scale)
        assert same(W.views[i].cpu().numpy(), w) and same(opt.accums[i].cpu().numpy(), a), i
    # a supplied count of non-finite elements skips, whatever the gradients hold
    ext2 = torch.tensor([1.0, 1.0], dtype=torch.float64, device=dev)
    keep = W.buf.clone()
    opt.step(G.views, stats=ext2)
    assert torch.equal(W.buf, keep) and int(opt.skipped_steps) == 1
    # sharded_step without a process group: the whole tensor, the same kernel, the same stats
    p = torch.from_numpy(rng.standard_normal(5000).astype(dt)).to(dev)
    gr = torch.from_numpy(rng.standard_normal(5000).astype(dt)).to(dev)
    o2 = MomentumOptimizer([p], LR, MOM, clip_norm=1.0, use_nesterov=True)
    p0 = p.cpu().numpy()
    st = grad_sumsq([gr]) * 4
    o2.sharded_step(p, gr, stats=st)
    w, a = guarded_step_ref(p0, gr.cpu().numpy(), np.zeros_like(p0), LR, MOM, nesterov=True,
                            scale=clip_scale_ref(st.cpu().numpy()[0], 1.0, dt))
    assert same(p.cpu().numpy(), w) and same(o2.accums[0].cpu().numpy(), a) and o2.grad_stats is st
