"""GPU tests of the momentum optimizer (pointwise_amd/optim.py, csrc/conv3p_optim.hpp).

The contract is bit-equality with tests/optim_ref.py -- numpy's separately rounded `a * m + g` and `w - a * lr` in the
parameter's dtype -- for every size, alignment and grouping, and of the fused fc step with the separate path.  The two
model-level tests run two training steps and hold step 2's forward pass against the CPU composition evaluated with the
numpy-updated parameters, within the tolerances of test_model_step.py / test_seg_model_step.py."""
import itertools

import numpy as np
import pytest

from oracle import head_numpy, oracle
from tests.optim_ref import MomentumRef, momentum_step_ref
from tests.seg_head_ref import seg_head_ref

LR, MOM = float(np.float32(0.001)), 0.9
SIZES = (0, 1, 3, 4, 63, 64, 65, 729, 6561, 1000003)
FC1 = (73728, 512)                                     # the model's fc1: 2048 points x 36 channels -> 512
GUARD = 8                                              # elements around every slice that must stay untouched


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from pointwise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def tdt(dt):
    import torch
    return torch.float32 if dt == np.float32 else torch.float64


class Sliced:
    """A device tensor of n elements at element offset `off` of a larger zeroed buffer (torch allocations are aligned
    to 512 bytes, so `off` is the tensor's offset inside a 16-byte line, in elements)."""

    def __init__(self, dev, dt, arr, off):
        import torch
        self.buf = torch.zeros(arr.size + GUARD, dtype=tdt(dt), device=dev)
        self.off, self.n = off, arr.size
        self.t = self.buf[off:off + arr.size]
        assert arr.size == 0 or self.t.data_ptr() % 16 == (off * arr.itemsize) % 16
        self.set(arr)

    def set(self, arr):
        import torch
        self.t.copy_(torch.from_numpy(arr))

    def get(self):
        return self.t.cpu().numpy()

    def guard_untouched(self):
        b = self.buf.cpu().numpy()
        return not b[:self.off].any() and not b[self.off + self.n:].any()


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def run_steps(dev, dt, sizes_offs, seed, check_at=(1, 5)):
    """Every (n, (offset of param, grad, accum)) as one tensor triple, all stepped together by momentum_step (16 per
    launch); bit-compared with the restatement after the steps in `check_at`."""
    from pointwise_amd.optim import momentum_step
    rng = np.random.default_rng(seed)
    W, G, A, ref = [], [], [], []
    for n, (ow, og, oa) in sizes_offs:
        w, a = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
        W.append(Sliced(dev, dt, w, ow))
        G.append(Sliced(dev, dt, np.zeros(n, dt), og))
        A.append(Sliced(dev, dt, a, oa))
        ref.append([w, a])
    for step in range(1, max(check_at) + 1):
        for i, (n, _) in enumerate(sizes_offs):
            g = rng.standard_normal(n).astype(dt)
            G[i].set(g)
            ref[i] = list(momentum_step_ref(ref[i][0], g, ref[i][1], LR, MOM))
        momentum_step([s.t for s in W], [s.t for s in G], [s.t for s in A], LR, MOM)
        if step in check_at:
            for i, so in enumerate(sizes_offs):
                assert same(A[i].get(), ref[i][1]), ("accum", so, step)
                assert same(W[i].get(), ref[i][0]), ("param", so, step)
    for i, so in enumerate(sizes_offs):
        assert W[i].guard_untouched() and A[i].guard_untouched() and G[i].guard_untouched(), so


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_bit_equal_over_sizes_and_alignments(dev, dt):
    offs = list(itertools.product(range(4), repeat=3))                       # every mix of 16-byte alignment
    for n in SIZES[:-1]:
        run_steps(dev, dt, [(n, o) for o in offs], seed=100 + n)
    some = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 0), (1, 0, 0), (0, 0, 3), (2, 3, 1)]
    run_steps(dev, dt, [(SIZES[-1], o) for o in some], seed=7)
    # all sizes in one call, in both orders: empty tensors first / last / between
    run_steps(dev, dt, [(n, (n % 4, n % 4, n % 4)) for n in SIZES], seed=8)
    run_steps(dev, dt, [(n, (0, 0, 0)) for n in reversed(SIZES)], seed=9)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_bit_equal_at_the_shape_of_fc1(dev, dt):
    """151 MB (302 in fp64) per array: more chunks than the grid cap, so the grid-stride loop runs."""
    import torch
    from pointwise_amd.optim import MomentumOptimizer
    rng = np.random.default_rng(3)
    w = rng.standard_normal(FC1, dtype=np.float32).astype(dt)
    W = torch.from_numpy(w).to(dev)
    opt = MomentumOptimizer([W], LR, MOM)
    ref = MomentumRef([w], LR, MOM)
    for step in range(1, 6):
        g = rng.standard_normal(FC1, dtype=np.float32).astype(dt)
        opt.step([torch.from_numpy(g).to(dev)])
        ref.step([g])
        if step in (1, 5):
            assert same(opt.accums[0].cpu().numpy(), ref.accums[0]) and same(W.cpu().numpy(), ref.params[0]), step
    assert opt.global_step == 5


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_bit_equal_on_the_stack_layout(dev, dt):
    """The stack's real layout: st.filters with st.grad_views, views into fused_grad at element offsets 729, 2916, ...
    (4-byte alignment only)."""
    import torch
    from pointwise_amd import stack
    from pointwise_amd.optim import MomentumOptimizer
    st = stack.Conv3pStack(3, 13, device=dev, dtype=tdt(dt), seed=41)
    assert [v.data_ptr() - st.fused_grad.data_ptr() for v in st.grad_views][1] == 729 * np.dtype(dt).itemsize
    sched = lambda s: 0.01 * 0.5 ** s
    opt = MomentumOptimizer(st.filters, sched, MOM)
    ref = MomentumRef([f.cpu().numpy() for f in st.filters], sched, MOM)
    rng = np.random.default_rng(42)
    for step in range(1, 6):
        fused = rng.standard_normal(st.fused_grad.numel()).astype(dt)
        st.fused_grad.copy_(torch.from_numpy(fused).to(dev))
        opt.step(st.grad_views)
        ref.step([v.cpu().numpy() for v in st.grad_views])
        if step in (1, 5):
            for i in range(5):
                assert same(opt.accums[i].cpu().numpy(), ref.accums[i]) and same(st.filters[i].cpu().numpy(), ref.params[i])
    assert same(st.fused_grad.cpu().numpy(), fused)                          # gradients are read only


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_grouping_into_launches_does_not_matter(dev, dt):
    """17 tensors (two launches) against 17 single-tensor calls."""
    import torch
    from pointwise_amd.optim import momentum_step
    rng = np.random.default_rng(17)
    sizes = [5000 + 731 * i for i in range(16)] + [70001]
    mk = lambda: [torch.from_numpy(rng.standard_normal(n).astype(dt)).to(dev) for n in sizes]
    W, G, A = mk(), mk(), mk()
    W1, A1 = [w.clone() for w in W], [a.clone() for a in A]
    for _ in range(3):
        momentum_step(W, G, A, LR, MOM)
        for w, g, a in zip(W1, G, A1):
            momentum_step([w], [g], [a], LR, MOM)
    for i in range(17):
        assert torch.equal(W[i], W1[i]) and torch.equal(A[i], A1[i]), i
        w, a = momentum_step_ref(*(t.cpu().numpy() for t in (W[i], G[i], A[i])), LR, MOM)    # ... and still the rule
        momentum_step([W[i]], [G[i]], [A[i]], LR, MOM)
        assert same(W[i].cpu().numpy(), w) and same(A[i].cpu().numpy(), a)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_nan_and_inf_reach_exactly_their_element(dev, dt):
    import torch
    from pointwise_amd.optim import momentum_step
    rng = np.random.default_rng(23)
    n = 9001
    w, g, a = (rng.standard_normal(n).astype(dt) for _ in range(3))
    g[1234], g[77], g[9000] = np.nan, np.inf, -np.inf
    W, G, A = (torch.from_numpy(v).to(dev) for v in (w, g, a))
    momentum_step([W], [G], [A], LR, MOM)
    rw, ra = momentum_step_ref(w, g, a, LR, MOM)
    gw, ga = W.cpu().numpy(), A.cpu().numpy()
    assert same(gw, rw) and same(ga, ra)
    bad = np.zeros(n, bool)
    bad[[1234, 77, 9000]] = True
    assert np.array_equal(~np.isfinite(gw), bad) and np.array_equal(~np.isfinite(ga), bad)
    assert np.isnan(gw[1234]) and np.isnan(ga[1234]) and ga[77] == np.inf and gw[77] == -np.inf and gw[9000] == np.inf


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(3, 512, 512), (32, 512, 512), (64, 512, 512), (3, 1000, 512), (32, 1000, 512),
                                   (64, 1000, 512), (32, 1001, 40)])
def test_fused_fc_step_equals_grad_then_step(dev, M, K, N):
    """W, b, both accumulators and dx after fused_fc_step, against fully_connected_grad followed by step on copies,
    bit for bit, from non-zero accumulators.  K = 512 is a multiple of the workgroup's 128 rows (4 waves x 32), 1000 and
    1001 are not (a partial wave, a partial workgroup); N = 40 leaves a partial 32-column block."""
    import torch
    from pointwise_amd import head
    from pointwise_amd.optim import MomentumOptimizer
    g = torch.Generator().manual_seed(M * 7 + K)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, W, b, dy = rnd(M, K), rnd(K, N) * 0.05, rnd(N), rnd(M, N)
    aW, ab = rnd(K, N), rnd(N)
    y = head.fully_connected(x, W, b, selu=True)
    W2, b2 = W.clone(), b.clone()
    lr = 0.05
    opt, opt2 = MomentumOptimizer([W, b], lr, MOM), MomentumOptimizer([W2, b2], lr, MOM)
    for o in (opt, opt2):
        o.accums[0].copy_(aW)
        o.accums[1].copy_(ab)
    dx2, dW, db = head.fully_connected_grad(x, W2, y, dy, selu=True)         # dx2: from the OLD W
    opt2.step([dW, db])
    dx = opt.fused_fc_step(x, W, b, y, dy, selu=True)
    assert not torch.equal(opt2.accums[0], aW)
    assert torch.equal(dx, dx2)
    assert torch.equal(opt.accums[0], opt2.accums[0]) and torch.equal(opt.accums[1], opt2.accums[1])
    assert torch.equal(W, W2) and torch.equal(b, b2)
    assert opt.global_step == 0 and opt2.global_step == 1                    # the fused call is not a step() by itself
    # without a bias, and without dx
    W3, W4 = W.clone(), W.clone()
    o3, o4 = MomentumOptimizer([W3], lr, MOM), MomentumOptimizer([W4], lr, MOM)
    y3 = head.fully_connected(x, W3, None, selu=False)
    _, dW3, _ = head.fully_connected_grad(x, W4, y3, dy, selu=False, need_dx=False)
    o4.step([dW3])
    assert o3.fused_fc_step(x, W3, None, y3, dy, selu=False, need_dx=False) is None
    assert torch.equal(W3, W4) and torch.equal(o3.accums[0], o4.accums[0]) and not torch.equal(W3, W)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_sharded_step_without_a_process_group_and_the_slice_path(dev, dt):
    import torch
    from pointwise_amd.optim import MomentumOptimizer, momentum_step
    rng = np.random.default_rng(31)
    w = rng.standard_normal((173, 59)).astype(dt)
    Wa, Wb = torch.from_numpy(w).to(dev), torch.from_numpy(w).to(dev)
    oa, ob = MomentumOptimizer([Wa], LR, MOM), MomentumOptimizer([Wb], LR, MOM)
    for _ in range(3):
        g = torch.from_numpy(rng.standard_normal(w.shape).astype(dt)).to(dev)
        oa.step([g])
        assert ob.sharded_step(Wb, g.clone()) is Wb
        ob.step([None])                                                       # the step count moves with step() only
    assert torch.equal(Wa, Wb) and torch.equal(oa.accums[0], ob.accums[0]) and oa.global_step == ob.global_step == 3
    assert ob.accums[0].numel() == w.size                                    # one rank: the whole tensor
    # the slice path as a rank of a larger world drives it: an odd [lo, hi), a slice-sized accumulator
    lo, hi = 1237, 8191
    flat = Wa.reshape(-1)
    before = flat.cpu().numpy().copy()
    g = rng.standard_normal(hi - lo).astype(dt)
    acc = rng.standard_normal(hi - lo).astype(dt)
    A = torch.from_numpy(acc).to(dev)
    momentum_step([flat[lo:hi]], [torch.from_numpy(g).to(dev)], [A], LR, MOM)
    rw, ra = momentum_step_ref(before[lo:hi], g, acc, LR, MOM)
    after = flat.cpu().numpy()
    assert same(after[lo:hi], rw) and same(A.cpu().numpy(), ra)
    assert same(after[:lo], before[:lo]) and same(after[hi:], before[hi:])


def rel(got, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(1.0, np.abs(want).max()))


@pytest.mark.gpu
def test_two_training_steps_of_the_classification_model(dev):
    """Sizes, inputs and TOL of test_model_step.py.  Run A keeps the separate path (gradients, then step), run B lets
    fc1's gradient pass apply the update (ClassificationHead.backward(optimizer=...)).  Learning rate 0.05, halved every
    step: large enough that step 2's logits move by far more than TOL, so a missing update cannot pass, and small enough
    that the softmax does not saturate (the loss stays a number that can differ)."""
    import torch
    from pointwise_amd import head, stack, synth
    from pointwise_amd.optim import MomentumOptimizer, exponential_decay
    TOL, VOX = 2e-4, 0.1
    B, N, NCLS = 3, 192, 40
    rng = np.random.default_rng(21)
    Pn = synth.modelnet_like(B, N, seed=1500)
    labels = rng.integers(0, NCLS, size=B)
    mask = (rng.random((B, 512)) < 0.5).astype(np.float32)
    P, lab, keep = torch.from_numpy(Pn).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(mask).to(dev)
    sched = lambda s: exponential_decay(0.05, s, 1, 0.5)
    f32 = lambda v: np.float32(v)

    def forward(st, hd):
        acts = st.forward(P, P)
        feat = torch.cat(list(acts), dim=2).contiguous()
        logits = hd.forward(feat, training=True, keep_mask=keep)
        loss, dlogits = hd.loss(logits, lab)
        return logits, loss, dlogits

    def run(fused):
        st = stack.Conv3pStack(3, None, device=dev, seed=1501)
        hd = head.ClassificationHead(N, num_class=NCLS, device=dev, seed=7)
        params = list(st.filters) + hd.parameters()
        opt = MomentumOptimizer(params, sched, MOM)
        out = {"w0": [p.cpu().numpy().copy() for p in params]}
        for step in (1, 2):
            logits, loss, dlogits = forward(st, hd)
            dfeat = hd.backward(dlogits, optimizer=opt if fused else None)
            st.backward(dfeat)
            grads = list(st.grad_views) + hd.gradients()
            assert (grads[4] is None and grads[5] is None) == fused
            out["g%d" % step] = [g.cpu().numpy().copy() if g is not None else None for g in grads]
            out["logits%d" % step], out["loss%d" % step] = logits.cpu().numpy(), float(loss)
            opt.step(grads)
            out["w%d" % step] = [p.cpu().numpy().copy() for p in params]
            out["a%d" % step] = [a.cpu().numpy().copy() for a in opt.accums]
        logits, loss, _ = forward(st, hd)
        out["logits3"], out["loss3"] = logits.cpu().numpy(), float(loss)
        assert opt.global_step == 2
        return out

    A, Bf = run(False), run(True)
    lr1, lr2 = f32(sched(0)), f32(sched(1))
    assert lr1 == f32(0.05) and lr2 == f32(0.05) * f32(0.5)
    # after step 1: accum = 0 * m + g = g, param = w - g * lr, bit for bit from the device's own gradients
    for i in range(8):
        assert same(A["a1"][i], A["g1"][i]), i
        assert same(A["w1"][i], A["w0"][i] - A["g1"][i] * lr1), i
        # ... and after step 2, the full rule
        a2 = A["a1"][i] * f32(MOM) + A["g2"][i]
        assert same(A["a2"][i], a2) and same(A["w2"][i], A["w1"][i] - a2 * lr2), i
    # the fused fc1 path: the same parameters, accumulators and forward passes, bit for bit
    for k in ("w1", "a1", "w2", "a2"):
        for i in range(8):
            assert same(A[k][i], Bf[k][i]), (k, i)
    for k in ("logits1", "logits2", "logits3"):
        assert same(A[k], Bf[k]), k
    assert A["loss2"] == Bf["loss2"] and A["loss3"] == Bf["loss3"]
    for i in (0, 1, 2, 3, 6, 7):
        assert same(A["g2"][i], Bf["g2"][i]), i
    # step 2's (and 3's) forward against the CPU composition with the numpy-updated parameters
    for step, wk in ((2, "w1"), (3, "w2")):
        w = A[wk]
        x, ref_acts = Pn, []
        for li in range(4):
            s = stack.CLS_STRIDES[li]
            x = stack.selu_numpy(oracle.forward(Pn, x, w[li], (s, s, s), VOX))
            ref_acts.append(x)
        r = head_numpy.head_forward_backward(np.concatenate(ref_acts, axis=2), w[4], w[5], w[6], w[7], labels, 0.5,
                                             mask.astype(np.float64))
        e_l, e_s = rel(A["logits%d" % step], r["logits"]), abs(A["loss%d" % step] - r["loss"]) / max(1.0, abs(r["loss"]))
        moved = float(np.abs(A["logits%d" % step] - A["logits%d" % (step - 1)]).max())
        print("step %d: logits %.3e loss %.3e (TOL %.0e); loss %.6f ref %.6f; logits moved by %.3e since the step before"
              % (step, e_l, e_s, TOL, A["loss%d" % step], r["loss"], moved))
        assert r["loss"] > 1e-3
        assert moved > 50 * TOL                                              # the update matters at this learning rate
        assert e_l <= TOL and e_s <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_two_training_steps_of_the_segmentation_stack(dev, dt):
    """Sizes, inputs and tolerances of test_seg_model_step.py (global_points = 1: gradients of order 1).  All five
    filters are updated from fused_grad in ONE launch; step 2's loss is held against the CPU composition with the
    numpy-updated filters."""
    import torch
    from pointwise_amd import stack, synth
    from pointwise_amd.optim import MomentumOptimizer
    from pointwise_amd.seg_head import SegmentationHead
    VOX, EPS = 0.1, 2.0 ** -24
    tol_a, head_factor = {np.float32: (2e-5, 8 * EPS), np.float64: (1e-11, 1e-12)}[dt]
    B, N, CIN, NCLS = 2, 256, 9, 13
    R = B * N
    Pn = synth.room_like(B, N, seed=2600).astype(dt)
    Xn = synth.features(B, N, CIN, 2601, points=Pn, dtype=dt)
    labels = np.random.default_rng(2602).integers(0, NCLS, size=(B, N))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P, X, lab = t(Pn), t(Xn), t(labels)
    lr = 0.01
    st = stack.Conv3pStack(CIN, NCLS, device=dev, dtype=tdt(dt), seed=2603)
    hd = SegmentationHead(NCLS, device=dev)
    opt = MomentumOptimizer(st.filters, lr, MOM)
    w0 = [f.cpu().numpy().copy() for f in st.filters]
    acts = st.forward(P, X)
    loss1, dact = hd.loss(acts[4], lab, global_points=1)
    st.backward([dact])
    g1 = [v.cpu().numpy().copy() for v in st.grad_views]
    opt.step(st.grad_views)
    w1 = [f.cpu().numpy() for f in st.filters]
    for i in range(5):
        assert same(opt.accums[i].cpu().numpy(), g1[i]), i                   # 0 * m + g = g
        assert same(w1[i], w0[i] - g1[i] * dt(np.float32(lr))), i
        assert np.abs(w1[i] - w0[i]).max() > 1e-3                            # the step is far above every tolerance here
    acts = st.forward(P, X)
    loss2, _ = hd.loss(acts[4], lab, global_points=1)
    x, ref_acts = Xn, []
    for li in range(4):
        s = st.layers[li][2]
        x = stack.selu_numpy(oracle.forward(Pn, x, w1[li], (s, s, s), VOX))
        ref_acts.append(x)
    head_act = stack.selu_numpy(oracle.forward(Pn, np.concatenate(ref_acts, axis=2), w1[4], (1, 1, 1), VOX))
    r = seg_head_ref(head_act, labels, points=1)
    e = rel(acts[4].cpu().numpy(), head_act)
    loss_bound = head_factor * max(1.0, float(np.abs(head_act).max()) + np.log(NCLS)) * R + tol_a * R
    print("act %.3e (tol %.0e); loss %.6f ref %.6f diff %.3e bound %.3e; step 1's loss %.6f"
          % (e, tol_a, float(loss2), r["loss"], abs(float(loss2) - r["loss"]), loss_bound, float(loss1)))
    assert abs(float(loss2) - float(loss1)) > 10 * loss_bound                # the update matters
    assert e <= tol_a
    assert abs(float(loss2) - r["loss"]) <= loss_bound
