"""The guarded optimizer inside the two models' training steps, at the sizes of tests/test_cls_tail_model_step.py
(B = 3, N = 192, 40 classes) and tests/test_seg_model_step.py (B = 2, N = 256, 13 classes).

An optimizer that clips, skips or uses Nesterov's rule is not `fusable`: ClassificationHead.forward_backward(optimizer=)
writes all four gradients instead of updating inside the gradient passes, and step() updates all eight parameters.
That step is held, bit for bit, against the step composed by hand on an identically seeded model, and against the numpy
rule on the device's own gradients.  Then a batch with one Inf in its features, and a segmentation batch with one NaN
point weight, must leave every parameter as it was and cost exactly one step."""
import numpy as np
import pytest

from tests.optim_guarded_ref import clip_scale_ref, guarded_step_ref

LR, MOM = 0.05, 0.9
B, N, NCLS = 3, 192, 40


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
def test_classification_step_with_clipping_and_nesterov_then_a_skipped_batch(dev):
    import torch
    from pointwise_amd import head, prestep, stack, synth
    from pointwise_amd.optim import MomentumOptimizer, grad_sumsq
    rng = np.random.default_rng(21)
    raw = synth.modelnet_like(B, N, seed=1500)
    angles = rng.uniform(0, 2 * np.pi, size=B)
    noise = rng.standard_normal((B, N, 3))
    lab = torch.from_numpy(rng.integers(0, NCLS, size=B)).to(dev)
    keep = torch.from_numpy((rng.random((B, 512)) < 0.5).astype(np.float32)).to(dev)
    P = prestep.rotate_and_jitter(torch.from_numpy(raw).to(dev), angles=angles, noise=torch.from_numpy(noise).to(dev))

    def model():
        st = stack.Conv3pStack(3, None, device=dev, seed=1501)
        hd = head.ClassificationHead(N, num_class=NCLS, device=dev, seed=7)
        return st, hd, list(st.filters) + hd.parameters()

    def gradients(st, hd, X, optimizer=None):
        feat = torch.cat(list(st.forward(P, X)), dim=2).contiguous()
        loss, dfeat = hd.forward_backward(feat, lab, optimizer=optimizer, keep_mask=keep)
        st.backward(dfeat)
        return loss, list(st.grad_views) + hd.gradients()

    # a first pass measures the norm; clip_norm is half of it
    st0, hd0, _ = model()
    _, g0 = gradients(st0, hd0, P)
    s0 = grad_sumsq(g0).cpu().numpy()
    assert s0[1] == 0 and s0[0] > 0
    clip = 0.5 * float(np.sqrt(s0[0]))

    # A: through forward_backward(optimizer=);  Bm: composed by hand without it
    stA, hdA, pA = model()
    stB, hdB, pB = model()
    w0 = [p.cpu().numpy().copy() for p in pA]
    optA = MomentumOptimizer(pA, LR, MOM, use_nesterov=True, clip_norm=clip)
    optB = MomentumOptimizer(pB, LR, MOM, use_nesterov=True, clip_norm=clip)
    assert optA.fusable is False
    for step in range(2):
        _, gA = gradients(stA, hdA, P, optimizer=optA)
        assert None not in hdA.gradients() and len(gA) == 8 and None not in gA
        before = [(p.cpu().numpy().copy(), a.cpu().numpy().copy()) for p, a in zip(pA, optA.accums)]
        gA_host = [g.cpu().numpy().copy() for g in gA]
        optA.step(gA)
        _, gB = gradients(stB, hdB, P)
        optB.step(gB)
        assert optA.global_step == step + 1
        for i in range(8):
            assert torch.equal(pA[i], pB[i]) and torch.equal(optA.accums[i], optB.accums[i]), (step, i)
        assert torch.equal(optA.grad_stats, optB.grad_stats)
        # ... and the rule itself, from the device's gradients and the device's norm
        st_host = optA.grad_stats.cpu().numpy()
        scale = clip_scale_ref(st_host[0], clip, np.float32)
        print("step", step, "norm", float(np.sqrt(st_host[0])), "clip", clip, "scale", scale)
        assert st_host[1] == 0
        if step == 0:
            assert 0.49 < scale < 0.51                                        # the gradients of the measuring pass
        for i in range(8):
            w, a = guarded_step_ref(before[i][0], gA_host[i].reshape(before[i][0].shape), before[i][1], LR, MOM,
                                    nesterov=True, scale=scale)
            assert same(pA[i].cpu().numpy(), w) and same(optA.accums[i].cpu().numpy(), a), (step, i)
    assert all(np.abs(p.cpu().numpy() - w).max() > 0 for p, w in zip(pA, w0))

    # one Inf in the input features: the step changes nothing
    skipper = MomentumOptimizer(pA, LR, MOM, use_nesterov=True, clip_norm=clip, skip_nonfinite=True)
    skipper.load_state_dict(optA.state_dict())
    skipper.skip_nonfinite = True
    X = P.clone()
    X[1, 7, 2] = float("inf")
    loss, g = gradients(stA, hdA, X, optimizer=skipper)
    assert None not in g
    held = [(p.clone(), a.clone()) for p, a in zip(pA, skipper.accums)]
    skipper.step(g)
    for i in range(8):
        assert torch.equal(pA[i], held[i][0]) and torch.equal(skipper.accums[i], held[i][1]), i
    assert int(skipper.skipped_steps) == 1 and skipper.grad_stats.cpu().numpy()[1] > 0
    assert all(bool(torch.isfinite(p).all()) for p in pA)
    # the next clean batch trains on
    _, g = gradients(stA, hdA, P, optimizer=skipper)
    skipper.step(g)
    assert int(skipper.skipped_steps) == 1 and skipper.global_step == 4
    assert not torch.equal(pA[4], held[4][0]) and all(bool(torch.isfinite(p).all()) for p in pA)


@pytest.mark.gpu
def test_segmentation_step_with_a_nan_point_weight_is_skipped(dev):
    import torch
    from pointwise_amd import stack, synth
    from pointwise_amd.optim import MomentumOptimizer
    from pointwise_amd.seg_head import SegmentationHead
    Bs, Ns, CIN, C = 2, 256, 9, 13
    Pn = synth.room_like(Bs, Ns, seed=2600).astype(np.float32)
    Xn = synth.features(Bs, Ns, CIN, 2601, points=Pn, dtype=np.float32)
    labels = np.random.default_rng(2602).integers(0, C, size=(Bs, Ns))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P, X, lab = t(Pn), t(Xn), t(labels)
    st = stack.Conv3pStack(CIN, C, device=dev, dtype=torch.float32, seed=2603)
    hd = SegmentationHead(C, device=dev)
    opt = MomentumOptimizer(st.filters, 0.01, MOM, skip_nonfinite=True)
    assert len(st.filters) == 5
    pw = torch.ones((Bs, Ns), dtype=torch.float32, device=dev)
    pw[1, 100] = float("nan")
    acts = st.forward(P, X)
    _, dact = hd.loss(acts[4], lab, global_points=1, point_weights=pw)
    st.backward([dact])
    held = [f.clone() for f in st.filters]
    opt.step(st.grad_views)
    assert all(torch.equal(f, h) for f, h in zip(st.filters, held))
    assert all(not bool(a.any()) for a in opt.accums)                         # still the zeros they started as
    assert int(opt.skipped_steps) == 1 and opt.grad_stats.cpu().numpy()[1] > 0
    # the next clean step: finite, and a real update
    acts = st.forward(P, X)
    _, dact = hd.loss(acts[4], lab, global_points=1)
    st.backward([dact])
    g = [v.cpu().numpy().copy() for v in st.grad_views]
    opt.step(st.grad_views)
    assert int(opt.skipped_steps) == 1 and opt.grad_stats.cpu().numpy()[1] == 0
    for i in range(5):
        w, a = guarded_step_ref(held[i].cpu().numpy(), g[i], np.zeros_like(g[i]), 0.01, MOM)
        assert same(st.filters[i].cpu().numpy(), w) and same(opt.accums[i].cpu().numpy(), a), i
        assert np.isfinite(w).all() and np.abs(w - held[i].cpu().numpy()).max() > 0
    loss, _ = hd.loss(st.forward(P, X)[4], lab, global_points=1)
    assert np.isfinite(float(loss))
