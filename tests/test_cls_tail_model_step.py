"""tests/test_model_step.py's graph -- provider pre-step, the four-layer conv3p stack with its concat, the dense head,
softmax cross-entropy, forward and backward -- with ClassificationHead.forward_backward (the fused tail) in place of
forward / loss / backward: the same inputs, the same CPU restatement, the same bounds.  Then the same step with a
MomentumOptimizer over all eight parameters, and evaluate() on the batch."""
import numpy as np
import pytest

from oracle import head_numpy, oracle, prestep_numpy

TOL = 2e-4
VOX = 0.1
B, N, NCLS = 3, 192, 40


def rel(got, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(1.0, np.abs(want).max()))


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def batch():
    from pointwise_amd import synth
    rng = np.random.default_rng(21)
    raw = synth.modelnet_like(B, N, seed=1500)
    angles = rng.uniform(0, 2 * np.pi, size=B)
    noise = rng.standard_normal((B, N, 3))
    labels = rng.integers(0, NCLS, size=B)
    mask = (rng.random((B, 512)) < 0.5).astype(np.float32)
    return raw, angles, noise, labels, mask


def reference(stack, st, Pn, params, labels, mask):
    """The CPU composition of test_model_step.py: -> (concat, head dict, dx, [dW of the four filters])."""
    filters = [f.cpu().numpy() for f in st.filters]
    x, ref_acts = Pn, []
    for li in range(4):
        s = st.layers[li][2]
        x = stack.selu_numpy(oracle.forward(Pn, x, filters[li], (s, s, s), VOX))
        ref_acts.append(x)
    concat = np.concatenate(ref_acts, axis=2)
    r = head_numpy.head_forward_backward(concat, *params, labels, 0.5, mask.astype(np.float64))
    g = np.asarray(r["dfeat"], dtype=np.float32).reshape(B, N, 36)
    carry, dws = None, [None] * 4
    for li in (3, 2, 1, 0):
        s = st.layers[li][2]
        up = g[:, :, 9 * li:9 * li + 9]
        gi = stack.selu_grad_numpy(ref_acts[li], np.ascontiguousarray(up if carry is None else up + carry))
        carry, dws[li] = oracle.backward(gi, Pn, ref_acts[li - 1] if li > 0 else Pn, filters[li], (s, s, s), VOX)
    return concat, r, g, carry, dws


@pytest.mark.gpu
def test_classification_model_training_step_with_the_fused_tail(dev):
    import torch
    from pointwise_amd import head, prestep, stack
    raw, angles, noise, labels, mask = batch()
    P = prestep.rotate_and_jitter(torch.from_numpy(raw).to(dev), angles=angles, noise=torch.from_numpy(noise).to(dev))
    st = stack.Conv3pStack(3, None, device=dev, seed=1501)
    feat = torch.cat(list(st.forward(P, P)), dim=2).contiguous()
    hd = head.ClassificationHead(N, num_class=NCLS, device=dev, seed=7)
    loss, dfeat = hd.forward_backward(feat, torch.from_numpy(labels).to(dev), keep_mask=torch.from_numpy(mask).to(dev))
    dx, fused = st.backward(dfeat)

    Pn = prestep_numpy.jitter_point_cloud(prestep_numpy.rotate_point_cloud_by_angles(raw, angles), noise)
    assert rel(P.cpu().numpy(), Pn) <= 1e-6
    Pn = P.cpu().numpy()
    concat, r, g, carry, dws = reference(stack, st, Pn, [p.cpu().numpy() for p in hd.parameters()], labels, mask)
    assert rel(feat.cpu().numpy(), concat) <= 2e-5
    assert rel(hd.logits.cpu().numpy(), r["logits"]) <= TOL
    assert abs(float(loss) - r["loss"]) <= TOL * max(1.0, abs(r["loss"]))
    assert rel(dfeat.cpu().numpy().reshape(B, N, 36), g) <= TOL
    assert rel(hd.dW1.cpu().numpy(), r["dW1"]) <= TOL and rel(hd.dW2.cpu().numpy(), r["dW2"]) <= TOL
    assert rel(dx.cpu().numpy(), carry) <= TOL
    assert rel(fused.cpu().numpy(), np.concatenate([d.reshape(-1) for d in dws])) <= TOL

    # evaluate(): no dropout; np.argmax of the reference logits wherever its top-two margin is clear
    pred, cnt = hd.evaluate(feat, torch.from_numpy(labels).to(dev))
    par = [p.cpu().numpy() for p in hd.parameters()]
    fc1 = head_numpy.fully_connected(concat.reshape(B, -1), par[0], par[1])
    ev = head_numpy.fully_connected(fc1, par[2], par[3])
    top = np.sort(ev, axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-3
    assert clear.mean() >= 0.9
    assert np.array_equal(pred.cpu().numpy()[clear], np.argmax(ev, axis=1)[clear])
    assert int(cnt["seen"].sum()) == B and int(cnt["invalid"]) == 0


@pytest.mark.gpu
def test_one_fused_optimizer_step_over_all_eight_parameters(dev):
    """Momentum from zero accumulators: param' = param - lr * grad.  Every parameter is held against the numpy rule on the
    REFERENCE gradient: |param' - (param - lr * grad_ref)| <= 2e-4 * lr * max(1, max|grad_ref|) -- the gradients' own
    bound of 2e-4 * max(1, max|grad_ref|), scaled by the learning rate that multiplies them.  lr = 0.5 keeps that bound
    three orders of magnitude above the fp32 rounding of the stored parameters (2^-24 * |param|, |param| < 4)."""
    import torch
    from pointwise_amd import head, prestep, stack
    from pointwise_amd.optim import MomentumOptimizer
    LR, MOM = 0.5, 0.9
    raw, angles, noise, labels, mask = batch()
    P = prestep.rotate_and_jitter(torch.from_numpy(raw).to(dev), angles=angles, noise=torch.from_numpy(noise).to(dev))
    st = stack.Conv3pStack(3, None, device=dev, seed=1501)
    hd = head.ClassificationHead(N, num_class=NCLS, device=dev, seed=7)
    params = list(st.filters) + hd.parameters()
    old = [p.cpu().numpy().astype(np.float64) for p in params]
    assert max(np.abs(p).max() for p in old) < 4.0
    concat, r, g, carry, dws = reference(stack, st, P.cpu().numpy(), old[4:], labels, mask)
    opt = MomentumOptimizer(params, LR, MOM)
    feat = torch.cat(list(st.forward(P, P)), dim=2).contiguous()
    loss, dfeat = hd.forward_backward(feat, torch.from_numpy(labels).to(dev), optimizer=opt,
                                      keep_mask=torch.from_numpy(mask).to(dev))
    assert opt.global_step == 0
    st.backward(dfeat)
    grads = list(st.grad_views) + hd.gradients()
    assert grads[4:] == [None, None, None, None]
    opt.step(grads)
    assert opt.global_step == 1
    assert abs(float(loss) - r["loss"]) <= TOL * max(1.0, abs(r["loss"]))
    ref_grads = dws + [r["dW1"], r["db1"], r["dW2"], r["db2"]]
    for i, (p, w0, gr) in enumerate(zip(params, old, ref_grads)):
        want = w0 - LR * gr.reshape(w0.shape)
        err = np.abs(p.cpu().numpy().astype(np.float64) - want).max()
        assert err <= TOL * LR * max(1.0, np.abs(gr).max()), (i, err)
        assert rel(opt.accums[i].cpu().numpy(), gr.reshape(w0.shape)) <= TOL, i
