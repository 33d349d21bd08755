"""One training step of the reference's segmentation model (scene_seg/pointcnn_scene_seg_acsd.py:43-71) assembled from
this repository's pieces -- the five-layer conv3p stack, the fused loss head, the stack's backward -- against the CPU
restatements composed the same way (oracle conv3p + numpy SELU + tests/seg_head_ref.py).  The segmentation twin of
test_model_step.py.  What is checked beyond the per-piece tests: the gradient that leaves SegmentationHead.loss is the
one Conv3pStack.backward([dact]) expects (layout, scale, and the SELU of layer 5 applied by the stack, not the head).

global_points = 1 is deliberate: with the mean over B N = 512 points every gradient is far below 1, and the project's
rel() divides by max(1, max|ref|), so a wrong gradient would pass.  With the SUM the gradients are of order 1 -- but not
all above 1: |softmax - onehot| < 1 always (0.949 here), max|dx| is 0.383 and the smallest layer's max|dW| 0.439 on this
input (the fused dW buffer: 7.38).  So that no comparison is loosened by the max(1, .), rel() here divides by max|ref|
itself, and the test asserts that every reference gradient is of order 1 (dact >= 0.9, dx and every dW >= 0.25, the
fused buffer >= 1).

Tolerances are the chained-stack ones (tests/test_stack_descriptors.py): fp32 activations 2e-5,
dx and the fused dW buffer 5e-5; fp64 1e-11 (1e-12 per op over the chained ops).  Loss: the head's own bound
(test_seg_head.py) plus the activation tolerance times R -- the activations feeding the loss already differ by up to
that much per point, and with global_points = 1 the loss is a sum over R points."""
import numpy as np
import pytest

from oracle import oracle
from tests.seg_head_ref import seg_head_ref

VOX = 0.1
EPS = 2.0 ** -24
TOL = {np.float32: (2e-5, 5e-5, 8 * EPS), np.float64: (1e-11, 1e-11, 1e-12)}   # activations, dx / dW, head loss factor


def rel(got, want):
    """max |got - want| / max |want|: a true relative error (never the absolute one of the project's max(1, .) form)."""
    want = np.asarray(want)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from pointwise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_segmentation_model_training_step(dev, dt):
    import torch
    from pointwise_amd import stack, synth
    from pointwise_amd.seg_head import SegmentationHead
    B, N, CIN, NCLS = 2, 256, 9, 13
    R = B * N
    tol_a, tol_g, head_factor = TOL[dt]
    P = synth.room_like(B, N, seed=2600).astype(dt)
    X = synth.features(B, N, CIN, 2601, points=P, dtype=dt)
    labels = np.random.default_rng(2602).integers(0, NCLS, size=(B, N))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # ---- device: stack -> loss head -> stack backward
    st = stack.Conv3pStack(CIN, NCLS, device=dev, dtype=torch.float32 if dt == np.float32 else torch.float64, seed=2603)
    acts = st.forward(t(P), t(X))
    hd = SegmentationHead(NCLS, device=dev)
    loss, dact, pred = hd.loss(acts[4], t(labels), global_points=1, need_pred=True)
    dx, fused = st.backward([dact])

    # ---- CPU: the same graph from the restatements
    filters = [f.cpu().numpy() for f in st.filters]
    x, ref_acts = X, []
    for li in range(4):
        s = st.layers[li][2]
        x = stack.selu_numpy(oracle.forward(P, x, filters[li], (s, s, s), VOX))
        ref_acts.append(x)
    concat = np.concatenate(ref_acts, axis=2)
    head = stack.selu_numpy(oracle.forward(P, concat, filters[4], (1, 1, 1), VOX))
    r = seg_head_ref(head, labels, points=1)
    g = stack.selu_grad_numpy(head, np.ascontiguousarray(r["dact"].astype(dt)))
    dconcat, dw4 = oracle.backward(g, P, concat, filters[4], (1, 1, 1), VOX)
    carry, dws = None, [None] * 4 + [dw4]
    for li in (3, 2, 1, 0):                                           # as stack.py's op-by-op backward splits dconcat
        s = st.layers[li][2]
        up = dconcat[:, :, 9 * li:9 * li + 9]
        gi = stack.selu_grad_numpy(ref_acts[li], np.ascontiguousarray(up if carry is None else up + carry))
        carry, dws[li] = oracle.backward(gi, P, ref_acts[li - 1] if li > 0 else X, filters[li], (s, s, s), VOX)
    ref_fused = np.concatenate([d.reshape(-1) for d in dws])

    # the sum (not the mean) keeps every compared gradient of order 1
    assert np.abs(r["dact"]).max() >= 0.9 and np.abs(carry).max() >= 0.25 and np.abs(ref_fused).max() >= 1.0
    for dw in dws:
        assert np.abs(dw).max() >= 0.25

    for li, (a, ra) in enumerate(zip(acts, ref_acts + [head])):
        e = rel(a.cpu().numpy(), ra) * min(1.0, float(np.abs(ra).max()))   # activations: on the scale max(1, max|ref|)
        print("act", li, e)
        assert e <= tol_a, ("activation", li, e)
    loss_bound = head_factor * max(1.0, float(np.abs(head).max()) + np.log(NCLS)) * R + tol_a * R
    print("loss", float(loss), r["loss"], abs(float(loss) - r["loss"]), loss_bound)
    assert abs(float(loss) - r["loss"]) <= loss_bound
    e_d, e_x, e_w = rel(dact.cpu().numpy(), r["dact"]), rel(dx.cpu().numpy(), carry), rel(fused.cpu().numpy(), ref_fused)
    print("dact %.3e dx %.3e dW %.3e" % (e_d, e_x, e_w))
    assert e_d <= tol_g and e_x <= tol_g and e_w <= tol_g
    # pred / counters: wherever the reference's two largest activations are further apart than the activation tolerance
    srt = np.sort(head.astype(np.float64), axis=2)
    clear = (srt[:, :, -1] - srt[:, :, -2]) > 2 * tol_a * max(1.0, np.abs(head).max())
    assert clear.mean() > 0.9 and np.array_equal(pred.cpu().numpy()[clear], r["pred"][clear])
    cnt = hd.counts()
    assert int(cnt["invalid"]) == 0 and int(cnt["seen"].sum()) == R
    assert np.array_equal(cnt["seen"].cpu().numpy(), np.bincount(labels.reshape(-1), minlength=NCLS))
