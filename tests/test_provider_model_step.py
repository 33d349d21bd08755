"""The batch provider in front of the two models' training steps (-m gpu): three batches from BatchProvider give
bitwise the same loss and the same first-layer grad_filter as the same batches assembled by the composed path --
torch indexing, prestep.rotate_and_jitter with the provider's exported cos_sin / noise, prestep.sort_order_xyz, the
gathers, the [:, :, 0:3] slice and the label cast.  Every piece of that path is deterministic and the arithmetic is
shared (augment_point, the sort network), so there is nothing to bound: equal bits."""
import numpy as np
import pytest

from pointwise_amd import synth


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def composed(pv, cur_batch, rnd):
    """The batch of the issue's list, from the provider's resident tensors and exported randoms."""
    import torch
    from pointwise_amd import prestep
    B = pv.batch_size
    idx = pv.permutation[cur_batch * B:(cur_batch + 1) * B].long()
    rows = pv.data[idx][:, 0:pv.num_points, :]
    xyz = rows[:, :, 0:3].contiguous()
    if pv.rotate or pv.jitter:
        cs = rnd["cos_sin"].cpu().numpy()
        xyz = prestep._augment(xyz, cs, rnd["noise"], pv.sigma, pv.clip)
    rows = torch.cat([xyz, rows[:, :, 3:]], dim=2).contiguous()
    lab = pv.labels[idx]
    if lab.dim() == 2:
        lab = lab[:, 0:pv.num_points].contiguous()
    if pv.sort_cloud:
        order = prestep.sort_order_xyz(rows)
        rows = prestep._gather(rows, order)
        if lab.dim() == 2:
            lab = prestep._gather(lab, order)
    return rows[:, :, 0:3].contiguous(), rows, lab.to(torch.int32)


@pytest.mark.gpu
def test_classification_steps_from_the_provider(dev):
    import torch
    from pointwise_amd import head, provider, stack
    S, B, N, NCLS = 6, 2, 256, 40
    data = synth.modelnet_like(S, N, seed=3100)
    labels = np.random.default_rng(3101).integers(0, NCLS, size=S).astype(np.uint8)
    pv = provider.BatchProvider(data, labels, B, training=True, sort_cloud=True, seed=12, device=dev)
    assert pv.num_batches == 3 and pv.rotate and pv.jitter
    mask = torch.from_numpy((np.random.default_rng(3102).random((B, 512)) < 0.5).astype(np.float32)).to(dev)

    def step(points, inp, lab):
        st = stack.Conv3pStack(3, None, device=dev, seed=3103)
        hd = head.ClassificationHead(N, num_class=NCLS, device=dev, seed=7)
        feat = torch.cat(list(st.forward(points, inp)), dim=2).contiguous()
        loss, dfeat = hd.forward_backward(feat, lab, keep_mask=mask)
        st.backward(dfeat)
        return float(loss), st.grad_views[0].clone()

    for k in range(3):
        points, inp, lab, rnd = pv.get_batch_point_cloud(return_randoms=True)
        c_points, c_inp, c_lab = composed(pv, k, rnd)
        assert torch.equal(points, c_points) and torch.equal(inp, c_inp) and torch.equal(lab, c_lab)
        got, want = step(points, inp, lab), step(c_points, c_inp, c_lab)
        assert got[0] == want[0] and np.isfinite(got[0]) and torch.equal(got[1], want[1])
        assert float(got[1].abs().max()) > 0
        if pv.has_next_batch():
            pv.next_batch()
    assert int(pv.bad_index) == 0 and not pv.has_next_batch()


@pytest.mark.gpu
def test_segmentation_steps_from_the_provider(dev):
    import torch
    from pointwise_amd import provider, stack
    from pointwise_amd.seg_head import SegmentationHead
    S, B, N, K, NCLS = 6, 2, 256, 9, 13
    P = synth.room_like(S, N, seed=3200)
    data = synth.features(S, N, K, 3201, points=P)
    data[:, :, 0:3] = P
    labels = np.random.default_rng(3202).integers(0, NCLS, size=(S, N)).astype(np.uint8)
    pv = provider.BatchProvider(data, labels, B, training=True, sort_cloud=True, seed=13, device=dev)
    assert pv.num_batches == 3 and not pv.rotate and not pv.jitter

    def step(points, inp, lab):
        st = stack.Conv3pStack(K, NCLS, device=dev, seed=3203)
        hd = SegmentationHead(NCLS, device=dev)
        acts = st.forward(points, inp)
        loss, dact = hd.loss(acts[4], lab)
        st.backward([dact])
        return float(loss), st.grad_views[0].clone()

    for k in range(3):
        points, inp, lab, rnd = pv.get_batch_point_cloud(return_randoms=True)
        c_points, c_inp, c_lab = composed(pv, k, rnd)
        assert torch.equal(points, c_points) and torch.equal(inp, c_inp) and torch.equal(lab, c_lab)
        assert torch.equal(points, inp[:, :, 0:3])
        got, want = step(points, inp, lab), step(c_points, c_inp, c_lab)
        assert got[0] == want[0] and np.isfinite(got[0]) and torch.equal(got[1], want[1])
        assert float(got[1].abs().max()) > 0
        if pv.has_next_batch():
            pv.next_batch()
    assert int(pv.bad_index) == 0
