"""The Morton order on the device (-m gpu): prestep.sort_order_morton / sort_point_cloud_morton(2) and the fused batch
provider with sort_method="morton" against the numpy statement of the definition (tests/morton_ref.py).

Bounds: none.  The quantisation is a fixed sequence of IEEE double operations on both sides and the rest is integer
work, so every comparison of orders is np.array_equal on int32, and every comparison of gathered rows is bit for bit."""
import numpy as np
import pytest

from pointwise_amd import synth
from tests import morton_ref as ref


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def T(a, dev):
    import torch
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else a.copy()).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows9():
    xyz = synth.room_like(2, 517, 31)
    return np.ascontiguousarray(synth.features(2, 517, 9, 32, points=xyz))


BATCHES = {
    "uniform_cube_3x300": lambda: synth.uniform_cube(3, 300, 21),                 # not a power of two: padding keys
    "modelnet_like_2x2048": lambda: synth.modelnet_like(2, 2048, 22),
    "room_like_1x8192": lambda: synth.room_like(1, 8192, 23),                     # the limit: 64 KB of keys
    "lattice_2x2048": lambda: synth.lattice(2, 2048, seed=4),                     # 128 and 134 ties, the far corner's code
    "1x1": lambda: np.array([[[0.5, -1.0, 2.0]]], dtype=np.float32),
    "all_equal_33": lambda: np.full((1, 33, 3), -0.3, dtype=np.float32),
    "nonfinite": lambda: ref.nonfinite_cloud()[None],
    "row_floats_9": _rows9,                                                       # the row stride
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_sort_order_morton(dev, name):
    from pointwise_amd import prestep
    batch = BATCHES[name]()
    assert batch.dtype == np.float32
    got = prestep.sort_order_morton(T(batch, dev)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref.batch_order(batch))
    if name == "all_equal_33":
        assert got[0].tolist() == list(range(33))
    if name == "nonfinite":
        assert got[0, -3:].tolist() == [3, 10, 20]


@pytest.mark.gpu
def test_limits(dev):
    import torch
    from pointwise_amd import prestep
    from pointwise_amd.conv3p_op import Conv3pRuntimeError
    with pytest.raises(Conv3pRuntimeError):
        prestep.sort_order_morton(torch.zeros((1, 8193, 3), device=dev))          # unsupported, says so
    assert prestep.sort_point_cloud_morton(torch.zeros((0, 5, 3), device=dev)).shape == (0, 5, 3)


@pytest.mark.gpu
def test_sort_point_cloud_morton_gathers_rows_and_attributes(dev):
    from pointwise_amd import prestep
    rows = _rows9()
    order = ref.batch_order(rows)
    got = prestep.sort_point_cloud_morton(T(rows, dev)).cpu().numpy()
    assert np.array_equal(bits(got), bits(ref.gather(rows, order)))
    rng = np.random.default_rng(33)
    for attr in (rng.integers(0, 41, size=(2, 517)).astype(np.int64), rng.integers(0, 250, size=(2, 517)).astype(np.uint8),
                 rng.standard_normal((2, 517, 5)).astype(np.float32)):
        s, a = prestep.sort_point_cloud_morton2(T(rows, dev), T(attr, dev))
        assert np.array_equal(bits(s.cpu().numpy()), bits(got))
        assert a.cpu().numpy().dtype == attr.dtype and np.array_equal(a.cpu().numpy(), ref.gather(attr, order))
    lat = synth.lattice(2, 2048, seed=4)                                           # ties: the earlier row first
    got = prestep.sort_point_cloud_morton(T(lat, dev)).cpu().numpy()
    assert np.array_equal(bits(got), bits(ref.gather(lat, ref.batch_order(lat))))


def dataset(S, Nsrc, K, seed):
    rng = np.random.default_rng(seed)
    xyz = synth.room_like(S, Nsrc, seed)
    d = np.concatenate([xyz, rng.standard_normal((S, Nsrc, K - 3)).astype(np.float32)], axis=2)
    d[0, 5, 0:3] = d[0, 9, 0:3]                                                    # a tie in sample 0
    return np.ascontiguousarray(d)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Nsrc,N,K,B", [(5, 320, 300, 3, 4), (3, 2048, 2048, 9, 2)])
def test_fused_provider_without_augmentation(dev, S, Nsrc, N, K, B):
    from pointwise_amd import provider
    data = dataset(S, Nsrc, K, 40 + K)
    lab = np.random.default_rng(41).integers(0, 250, size=(S, Nsrc)).astype(np.uint8)
    perm = np.array([1, 0] + list(range(S - 1, 0, -1)), dtype=np.int32)
    start = 1
    samples = perm[start:start + B]                                                # sample 0 (the tie), then S - 1, S - 2 ..
    pts, inp, labels, bad, rnd = provider.assemble_batch(T(data, dev), T(lab, dev), B, num_points=N, perm=T(perm, dev),
                                                         start=start, sort_cloud=True, sort_method="morton",
                                                         return_randoms=True)
    src = data[samples][:, 0:N]
    order = rnd["order"].cpu().numpy()
    assert order.dtype == np.int32 and np.array_equal(order, ref.batch_order(src))
    want = ref.gather(src, order)
    assert np.array_equal(bits(inp.cpu().numpy()), bits(want))
    assert np.array_equal(bits(pts.cpu().numpy()), bits(want[:, :, 0:3]))
    assert np.array_equal(labels.cpu().numpy(), ref.gather(lab[samples][:, 0:N], order).astype(np.int32))
    assert int(bad) == 0
    # the method is inert without sort_cloud
    flat = provider.assemble_batch(T(data, dev), T(lab, dev), B, num_points=N, perm=T(perm, dev), start=start,
                                   sort_method="morton")
    assert np.array_equal(bits(flat[1].cpu().numpy()), bits(src))


@pytest.mark.gpu
def test_fused_provider_orders_the_values_it_writes(dev):
    """Rotation and jitter drawn on the device: whatever the last ulp of the augmentation, the order must be the Morton
    order of the augmented cloud as written to `points`."""
    import torch
    from pointwise_amd import prestep, provider
    S, N, B = 4, 300, 4
    data = dataset(S, N, 3, 50)
    lab = np.arange(S, dtype=np.int64)
    perm = np.arange(S)[::-1].astype(np.int32).copy()
    d_t, l_t, p_t = T(data, dev), T(lab, dev), T(perm, dev)
    kw = dict(perm=p_t, rotate=True, jitter=True, sort_cloud=True, sort_method="morton", seed=77, step=(1 << 33) + 9)
    pts, inp, labels, bad, rnd = provider.assemble_batch(d_t, l_t, B, return_randoms=True, **kw)
    keep = [t.clone() for t in (pts, inp, labels, rnd["order"])]
    order = rnd["order"].cpu().numpy()
    p = pts.cpu().numpy()
    aug = np.empty_like(p)
    for b in range(B):
        assert sorted(order[b].tolist()) == list(range(N))
        aug[b, order[b]] = p[b]                                                    # un-sort: the cloud the kernel keyed on
    assert np.abs(aug - data[perm[:B]]).max() > 0.01                              # it was augmented
    assert np.array_equal(order, ref.batch_order(aug))
    assert labels.cpu().tolist() == lab[perm[:B]].tolist() and int(bad) == 0 and torch.equal(pts, inp)
    # with the randoms handed in: the composition of the pre-step's calls, bit for bit
    angles = np.random.default_rng(51).uniform(0, 2 * np.pi, size=B)
    noise = T(np.random.default_rng(52).standard_normal((B, N, 3)), dev)
    cs = T(np.stack([np.cos(angles), np.sin(angles)], axis=1), dev)
    given = dict(perm=p_t, rotate=True, jitter=True, sort_cloud=True, sort_method="morton", cos_sin=cs, noise=noise)
    fused = provider.assemble_batch(d_t, l_t, B, return_randoms=True, **given)
    fused_keep = [t.clone() for t in fused[:3]] + [fused[4]["order"].clone()]
    augmented = prestep.rotate_and_jitter(T(data[perm[:B]], dev), angles, noise=noise)
    assert torch.equal(fused_keep[0], prestep.sort_point_cloud_morton(augmented))
    assert torch.equal(fused_keep[3], prestep.sort_order_morton(augmented))
    xyz = provider.assemble_batch(d_t, l_t, B, **{**given, "sort_method": "xyz"})[0]
    assert torch.equal(xyz, prestep.sort_point_cloud_xyz(augmented)) and not torch.equal(xyz, fused_keep[0])
    # and both calls equal themselves on a second run
    again = provider.assemble_batch(d_t, l_t, B, return_randoms=True, **given)
    for a, b in zip(fused_keep, list(again[:3]) + [again[4]["order"]]):
        assert torch.equal(a, b)
    twice = provider.assemble_batch(d_t, l_t, B, return_randoms=True, **kw)
    for a, b in zip(keep, list(twice[:3]) + [twice[4]["order"]]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_a_sample_index_outside_the_data_set_in_a_morton_batch(dev):
    from pointwise_amd import provider
    S, N, K = 3, 300, 9
    data = dataset(S, N, K, 60)
    lab = np.random.default_rng(61).integers(0, 13, size=(S, N)).astype(np.uint8)
    perm = np.array([1, S, 2], dtype=np.int32)
    pts, inp, labels, bad, rnd = provider.assemble_batch(T(data, dev), T(lab, dev), 3, perm=T(perm, dev), sort_cloud=True,
                                                         sort_method="morton", return_randoms=True)
    order = rnd["order"].cpu().numpy()
    assert int(bad) == 1
    assert not pts[1].cpu().numpy().any() and not inp[1].cpu().numpy().any() and (labels[1].cpu().numpy() == -1).all()
    assert order[1].tolist() == list(range(N))
    for b, s in ((0, 1), (2, 2)):
        assert np.array_equal(order[b], ref.order(data[s]))
        assert np.array_equal(bits(inp[b].cpu().numpy()), bits(data[s][order[b]]))
        assert np.array_equal(labels[b].cpu().numpy(), lab[s][order[b]].astype(np.int32))


@pytest.mark.gpu
def test_batch_provider_with_a_sort_method(dev):
    import torch
    from pointwise_amd import provider
    S, B, N = 6, 2, 190
    data = dataset(S, 200, 3, 70)
    lab = (np.arange(S) + 10).astype(np.uint8)
    d_t, l_t = T(data, dev), T(lab, dev)

    def epochs(bp, **kw):
        count = 0
        for epoch in range(2):
            assert bp.epoch == epoch and bp.num_batches == 3
            while True:
                got = bp.get_batch_point_cloud()
                want = provider.assemble_batch(d_t, l_t, B, N, bp.permutation, bp.cur_batch * B, rotate=True, jitter=True,
                                               sort_cloud=True, seed=9, step=bp.step, **kw)
                for a, b in zip(got, want[:3]):
                    assert torch.equal(a, b)
                count += 1
                if not bp.has_next_batch():
                    break
                bp.next_batch()
            bp.next_epoch()
        assert count == 6
        return got[0].clone()

    mo = provider.BatchProvider(data, lab, B, num_points=N, training=True, sort_cloud=True, seed=9, device=dev,
                                sort_method="morton")
    assert mo.sort_method == "morton" and mo.rotate and mo.jitter
    assert mo.state_dict() == {"seed": 9, "epoch": 0, "cur_batch": 0}                 # a setting, not state
    last_morton = epochs(mo, sort_method="morton")
    # the default method is the parent commit's call: assemble_batch(sort_cloud=True) without the new keyword
    xy = provider.BatchProvider(data, lab, B, num_points=N, training=True, sort_cloud=True, seed=9, device=dev)
    assert xy.sort_method == "xyz"
    last_xyz = epochs(xy)
    assert not torch.equal(last_morton, last_xyz)
    # inert while sort_cloud is false
    a = provider.BatchProvider(data, lab, B, num_points=N, training=False, device=dev, sort_method="morton")
    b = provider.BatchProvider(data, lab, B, num_points=N, training=False, device=dev)
    for x, y in zip(a.get_batch_point_cloud(), b.get_batch_point_cloud()):
        assert torch.equal(x, y)
