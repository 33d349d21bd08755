"""The batch provider on the device (-m gpu): pointwise_amd.provider against the reference's own fixtures
(tests/golden/prestep_*.npz, explicit randoms), against the numpy restatement tests/provider_ref.py (assembly bit-exact
where there is no rotation; the device's draws within 1e-12 of the restated ones), and the provider class's epochs.

Bounds.  Rotation: ONE float32 ulp of the reference (test_prestep.py's bar: the reference's 3x3 product runs in BLAS in
float64, whose rounding in the 16th digit can move the float32 result by one ulp).  Jitter alone, sort, gather, label
cast: exact.  Drawn angles and normals: 1e-12 absolute against the restatement -- four orders of magnitude above what
two double-precision libms differ by on values below 7, four below what could move the float32 output (sigma * 1e-12
against an ulp of 4e-9 at 0.05)."""
import os

import numpy as np
import pytest

from pointwise_amd import synth
from tests import provider_ref as ref

G = os.path.join(os.path.dirname(__file__), "golden")
DRAW_BOUND = 1e-12


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.abs(a - b).max()) if a.size else 0


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


def cs_of(angles):
    return np.stack([np.cos(angles), np.sin(angles)], axis=1)


def dataset(S, Nsrc, K, seed):
    rng = np.random.default_rng(seed)
    xyz = synth.room_like(S, Nsrc, seed)
    return np.ascontiguousarray(np.concatenate([xyz, rng.standard_normal((S, Nsrc, K - 3)).astype(np.float32)], axis=2))


# ------------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.gpu
def test_augmentation_matches_the_reference_fixture(dev):
    from pointwise_amd import provider
    g = np.load(os.path.join(G, "prestep_augment.npz"))
    data, lab = T(g["points"], dev), T(np.arange(4, dtype=np.uint8), dev)
    cs, noise = T(cs_of(g["angles"]), dev), T(g["noise"], dev)
    pts, inp, labels, bad = provider.assemble_batch(data, lab, 4, rotate=True, jitter=True, cos_sin=cs, noise=noise)
    assert ulp_diff(pts.cpu().numpy(), g["fed"]) <= 1
    assert np.array_equal(inp.cpu().numpy(), pts.cpu().numpy())                       # K = 3: input == points
    assert labels.dtype.is_floating_point is False and labels.cpu().tolist() == [0, 1, 2, 3] and int(bad) == 0
    rot = provider.assemble_batch(data, lab, 4, rotate=True, cos_sin=cs)[0]
    assert ulp_diff(rot.cpu().numpy(), g["rotated"]) <= 1
    jit = provider.assemble_batch(T(g["rotated"], dev), lab, 4, jitter=True, noise=noise)[0]
    assert np.array_equal(jit.cpu().numpy(), g["fed"])                                # no matrix product: exact


@pytest.mark.gpu
def test_sort_matches_the_reference_fixtures(dev):
    from pointwise_amd import prestep, provider
    g = np.load(os.path.join(G, "prestep_sort.npz"))
    for name in ("generic", "lattice_unique"):
        src = g[name + "_in"]
        lab = T(np.zeros(src.shape[0], dtype=np.uint8), dev)
        pts, inp, _, bad, rnd = provider.assemble_batch(T(src, dev), lab, src.shape[0], sort_cloud=True, return_randoms=True)
        assert np.array_equal(pts.cpu().numpy(), g[name + "_sorted"]) and np.array_equal(inp.cpu().numpy(), g[name + "_sorted"])
        assert np.array_equal(rnd["order"].cpu().numpy(), prestep.sort_order_xyz(T(src, dev)).cpu().numpy())
    src = g["room9_labels_in"]
    pts, inp, lab, bad, rnd = provider.assemble_batch(T(src, dev), T(g["room9_labels_attr"], dev), 2, sort_cloud=True,
                                                      return_randoms=True)
    assert np.array_equal(inp.cpu().numpy(), g["room9_labels_sorted"])
    assert np.array_equal(pts.cpu().numpy(), g["room9_labels_sorted"][:, :, 0:3])
    assert np.array_equal(lab.cpu().numpy(), g["room9_labels_attr_sorted"].astype(np.int32))
    assert np.array_equal(rnd["order"].cpu().numpy(), prestep.sort_order_xyz(T(src, dev)).cpu().numpy())
    assert int(bad) == 0


# ------------------------------------------------------------------------------- assembly against the restatement
SHAPES = [(1, 1, 1, 3, 1), (5, 70, 63, 3, 3), (4, 257, 257, 9, 4), (6, 2053, 2048, 3, 2), (3, 4096, 4096, 9, 2),
          (2, 8192, 8192, 12, 1)]
_DATASETS = {}


def shared_dataset(S, Nsrc, K):
    """One data set per shape, computed once and never written to."""
    key = (S, Nsrc, K)
    if key not in _DATASETS:
        rng = np.random.default_rng(S * 1000 + K)
        d = dataset(S, Nsrc, K, 700 + Nsrc)
        if Nsrc >= 63:
            d[0, 5, 0:3] = d[0, 9, 0:3]                                  # equal keys: the tie goes to the source row
            d[0, 11, 0] = -0.0
            d[0, 12, 0] = 0.0
        d.setflags(write=False)
        _DATASETS[key] = (d, rng.integers(0, 250, size=S), rng.integers(0, 250, size=(S, Nsrc)),
                          rng.standard_normal((8, min(Nsrc, 8192), 3)))
    return _DATASETS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("sort_cloud", [False, True], ids=["flat", "sort"])
@pytest.mark.parametrize("S,Nsrc,N,K,B", SHAPES)
def test_assembly_is_bit_exact_without_rotation(dev, S, Nsrc, N, K, B, sort_cloud):
    """Jitter from a given noise, a perm with a repeated and a reversed index and start > 0, every label type, one per
    sample and one per point."""
    from pointwise_amd import provider
    data, lab_s, lab_p, noise_all = shared_dataset(S, Nsrc, K)
    perm = np.concatenate([[0, 0], np.arange(S)[::-1], np.arange(S)]).astype(np.int32)
    start = 1
    samples = perm[start:start + B]
    noise = np.ascontiguousarray(noise_all[:B, :N])
    d_t, perm_t, noise_t = T(data, dev), T(perm, dev), T(noise, dev)
    for per_point in (False, True):
        want = ref.assemble(data, lab_p if per_point else lab_s, samples, N, noise=noise, sort_cloud=sort_cloud)
        for dt in (np.uint8, np.int32, np.int64):
            lab = (lab_p if per_point else lab_s).astype(dt)
            pts, inp, labels, bad, rnd = provider.assemble_batch(d_t, T(lab, dev), B, num_points=N, perm=perm_t, start=start,
                                                                 jitter=True, noise=noise_t, sort_cloud=sort_cloud,
                                                                 return_randoms=True)
            pts, inp = pts.cpu().numpy(), inp.cpu().numpy()
            assert np.array_equal(pts.view(np.uint32), want[0].view(np.uint32)), (per_point, dt)
            assert np.array_equal(inp.view(np.uint32), want[1].view(np.uint32)), (per_point, dt)
            assert np.array_equal(inp[:, :, 0:3], pts)
            assert labels.cpu().numpy().dtype == np.int32 and np.array_equal(labels.cpu().numpy(), want[2])
            order = rnd["order"].cpu().numpy()
            assert np.array_equal(order, want[3]) and int(bad) == 0
            src_rows = data[samples][:, 0:N, 3:]
            assert np.array_equal(inp[:, :, 3:], np.stack([src_rows[b][order[b]] for b in range(B)]))
            assert np.array_equal(rnd["noise"].cpu().numpy(), noise)


# ------------------------------------------------------------------------------- the device's draws
@pytest.mark.gpu
@pytest.mark.parametrize("S,N,B", [(4, 300, 4), (2, 2048, 2)])
def test_device_drawn_randoms(dev, S, N, B):
    import torch
    from pointwise_amd import provider
    seed, step = 0x1234567890ABCDEF, (1 << 33) + 5
    data = dataset(S, N, 3, 800 + N)
    lab = np.arange(S, dtype=np.int64)
    perm = np.arange(S)[::-1].astype(np.int32).copy()
    d_t, l_t, p_t = T(data, dev), T(lab, dev), T(perm, dev)
    kw = dict(perm=p_t, rotate=True, jitter=True, sort_cloud=True, seed=seed, step=step)
    pts, inp, labels, bad, rnd = provider.assemble_batch(d_t, l_t, B, return_randoms=True, **kw)
    keep = [t.clone() for t in (pts, inp, labels)]
    cs, noise = rnd["cos_sin"].cpu().numpy(), rnd["noise"].cpu().numpy()
    samples = perm[:B]
    angles, normals = ref.draw_angles(seed, step, samples), ref.draw_noise(seed, step, samples, N)
    got_angle = np.mod(np.arctan2(cs[:, 1], cs[:, 0]), 2 * np.pi)
    d_angle = np.abs(got_angle - angles)
    d_angle = np.minimum(d_angle, 2 * np.pi - d_angle).max()
    d_noise = np.abs(noise - normals).max()
    print("max |angle - restated| %.3e   max |noise - restated| %.3e" % (d_angle, d_noise))
    assert d_angle <= DRAW_BOUND and d_noise <= DRAW_BOUND
    assert np.abs(np.hypot(cs[:, 0], cs[:, 1]) - 1.0).max() <= 1e-15
    # the outputs against the restatement applied to the restated randoms (sorted rows: compare in source order)
    want = ref.assemble(data, lab, samples, N, angles=angles, noise=normals)
    order = rnd["order"].cpu().numpy().astype(np.int64)
    back = np.empty_like(want[0])
    for b in range(B):
        back[b, order[b]] = pts.cpu().numpy()[b]
        assert sorted(order[b].tolist()) == list(range(N))
    assert ulp_diff(back, want[0]) <= 1
    assert np.array_equal(labels.cpu().numpy(), want[2])
    # given its own randoms back, the call is the same bitwise; and it is reproducible
    again = provider.assemble_batch(d_t, l_t, B, perm=p_t, rotate=True, jitter=True, sort_cloud=True,
                                    cos_sin=rnd["cos_sin"].clone(), noise=rnd["noise"].clone())
    twice = provider.assemble_batch(d_t, l_t, B, **kw)
    for a, b, c in zip(keep, again, twice):
        assert torch.equal(a, b) and torch.equal(a, c)
    for other in (dict(step=step + 1), dict(seed=seed + 1)):
        diff = provider.assemble_batch(d_t, l_t, B, **{**kw, **other})[0]
        assert not torch.equal(diff, keep[0])
    # a sample's rows do not depend on its place in the batch
    if B == 4:
        for s in range(S):
            alone = provider.assemble_batch(d_t, l_t, 1, perm=T(np.array([s], dtype=np.int32), dev), **{k: v for k, v in kw.items() if k != "perm"})
            for pos in range(4):
                pm = np.array([(s + 1) % S] * 4, dtype=np.int32)
                pm[pos] = s
                inb = provider.assemble_batch(d_t, l_t, 4, perm=T(pm, dev), **{k: v for k, v in kw.items() if k != "perm"})
                assert torch.equal(inb[0][pos], alone[0][0]) and torch.equal(inb[1][pos], alone[1][0])
                assert int(inb[2][pos]) == int(alone[2][0])


# ------------------------------------------------------------------------------- limits
@pytest.mark.gpu
def test_limits(dev):
    import torch
    from pointwise_amd import provider
    from pointwise_amd.conv3p_op import Conv3pRuntimeError
    data = dataset(2, 9000, 3, 900)
    lab = np.array([3, 4], dtype=np.uint8)
    d_t, l_t = T(data, dev), T(lab, dev)
    with pytest.raises(Conv3pRuntimeError):
        provider.assemble_batch(d_t, l_t, 2, sort_cloud=True)                         # N > 8192: unsupported, says so
    noise = np.random.default_rng(1).standard_normal((2, 9000, 3))
    pts, inp, labels, bad = provider.assemble_batch(d_t, l_t, 2, jitter=True, noise=T(noise, dev))
    want = ref.assemble(data, lab, [0, 1], 9000, noise=noise)
    assert np.array_equal(pts.cpu().numpy(), want[0]) and np.array_equal(inp.cpu().numpy(), want[1])
    assert np.array_equal(labels.cpu().numpy(), want[2]) and int(bad) == 0
    empty = provider.assemble_batch(d_t, l_t, 0, sort_cloud=True)
    assert tuple(empty[0].shape) == (0, 9000, 3) and tuple(empty[2].shape) == (0,) and int(empty[3]) == 0
    none = provider.assemble_batch(d_t, l_t, 2, num_points=0)
    assert tuple(none[1].shape) == (2, 0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("sort_cloud", [False, True], ids=["flat", "sort"])
def test_sample_indices_outside_the_data_set_are_not_read(dev, sort_cloud):
    from pointwise_amd import provider
    S, N, K = 3, 300, 9
    data, _, lab_p, _ = shared_dataset(4, 257, 9)
    data, lab_p = data[:S], lab_p[:S]
    perm = np.array([1, -1, 2, S, 0], dtype=np.int32)
    for lab in (lab_p.astype(np.uint8), np.arange(S, dtype=np.int64)):
        got = provider.assemble_batch(T(data, dev), T(lab, dev), 5, perm=T(perm, dev), rotate=False, jitter=True,
                                      sort_cloud=sort_cloud, seed=4, step=5)
        clean = provider.assemble_batch(T(data, dev), T(lab, dev), 3, perm=T(perm[[0, 2, 4]].copy(), dev), jitter=True,
                                        sort_cloud=sort_cloud, seed=4, step=5)
        assert int(got[3]) == 2 and int(clean[3]) == 0
        pts, inp, labels = (t.cpu().numpy() for t in got[:3])
        for b in (1, 3):
            assert not pts[b].any() and not inp[b].any() and (labels[b] == -1).all()
        for i, b in enumerate((0, 2, 4)):
            assert np.array_equal(pts[b], clean[0][i].cpu().numpy()) and np.array_equal(inp[b], clean[1][i].cpu().numpy())
            assert np.array_equal(labels[b], clean[2][i].cpu().numpy())


# ------------------------------------------------------------------------------- the provider class
@pytest.mark.gpu
def test_batch_provider_epochs(dev):
    import torch
    from pointwise_amd import provider
    S, B, N = 7, 2, 64
    data = dataset(S, 70, 3, 950)
    lab = np.arange(S, dtype=np.uint8) + 10
    # evaluation: identity order, no augmentation, the reference's loop (train_modelnet40_acsd.py's `while True`)
    ev = provider.BatchProvider(data, lab, B, num_points=N, training=False, device=dev)
    assert (ev.num_batches, ev.num_points, ev.num_channels) == (3, N, 3) and not ev.rotate and not ev.jitter
    seen = []
    while True:
        pts, inp, labels = ev.get_batch_point_cloud()
        k = len(seen)
        assert np.array_equal(pts.cpu().numpy(), data[k * B:(k + 1) * B, 0:N]) and torch.equal(pts, inp)
        assert labels.cpu().tolist() == lab[k * B:(k + 1) * B].tolist()
        seen.append(k)
        if not ev.has_next_batch():
            break
        assert ev.next_batch() is True
    assert seen == [0, 1, 2] and int(ev.bad_index) == 0                  # the seventh cloud is dropped

    tr = provider.BatchProvider(data, lab, B, num_points=N, training=True, seed=5, device=dev)
    assert tr.rotate and tr.jitter
    perms = []
    for epoch in range(2):
        p = tr.permutation.cpu().numpy()
        assert sorted(p.tolist()) == list(range(S))
        assert np.array_equal(p, np.random.default_rng([5, epoch]).permutation(S))
        perms.append(p)
        tr.next_epoch()
    assert not np.array_equal(perms[0], perms[1]) and tr.epoch == 2 and tr.cur_batch == 0
    # labels follow the permutation; a batch stays valid while the next is assembled
    first = tr.get_batch_point_cloud()
    kept = [t.clone() for t in first]
    assert first[2].cpu().tolist() == lab[tr.permutation.cpu().numpy()[0:B]].tolist()
    tr.next_batch()
    state = tr.state_dict()
    assert state == {"seed": 5, "epoch": 2, "cur_batch": 1} and tr.step == 2 * 3 + 1
    second = tr.get_batch_point_cloud()
    for a, b in zip(first, kept):
        assert torch.equal(a, b)
    assert not torch.equal(second[0], first[0]) and second[0].data_ptr() != first[0].data_ptr()
    # resume
    other = provider.BatchProvider(data, lab, B, num_points=N, training=True, seed=99, device=dev)
    other.load_state_dict(state)
    resumed = other.get_batch_point_cloud()
    for a, b in zip(second, resumed):
        assert torch.equal(a, b)
    # scene data: per-point labels, no augmentation by default, sorted
    rooms, _, lab_p, _ = shared_dataset(4, 257, 9)
    sc = provider.BatchProvider(rooms, lab_p.astype(np.uint8), 2, training=True, sort_cloud=True, seed=1, device=dev)
    assert not sc.rotate and not sc.jitter and sc.num_channels == 9 and sc.num_points == 257
    pts, inp, labels = sc.get_batch_point_cloud()
    want = ref.assemble(rooms, lab_p, sc.permutation.cpu().numpy()[0:2], 257, sort_cloud=True)
    assert np.array_equal(inp.cpu().numpy(), want[1]) and np.array_equal(pts.cpu().numpy(), want[0])
    assert np.array_equal(labels.cpu().numpy(), want[2])
