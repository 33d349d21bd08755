"""The wide sort on the device (-m gpu): prestep.sort_order / sort_point_cloud(2) and the provider with wide_sort=True,
for clouds of up to 65536 points (include/conv3p.h: conv3p_sort_order_f32, conv3p_provider_batch_wide_f32).

Bounds: none.  Both orders are strict total orders -- the row index breaks every tie -- so the result is unique:
every comparison of orders is np.array_equal / torch.equal on int32 and every comparison of rows is bit for bit.
References: tests/morton_ref.batch_order for "morton"; np.lexsort((arange, z, y, x)) on the float32 values for "xyz"
(util.py:66-68: three stable argsorts; lexsort compares values, so -0.0 == +0.0, and puts NaN last).  A reference is
computed once per batch and method and shared by the tests that need it."""
import functools

import numpy as np
import pytest

from pointwise_amd import synth
from tests import morton_ref

METHODS = ("xyz", "morton")


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


def xyz_order(batch):
    batch = np.asarray(batch)
    idx = np.arange(batch.shape[1])
    return np.stack([np.lexsort((idx, c[:, 2], c[:, 1], c[:, 0])) for c in batch]).astype(np.int32)


def ref_order(batch, method):
    return xyz_order(batch) if method == "xyz" else morton_ref.batch_order(batch)


def _special(N):
    """Three clouds of N rows: (0) NaN / +-Inf rows, the last row among them, -0.0 beside +0.0 and repeated rows; (1) all
    rows identical; (2) no finite row."""
    rng = np.random.default_rng(N)
    a = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    a[N - 1] = (np.nan, 0.25, -0.5)                                      # N = 65536: the Morton key is all ones
    a[N - 2, 2] = np.inf
    a[7, 0] = -np.inf
    a[N // 2] = (np.inf, np.nan, -np.inf)
    a[100:104, 0] = (0.0, -0.0, 0.0, -0.0)                               # equal values: y, z and the index decide
    a[100:104, 1:] = a[100, 1:]
    a[9000:9010] = a[5]                                                  # ties with a row of another chunk
    a[N - 20:N - 10] = a[5]
    a[200, 0], a[201, 0] = -0.0, 0.0
    b = np.full((N, 3), -0.3, dtype=np.float32)
    c = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    c[np.arange(N), rng.integers(0, 3, size=N)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=N)
    return np.stack([a, b, c])


BATCHES = {
    "modelnet_like_2x8193": lambda: synth.modelnet_like(2, 8193, seed=3),       # one full chunk and a row, whatever the chunk
    "lattice_2x20000": lambda: synth.lattice(2, 20000, seed=4),                 # ties across chunk borders; odd run counts
    "uniform_cube_3x24577": lambda: synth.uniform_cube(3, 24577, seed=5),
    "room_like_2x65536": lambda: synth.room_like(2, 65536, seed=7),             # the limit: no padding
    "1x1": lambda: synth.uniform_cube(1, 1, seed=11),
    "1x64": lambda: synth.uniform_cube(1, 64, seed=12),
    "2x300": lambda: synth.uniform_cube(2, 300, seed=13),
    "2x8192": lambda: synth.uniform_cube(2, 8192, seed=14),
    "special_3x65536": lambda: _special(65536),
    "special_3x20000": lambda: _special(20000),
}


@functools.lru_cache(maxsize=None)
def batch(name):
    b = np.ascontiguousarray(BATCHES[name](), dtype=np.float32)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def reference(name, method):
    r = ref_order(batch(name), method)
    r.setflags(write=False)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", [n for n in BATCHES if not n.startswith("special")])
def test_orders_equal_the_references(dev, name, method):
    from pointwise_amd import prestep
    x = batch(name)
    want = reference(name, method)
    got = prestep.sort_order(T(x, dev), method).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == x.shape[:2] and np.array_equal(got, want)
    rows9 = np.concatenate([x, synth.features(x.shape[0], x.shape[1], 6, 9, points=x)], axis=2)   # the row stride
    assert rows9.shape[2] == 9 and np.array_equal(prestep.sort_order(T(rows9, dev), method).cpu().numpy(), want)


def test_the_lattice_ties_cross_chunk_borders():
    """Not a GPU test: the figures the shapes were chosen by."""
    lat = batch("lattice_2x20000")
    for c in lat:
        assert 8000 < c.shape[0] - np.unique(morton_ref.codes(c)).size < 9500
        assert 8000 < c.shape[0] - np.unique(c, axis=0).shape[0] < 9500
    for chunk in (256, 512, 1024, 2048, 4096, 8192):
        runs, odd = -(-20000 // chunk), False
        while runs > 1:
            odd |= runs % 2 == 1
            runs = -(-runs // 2)
        assert odd, chunk


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [65536, 20000])
def test_special_rows(dev, N, method):
    from pointwise_amd import prestep
    name = "special_3x%d" % N
    x, want = batch(name), reference(name, method)
    got = prestep.sort_order(T(x, dev), method).cpu().numpy()
    assert np.array_equal(got, want)
    assert got[1].tolist() == list(range(N))                              # all rows identical: the identity (Morton: e = 0)
    nonfinite = np.flatnonzero(~np.isfinite(x[0]).all(axis=1))
    assert nonfinite.tolist() == [7, N // 2, N - 2, N - 1]
    if method == "morton":
        assert got[0, -4:].tolist() == nonfinite.tolist()                 # the far code, by index; row N - 1 really last
        assert (morton_ref.codes(x[0])[nonfinite] == morton_ref.FAR).all()
        assert got[2].tolist() == list(range(N))                          # no finite row: every code is the far one
    else:
        assert got[0, 0] == 7 and got[0, -2:].tolist() == [N // 2, N - 1]   # -Inf first; +Inf, then NaN, last
        i100 = got[0].tolist().index(100)
        assert got[0, i100:i100 + 4].tolist() == [100, 101, 102, 103]     # -0.0 == +0.0: the index decides
        five = got[0].tolist().index(5)
        assert got[0, five:five + 21].tolist() == [5] + list(range(9000, 9010)) + list(range(N - 20, N - 10))
    rows = prestep.sort_point_cloud(T(x, dev), method).cpu().numpy()
    assert np.array_equal(bits(rows), bits(morton_ref.gather(x, want)))   # -0.0's sign and the NaNs' payloads survive


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_agreement_with_the_one_workgroup_kernels(dev, method):
    import torch
    from pointwise_amd import prestep
    old = {"xyz": prestep.sort_order_xyz, "morton": prestep.sort_order_morton}[method]
    for N in (300, 2048, 8192):
        x = T(synth.room_like(2, N, seed=N), dev)
        assert torch.equal(prestep.sort_order(x, method), old(x))
    lab = T(np.random.default_rng(1).integers(0, 13, size=(2, 8192)).astype(np.uint8), dev)
    old2 = {"xyz": prestep.sort_point_cloud_xyz2, "morton": prestep.sort_point_cloud_morton2}[method]
    for a, b in zip(prestep.sort_point_cloud2(x, lab, method), old2(x, lab)):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_reproducible_and_independent_of_the_batch_and_the_workspace(dev, method):
    import torch
    from pointwise_amd import _lib, prestep
    name = "uniform_cube_3x24577"
    x = T(batch(name), dev)
    first = prestep.sort_order(x, method)
    assert np.array_equal(first.cpu().numpy(), reference(name, method))
    assert torch.equal(prestep.sort_order(x, method), first)
    for b in range(3):                                                    # a cloud alone, and in another place and batch size
        assert torch.equal(prestep.sort_order(x[b:b + 1].contiguous(), method)[0], first[b])
    assert torch.equal(prestep.sort_order(x[[2, 0]].contiguous(), method), first[[2, 0]])
    need = _lib.load().conv3p_sort_order_workspace_bytes(3, 24577, prestep.SORT_METHODS[method])
    for fill in (0x00, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        assert torch.equal(prestep.sort_order(x, method, workspace=ws), first)


def dataset(S, Nsrc, K, seed):
    rng = np.random.default_rng(seed)
    xyz = synth.room_like(S, Nsrc, seed)
    d = np.concatenate([xyz, rng.standard_normal((S, Nsrc, K - 3)).astype(np.float32)], axis=2)
    d[0, 5, 0:3] = d[0, 9, 0:3]                                            # a tie in sample 0
    return np.ascontiguousarray(d)


def _outputs(res):
    return list(res[:4]) + [res[4][k] for k in ("cos_sin", "noise", "order")]


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("S,N,B", [(4, 300, 4), (2, 2048, 2)])
def test_provider_equals_the_one_launch_call(dev, S, N, B, method):
    """Wherever conv3p_provider_batch_f32 accepts the call, every output of the wide entry is bit-equal to it."""
    import torch
    from pointwise_amd import provider
    rng = np.random.default_rng(S * N)
    perm = T(rng.permutation(S).astype(np.int32)[:B], dev)
    bad_perm = perm.clone()
    bad_perm[1] = S                                                       # one sample outside the data set
    cs = rng.uniform(0, 2 * np.pi, size=B)
    cs = T(np.stack([np.cos(cs), np.sin(cs)], axis=1), dev)
    noise = T(rng.standard_normal((B, N, 3)), dev)
    cases = 0
    for K, per_point, ldtype in ((3, False, np.uint8), (3, False, np.int64), (9, True, np.uint8), (9, True, np.int32),
                                 (9, True, np.int64), (3, False, np.int32)):
        data = T(dataset(S, N + 7, K, 80 + K), dev)
        lab = T(rng.integers(0, 200, size=(S, N + 7) if per_point else (S,)).astype(ldtype), dev)
        for kw in (dict(), dict(rotate=True, jitter=True, seed=5, step=(1 << 33) + 3), dict(rotate=True, cos_sin=cs),
                   dict(jitter=True, noise=noise), dict(rotate=True, jitter=True, cos_sin=cs, noise=noise),
                   dict(rotate=True, jitter=True, seed=6, step=1, perm=bad_perm)):
            kw = dict(dict(perm=perm, num_points=N, sort_cloud=True, sort_method=method, return_randoms=True), **kw)
            want = [t.clone() for t in _outputs(provider.assemble_batch(data, lab, B, **kw))]
            got = _outputs(provider.assemble_batch(data, lab, B, wide_sort=True, **kw))
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and torch.equal(a, b)
            assert int(got[3]) == (1 if kw["perm"] is bad_perm else 0)
            cases += 1
    assert cases == 36


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [9000, 20000])
@pytest.mark.parametrize("K", [3, 9])
def test_provider_beyond_the_one_launch_limit(dev, K, N, method):
    """No yardstick in the project above 8192: the wide call against the unsorted call with the same randoms, ordered by
    the numpy reference and gathered in numpy."""
    import torch
    from pointwise_amd import provider
    S, B = 3, 2
    rng = np.random.default_rng(N + K)
    data = dataset(S, N + 5, K, N + K)
    per_point = K == 9
    lab = rng.integers(0, 250, size=(S, N + 5)).astype(np.uint8) if per_point else rng.integers(0, 40, size=S).astype(np.int64)
    d_t, l_t, perm = T(data, dev), T(lab, dev), T(np.array([2, 0, 1], dtype=np.int32), dev)
    kw = dict(num_points=N, perm=perm, start=1, rotate=not per_point, jitter=True, seed=21, step=(1 << 32) + 4)
    wide = provider.assemble_batch(d_t, l_t, B, sort_cloud=True, sort_method=method, wide_sort=True, return_randoms=True, **kw)
    keep = [t.clone() for t in _outputs(wide)]
    rnd = dict(noise=keep[5], **({"cos_sin": keep[4]} if kw["rotate"] else {}))
    flat = provider.assemble_batch(d_t, l_t, B, **dict(kw, **rnd))         # the unsorted batch
    f_pts, f_inp, f_lab = (t.cpu().numpy() for t in flat[:3])
    assert np.abs(f_pts - data[[0, 1], :N, 0:3]).max() > 0.005           # it was augmented
    order = keep[6].cpu().numpy()
    assert order.dtype == np.int32 and np.array_equal(order, ref_order(f_pts, method))
    assert np.array_equal(bits(keep[0].cpu().numpy()), bits(morton_ref.gather(f_pts, order)))
    assert np.array_equal(bits(keep[1].cpu().numpy()), bits(morton_ref.gather(f_inp, order)))
    want_lab = morton_ref.gather(f_lab, order) if per_point else f_lab
    assert np.array_equal(keep[2].cpu().numpy(), want_lab) and int(keep[3]) == 0
    again = provider.assemble_batch(d_t, l_t, B, sort_cloud=True, sort_method=method, wide_sort=True, return_randoms=True, **kw)
    for a, b in zip(_outputs(again), keep):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_batch_provider_with_wide_sort(dev):
    import torch
    from pointwise_amd import provider
    S, B, N = 4, 2, 9000
    data = dataset(S, N, 3, 90)
    lab = (np.arange(S) + 10).astype(np.uint8)
    bp = provider.BatchProvider(data, lab, B, training=True, sort_cloud=True, seed=9, device=dev, wide_sort=True)
    assert bp.wide_sort and bp.rotate and bp.jitter and bp.num_batches == 2
    assert bp.state_dict() == {"seed": 9, "epoch": 0, "cur_batch": 0}
    seen, state, after = [], None, None
    for epoch in range(2):
        assert bp.epoch == epoch
        while True:
            pts, inp, labels = bp.get_batch_point_cloud()
            assert int(bp.bad_index) == 0 and torch.equal(pts, inp) and pts.shape == (B, N, 3)
            x = pts.cpu().numpy()
            assert np.array_equal(xyz_order(x), np.tile(np.arange(N, dtype=np.int32), (B, 1)))   # the batch is sorted
            if after is None and state is not None:
                after = [t.clone() for t in (pts, inp, labels)]
            seen.append(labels.cpu().tolist())
            if not bp.has_next_batch():
                break
            bp.next_batch()
            if state is None:
                state = bp.state_dict()                                    # before the second batch of the first epoch
        bp.next_epoch()
    assert len(seen) == 4 and sorted(seen[0] + seen[1]) == sorted(seen[2] + seen[3]) == [10, 11, 12, 13]
    other = provider.BatchProvider(data, lab, B, training=True, sort_cloud=True, seed=1, device=dev, wide_sort=True)
    other.load_state_dict(state)
    for a, b in zip(other.get_batch_point_cloud(), after):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_limits(dev):
    import torch
    from pointwise_amd import prestep, provider
    from pointwise_amd.conv3p_op import Conv3pRuntimeError
    for method in METHODS:
        with pytest.raises(Conv3pRuntimeError):
            prestep.sort_order(torch.zeros((1, 65537, 3), device=dev), method)
        assert prestep.sort_point_cloud(torch.zeros((0, 5, 3), device=dev), method).shape == (0, 5, 3)
    data, lab = torch.zeros((1, 65537, 3), device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(Conv3pRuntimeError):
        provider.assemble_batch(data, lab, 1, sort_cloud=True, wide_sort=True)
    with pytest.raises(Conv3pRuntimeError):
        provider.BatchProvider(data, lab, 1, training=False, sort_cloud=True, device=dev, wide_sort=True).get_batch_point_cloud()
    # inert without sort_cloud
    d = T(dataset(3, 9000, 9, 95), dev)
    l = T(np.random.default_rng(96).integers(0, 13, size=(3, 9000)).astype(np.uint8), dev)
    kw = dict(rotate=True, jitter=True, seed=2, step=3, return_randoms=True)
    plain = [t.clone() for t in _outputs(provider.assemble_batch(d, l, 3, **kw))]
    for a, b in zip(_outputs(provider.assemble_batch(d, l, 3, wide_sort=True, **kw)), plain):
        assert torch.equal(a, b)
