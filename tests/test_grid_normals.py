"""GPU tests (-m gpu) of GridSubsample.normals / with_normals on conv3p_grid_normals_f32: samples, flags, moments and the
counts bit for bit against tests/grid_normals_ref.py, normals and curvature against the float64 eigen-decomposition of the
device's own moments with include/conv3p.h's bounds (grid_normals_ref.compare_r5), in both subsampling modes unless a test
names one -- one row; a full block of cells; voxel counts around the 64 voxels of a wave, the 256 of a workgroup and the
524 288 one pass of the largest grid takes, cut by max_voxels and followed by filler rows, trimmed and untrimmed; a flat
cloud under three orientations; a sphere; a room; a line; a NaN representative; many clouds with a viewpoint per room;
reproducibility; with_normals."""
import numpy as np
import pytest

from tests import grid_normals_ref as gn
from tests import grid_ref as gr

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("mean", "center")


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def subsample(data, **kw):
    import torch
    from pointwise_amd import grid
    d = torch.from_numpy(np.ascontiguousarray(data)).to(_dev())
    return d, grid.grid_subsample(d, None, **kw)


def host(nrm):
    return {k: getattr(nrm, k).cpu().numpy() for k in ("normals", "curvature", "samples", "flags", "moments", "stats")
            if getattr(nrm, k) is not None}


def same(a, b, what):
    for k in a:
        gn_bits(a[k], b[k], "%s: %s" % (what, k))


def gn_bits(got, want, what):
    from tests.grid_interp_ref import assert_same
    assert_same(got, want, what)


def check(g, viewpoint=None, min_neighbors=6, what="", max_left_out=None):
    """normals() with and without the moments against the reference -> (the device's outputs, the reference's, (compared,
    flags-0 voxels, worst angle ratio)).  The neighbour table is the device's own (tests/test_grid_interp.py checks it)."""
    import torch
    kw = {"viewpoint": viewpoint, "min_neighbors": min_neighbors}
    got = host(g.normals(return_moments=True, **kw))
    vd, neigh, nv = g.data.cpu().numpy(), g.neighbors().cpu().numpy(), int(g.stats[0])
    M = vd.shape[0]
    assert got["normals"].shape == (M, 3) and got["moments"].shape == (M, 9) and got["stats"].shape == (4,)
    vp = viewpoint.cpu().numpy() if isinstance(viewpoint, torch.Tensor) else viewpoint
    room = g.voxel_room.cpu().numpy() if getattr(g, "voxel_room", None) is not None else None
    samples, flags, moments, stats = gn.moments_ref(vd, neigh, nv, min_neighbors)
    gn_bits(got["samples"], samples, what + ": samples")
    gn_bits(got["flags"], flags, what + ": flags")
    gn_bits(got["moments"], moments, what + ": moments")
    gn_bits(got["stats"], stats, what + ": stats")
    assert int(stats.sum()) == M and int(stats[3]) == M - min(max(nv, 0), M)
    r5 = gn.compare_r5(got["normals"], got["curvature"], got["flags"], got["moments"], vd, vp, room, max_left_out)
    print("%s: %d voxels, stats %s, compared %d of %d, worst angle ratio %.3f (bound 64)" % ((what, M, stats.tolist()) + r5))
    bare = g.normals(**kw)                               # moments NULL: everything else the same bits
    assert bare.moments is None
    same(host(bare), {k: v for k, v in got.items() if k != "moments"}, what + ", without the moments")
    ref = {"samples": samples, "flags": flags, "moments": moments, "stats": stats}
    return got, ref, r5


def cells_cloud(count, seed, rows_per_cell=2, step=0.1):
    """count occupied cells of a lattice about 1.3 count large, rows_per_cell rows in each -> float32 (rows, 4)."""
    rng = np.random.default_rng(seed)
    n = int(np.ceil((1.3 * count) ** (1.0 / 3.0)))
    cells = np.concatenate([[0], 1 + rng.permutation(n ** 3 - 1)[:count - 1]])
    ijk = np.stack([cells // (n * n), (cells // n) % n, cells % n], axis=1)
    xyz = np.concatenate([(ijk + 0.2 + 0.6 * rng.random((count, 3))) * step for _ in range(rows_per_cell)])
    xyz[0] = 0.0
    return np.concatenate([xyz, rng.random((xyz.shape[0], 1))], axis=1).astype(F)


# ---------------------------------------------------------------------------------------------------- 1: the small ends
@pytest.mark.parametrize("mode", MODES)
def test_one_row_and_a_full_block_of_cells(mode):
    d, g = subsample(np.array([[0.3, -1.0, 2.0, 5.0]], F), voxel=0.1, mode=mode)
    got, ref, _ = check(g, what="one row")
    assert got["samples"].tolist() == [1] and got["flags"].tolist() == [1] and got["stats"].tolist() == [0, 1, 0, 0]
    d, g = subsample(np.array([[0.3, -1.0, 2.0], [5.0, 5.0, 5.0], [np.nan, 0.0, 0.0]], F), voxel=0.1, mode=mode)
    got, ref, _ = check(g, what="two voxels and a filler row", viewpoint=(0.0, 0.0, 0.0), min_neighbors=3)
    assert got["flags"].tolist() == [1, 1, -1] and got["stats"].tolist() == [0, 2, 0, 1] and not got["normals"].any()
    # the 5 x 5 x 5 block of tests/test_grid_interp.py::test_a_full_block_of_cells
    rng = np.random.default_rng(21)
    ijk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = np.concatenate([(ijk + 0.1 + 0.8 * rng.random((125, 3))) * 0.2 for _ in range(3)])
    xyz[0] = 0.0
    d, g = subsample(rng.permutation(xyz).astype(F), voxel=0.2, mode=mode)
    got, ref, _ = check(g, min_neighbors=9, what="full block", viewpoint=(0.5, 0.5, 3.0))
    s = got["samples"]
    assert int(g.stats[0]) == 125 and s[62] == 27 and (s[:125] == 27).sum() == 27 and (s[:125] == 8).sum() == 8
    assert [s[c] for c in (0, 4, 20, 24, 100, 104, 120, 124)] == [8] * 8
    few = np.nonzero(got["flags"] == 1)[0]
    assert few.tolist() == np.nonzero(ref["samples"][:125] < 9)[0].tolist() == [0, 4, 20, 24, 100, 104, 120, 124]
    assert got["stats"].tolist() == [117, 8, 0, xyz.shape[0] - 125] and g.normals(min_neighbors=9).count() == 117


# ------------------------------------------------------------------------------- 2: the edges of the wave and the workgroup
@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 513])
def test_voxel_counts_around_the_wave_and_the_workgroup(count):
    for mode in MODES:
        data = cells_cloud(count, 300 + count)
        d, g = subsample(data, voxel=0.1, mode=mode, max_voxels=count + 37)        # ne = count < M: filler rows follow
        assert int(g.stats[0]) == count and g.data.shape[0] == count + 37
        got, ref, _ = check(g, viewpoint=(0.4, 0.3, 9.0), min_neighbors=4, what="%d voxels and 37 filler rows, %s" % (count, mode))
        assert got["stats"][3] == 37 and (got["flags"][count:] == -1).all() and not got["moments"][count:].any()
        assert got["stats"][0] > count // 4
        t = g.trim()
        trimmed, _, _ = check(t, viewpoint=(0.4, 0.3, 9.0), min_neighbors=4, what="%d voxels, trimmed, %s" % (count, mode))
        assert t.data.shape[0] == count and trimmed["stats"][3] == 0
        same({k: v[:count] for k, v in got.items() if k != "stats"}, {k: v for k, v in trimmed.items() if k != "stats"},
             "trimmed against untrimmed")
        d, cut = subsample(cells_cloud(count + 50, 900 + count), voxel=0.1, mode=mode, max_voxels=count)   # ne = M = count: the cut
        assert int(cut.stats[0]) == count and int(cut.stats[1]) == count + 50
        got, ref, _ = check(cut, min_neighbors=4, what="cut to %d voxels, %s" % (count, mode))
        assert got["stats"][3] == 0 and (cut.neighbors().cpu().numpy() < count).all()


def test_more_voxels_than_one_pass_of_the_grid():
    """2048 workgroups of 256 voxels take 524 288 voxels a pass: the voxel loop's second pass, mode center."""
    count = 2048 * 256 + 257
    d, g = subsample(cells_cloud(count, 77, rows_per_cell=1), voxel=0.1, mode="center", max_voxels=count + 3)
    assert int(g.stats[0]) == count
    got = host(g.normals(viewpoint=(1.0, 2.0, 50.0), return_moments=True))
    fl = got["flags"]
    assert got["stats"].tolist() == [(fl == 0).sum(), (fl == 1).sum(), (fl == 2).sum(), 3] and got["stats"][0] > count // 2
    assert (fl[count:] == -1).all() and not got["moments"][count:].any() and not got["normals"][count:].any()
    # the reference on the voxels at both ends and around the edge of the pass, as a problem of their own: these
    # voxels and their neighbours renumbered (the order of t, which is all the chains depend on, stays)
    rows = np.concatenate([np.arange(3000), np.arange(2048 * 256 - 3000, count)])         # both ends, and across the edge of the pass
    vd, neigh = g.data.cpu().numpy(), g.neighbors().cpu().numpy()
    need = np.unique(np.concatenate([rows, neigh[rows][neigh[rows] >= 0]]))
    remap = np.full(vd.shape[0], -1, np.int32)
    remap[need] = np.arange(need.size, dtype=np.int32)
    sub = np.where(neigh[need] >= 0, remap[np.maximum(neigh[need], 0)], -1).astype(np.int32)
    samples, flags, moments, _ = gn.moments_ref(vd[need], sub, need.size, 6)
    at = remap[rows]
    gn_bits(got["samples"][rows], samples[at], "samples")
    gn_bits(fl[rows], flags[at], "flags")
    gn_bits(got["moments"][rows], moments[at], "moments")
    r5 = gn.compare_r5(got["normals"][rows], got["curvature"][rows], fl[rows], got["moments"][rows], vd[rows], (1.0, 2.0, 50.0))
    print("%d voxels: stats %s, compared %d of %d, worst angle ratio %.3f (bound 64)" % ((count, got["stats"].tolist()) + r5))
    assert r5[1] > 5000


# ------------------------------------------------------------------------------------------------------------ 3: a flat cloud
@pytest.mark.parametrize("mode", MODES)
def test_the_flat_cloud_under_three_orientations(mode):
    data, _ = gr.cloud(3000, 4, 31, extent=(2.0, 1.5, 0.05))
    d, g = subsample(data, voxel=0.1, mode=mode)
    up, _, r5 = check(g, viewpoint=(1.0, 0.75, 10.0), what="flat, from above", max_left_out=0.01)
    ok = up["flags"] == 0
    assert ok.sum() > 250 and (up["normals"][ok, 2] > 0).all() and (np.abs(up["normals"][ok, 2]) > 0.9).all()
    down, _, _ = check(g, viewpoint=(1.0, 0.75, -10.0), what="flat, from below", max_left_out=0.01)
    assert (down["normals"][ok, 2] < 0).all()
    gn_bits(down["normals"][ok], -up["normals"][ok], "from below is the negation")
    free, _, _ = check(g, what="flat, no viewpoint", max_left_out=0.01)
    n = free["normals"][ok]
    top = n[np.arange(n.shape[0]), np.abs(n).argmax(axis=1)]
    assert (top > 0).all() and np.array_equal(np.abs(free["normals"]), np.abs(up["normals"]))
    gn_bits(free["curvature"], up["curvature"], "the curvature does not depend on the orientation")


# --------------------------------------------------------------------------------------------------------------- 4: a sphere
@pytest.mark.parametrize("mode", MODES)
def test_a_unit_sphere_seen_from_its_centre(mode):
    import torch
    d, g = subsample(gn.sphere(), voxel=0.1, mode=mode)
    got, _, r5 = check(g, viewpoint=torch.zeros((1, 3), device=d.device), what="sphere", max_left_out=0.01)
    ok = got["flags"] == 0
    p = g.data.cpu().numpy()[ok, :3].astype(np.float64)
    dot = (got["normals"][ok] * p).sum(axis=1)
    assert ok.sum() > 1000 and (dot < 0).all()
    radial = np.arccos(np.minimum(-dot / np.sqrt((p * p).sum(axis=1)), 1.0))
    assert radial.max() <= 0.35                          # tests/test_grid_normals_host.py measures 0.083 on the reference


# ----------------------------------------------------------------------------------------------------------------- 5: a room
@pytest.mark.parametrize("mode", MODES)
def test_a_room(mode):
    from pointwise_amd import synth
    xyz = synth.room_like(1, 20000, 7, extent=(2.0, 2.0, 2.0))[0].astype(F)
    d, g = subsample(xyz, voxel=0.1, mode=mode)
    got, _, r5 = check(g, viewpoint=(1.0, 1.0, 1.0), what="room", max_left_out=0.01)
    nv = int(g.stats[0])
    assert 2000 < nv < 2600 and 0 < got["stats"][1] < 60 and got["stats"][2] == 0 and got["stats"][0] + got["stats"][1] == nv
    assert r5[0] > 0.99 * r5[1]
    check(g.trim(), what="room, trimmed, no viewpoint, every voxel with three samples", min_neighbors=3, max_left_out=0.01)


# ----------------------------------------------------------------------------------------------------------------- 6: a line
@pytest.mark.parametrize("mode", MODES)
def test_a_line_has_a_unit_normal_of_some_direction(mode):
    x = (np.arange(400) + 0.5) * (5.0 / 400)
    data = np.stack([x, np.full(400, 0.31), np.full(400, -0.77)], axis=1).astype(F)
    data[::3, 1] += F(1e-3)                              # not exactly collinear: the trace stays positive either way
    d, g = subsample(data, voxel=0.1, mode=mode)
    got, _, r5 = check(g, viewpoint=(2.5, 4.0, 1.0), min_neighbors=3, what="line")
    nv = int(g.stats[0])
    ok = got["flags"] == 0
    assert nv >= 50 and ok.sum() == nv - 2 and (got["samples"][:nv] <= 3).all()     # the two ends have two samples
    lam = np.linalg.eigvalsh(gn.covariance(got["moments"][ok]))
    assert (lam[:, 1] < 1e-3 * lam[:, 2]).all()          # l0 ~ l1: the direction is not defined, and nothing is asked of it
    n = got["normals"][ok].astype(np.float64)
    assert np.isfinite(n).all() and np.abs(np.sqrt((n * n).sum(axis=1)) - 1).max() <= 1e-6      # (compare_r5 checked R6)


# ------------------------------------------------------------------------------------------------ 7: a NaN representative
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_representative_is_nobodys_sample(mode):
    data, _ = gr.cloud(6000, 4, 71, extent=(0.8, 0.8, 0.8))
    d, g = subsample(data, voxel=0.1, mode=mode)
    g = g.trim()
    before, _, _ = check(g, what="before the NaN")
    v = int(np.argmax(before["samples"] == 27))
    assert before["samples"][v] == 27
    neigh = g.neighbors().cpu().numpy()
    g.data[v, 0] = float("nan")
    after, _, _ = check(g, what="after the NaN")
    assert after["samples"][v] == 0 and after["flags"][v] == 1 and not after["moments"][v].any() and not after["normals"][v].any()
    around = np.setdiff1d(neigh[v], [v])
    assert around.size == 26 and np.array_equal(after["samples"][around], before["samples"][around] - 1)
    rest = np.setdiff1d(np.arange(g.data.shape[0]), neigh[v])
    same({k: x[rest] for k, x in after.items() if k != "stats"}, {k: x[rest] for k, x in before.items() if k != "stats"},
         "the voxels out of reach")


# ----------------------------------------------------------------------------------------------------------- 8: many clouds
SIZES = (5000, 4000, 60, 4500)


def raw_rooms():
    from pointwise_amd import synth
    rng = np.random.default_rng(5200)
    parts = []
    for k, n in enumerate(SIZES):                        # the rooms overlap in space: each starts at its own origin
        xyz = synth.room_like(1, n, 5201 + k, (2.2 - 0.3 * k, 1.6 + 0.2 * k, 2.0))[0]
        parts.append(np.concatenate([xyz, rng.random((n, 3))], axis=1).astype(F))
    parts[2][:, 0] = np.nan                              # a room of non-finite rows only: it has no voxels
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)


@pytest.mark.parametrize("mode", MODES)
def test_many_clouds_with_a_viewpoint_each_equal_their_single_calls(mode):
    import torch
    from pointwise_amd import grid
    dev = _dev()
    data, start = raw_rooms()
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample_rooms(d, torch.from_numpy(start).to(dev), None, voxel=0.1, mode=mode)
    vps = np.array([[1.0, 1.0, 5.0], [-3.0, 0.5, 1.0], [0.0, 0.0, 0.0], [1.0, 9.0, -2.0]], F)
    vp = torch.from_numpy(vps).to(dev)
    got, _, _ = check(g, viewpoint=vp, what="rooms, untrimmed")
    vstart = g.voxel_start.cpu().numpy()
    nv = int(g.stats[0])
    assert vstart[2] == vstart[3] and nv == vstart[4] > 1500 and g.data.shape[0] == data.shape[0]
    pieces = []
    for r in range(len(SIZES)):
        one = grid.grid_subsample(d[int(start[r]):int(start[r + 1])].contiguous(), None, voxel=0.1, mode=mode).trim()
        assert one.data.shape[0] == vstart[r + 1] - vstart[r]
        pieces.append(host(one.normals(viewpoint=vp[r:r + 1].contiguous(), return_moments=True)))
    whole = {k: np.concatenate([p[k] for p in pieces]) for k in pieces[0] if k != "stats"}
    same({k: v[:nv] for k, v in got.items() if k != "stats"}, whole, "rooms against their single calls")
    assert got["stats"][:3].tolist() == sum(p["stats"][:3] for p in pieces).tolist()
    t, _, _ = check(g.trim(), viewpoint=vp, what="rooms, trimmed")
    same({k: v[:nv] for k, v in got.items() if k != "stats"}, {k: v for k, v in t.items() if k != "stats"}, "rooms, trimmed")
    one_vp, _, _ = check(g, viewpoint=(1.0, 1.0, 5.0), what="rooms, one viewpoint")          # V = 1 with voxel_room
    a, b = int(vstart[0]), int(vstart[1])
    gn_bits(one_vp["normals"][a:b], got["normals"][a:b], "room 0 has that viewpoint in both calls")
    view, _, _ = check(g.room(3), viewpoint=vp[3:4].contiguous(), what="the view of room 3")
    gn_bits(view["normals"], got["normals"][vstart[3]:vstart[4]], "the view of room 3 against the whole")


# ------------------------------------------------------------------------------------- 9, 10: reproducibility; with_normals
def test_two_calls_give_identical_bits():
    import torch
    data, _ = gr.cloud(20000, 6, 121, extent=(1.5, 1.2, 0.9))
    data[11, 1] = np.nan
    d, g = subsample(data, voxel=0.1, mode="mean")
    vp = torch.tensor([[0.7, 0.6, 0.4]], device=d.device)
    a = g.normals(viewpoint=vp, return_moments=True)
    first = host(a)
    from pointwise_amd import grid
    out = grid.GridNormals(g.data.shape[0], True, d.device)
    for t in (out.normals, out.curvature, out.moments):
        t.fill_(7.0)
    b = g.normals(viewpoint=vp, return_moments=True, out=out)
    assert b is out
    same(host(b), first, "the second call")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _, g2 = subsample(data, voxel=0.1, mode="mean")
        c = g2.normals(viewpoint=vp, return_moments=True)                 # the table too is built on the side stream
    side.synchronize()
    same(host(c), first, "a side stream")
    assert first["stats"][0] > 1000 and a.count() == first["stats"][0]


@pytest.mark.parametrize("mode", MODES)
def test_with_normals_puts_the_columns_side_by_side(mode):
    import torch
    data, _ = gr.cloud(5000, 6, 131, extent=(1.0, 0.8, 0.5))
    d, g = subsample(data, voxel=0.1, mode=mode)
    for obj in (g, g.trim()):
        nrm = obj.normals(viewpoint=(0.5, 0.4, 3.0))
        M = obj.data.shape[0]
        a, b = obj.with_normals(nrm), obj.with_normals(nrm, curvature=True)
        assert tuple(a.shape) == (M, 9) and tuple(b.shape) == (M, 10) and a.is_contiguous() and b.is_contiguous()
        assert a.dtype == torch.float32 and a.device == obj.data.device
        assert torch.equal(a[:, :6], obj.data) and torch.equal(a[:, 6:9], nrm.normals) and torch.equal(b[:, :9], a)
        assert torch.equal(b[:, 9], nrm.curvature) and nrm.count() > 200
