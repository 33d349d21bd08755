"""GPU tests (-m gpu) of GridSegments.geometry on conv3p_grid_segment_geometry, against tests/grid_geometry_ref.py on the
device's own segmentation (tests/test_grid_segments.py checks that).  Bit for bit: cell_box, box, moments, centroid, the
sign rule on the stored axes, extent recomputed from the device's own centroid and axes by G8, and the stats.  Within G6's
tolerance, which asks for no gap between eigenvalues: eigenvalues and axes.  The cases are the smallest at which the
kernels can go wrong: runs of equal segment that end at, before and behind a wave's 64 voxels and a wave's chunk of 64 *
steps, no run at all, two interleaved segments whose every atomic is contended, one run through every step.

Every check prints its worst figures of G6's bounds (i), (ii), (iv) in units of u = 2^-53 before it asserts them."""
import numpy as np
import pytest

from tests import grid_geometry_ref as gg

pytestmark = pytest.mark.gpu
F = np.float32
EXACT = ("cell_box", "box", "moments", "centroid", "extent", "stats")
# G6's t in units of u = 2^-53.  The worst measured over all the cases of this file on an MI355X: (i) 4.7, (ii) 6.1,
# (iv) 8.9; t is the next power of two at least ten times above the worst.
T_U = 128.0


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def lattice(occ, rows_per_cell=1, trim=True, **kw):
    """An occupancy (nx, ny, nz) -> the GridSubsample of a cloud with rows_per_cell rows in every occupied cell (voxel 1/4,
    dyadic coordinates: the cell of a row is exact), and the cells of its voxels.  Cell (0, 0, 0) is always occupied."""
    import torch
    from pointwise_amd import grid
    occ = np.asarray(occ, dtype=bool)
    assert occ[0, 0, 0]
    cells = np.argwhere(occ)
    xyz = np.concatenate([(cells + 0.25 + 0.5 * k / max(rows_per_cell, 1)) * 0.25 for k in range(rows_per_cell)]).astype(F)
    d = torch.from_numpy(np.random.default_rng(3).permutation(xyz)).to(_dev())
    g = grid.grid_subsample(d, None, voxel=0.25, **kw)
    g = g.trim() if trim else g
    got = g.voxel_cell.cpu().numpy()
    if "max_voxels" not in kw:
        assert np.array_equal(got[:cells.shape[0]], cells)
    return g, got


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def host(geo):
    return {k: getattr(geo, k).cpu().numpy() for k in EXACT + ("eigenvalues", "axes")}


def same(got, want, what, keys=EXACT):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s: %s" % (what, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s" % (what, k)


def check_geometry(g, seg, weight="voxels", what="", geo=None):
    """seg.geometry(weight) against the reference on the device's own inputs -> (device outputs, reference)."""
    geo = seg.geometry(weight) if geo is None else geo
    got = host(geo)
    S, ne = int(seg.stats[0]), int(g.stats[0])
    want = gg.geometry_ref(g.data.cpu().numpy(), g.voxel_cell.cpu().numpy(), g.voxel_count.cpu().numpy(),
                           seg.segment.cpu().numpy(), S, ne, {"voxels": 0, "rows": 1}[weight], got["eigenvalues"], got["axes"])
    same(got, want, what)
    M = got["moments"].shape[0]
    live = gg.live_rows(got["moments"], S)
    assert live.size == S == geo.num_segments() and geo.trim().axes.shape == (S, 3, 3), what
    dead = np.setdiff1d(np.arange(M), live)
    assert not got["eigenvalues"][dead].any() and not got["axes"][dead].any(), what + ": filler"
    assert np.array_equal(got["moments"][:, 0], (seg.size if weight == "voxels" else seg.rows).cpu().numpy()), what + ": W"
    for s in live:                                       # G7 on the stored vectors
        for k in range(3):
            assert np.array_equal(bits(gg.sign_rule(got["axes"][s, k])), bits(got["axes"][s, k])), (what, s, k)
    fig = gg.figures(got["moments"], S, got["eigenvalues"], got["axes"])     # asserts (iii)
    print("G6 figures in u [%s, %s]: (i) %.3f (ii) %.3f (iv) %.3f" % (what, weight, *fig))
    assert max(fig) <= T_U, (what, fig)
    return got, want


def check(g, labels=None, num_class=None, connectivity=26, what="", weights=("voxels", "rows")):
    import torch
    lab_t = torch.from_numpy(labels).to(g.voxel_count.device) if labels is not None else None
    seg = g.segments(lab_t, num_class, connectivity)
    return seg, [check_geometry(g, seg, w, what)[0] for w in weights]


# ------------------------------------------------------------------------------------------------ 1: cases known by hand
def test_the_hand_l_at_both_weights():
    occ = np.zeros((2, 2, 1), bool)
    occ[0, 0, 0] = occ[1, 0, 0] = occ[1, 1, 0] = True
    g, _ = lattice(occ, rows_per_cell=3)
    _, (v, r) = check(g, what="the L")
    assert v["moments"][0].tolist() == [3, 2, 1, 0, 2, 1, 0, 1, 0, 0] and r["moments"][0].tolist() == [9, 6, 3, 0, 6, 3, 0, 3, 0, 0]
    r2 = 1 / np.sqrt(2)
    for got in (v, r):
        assert got["cell_box"][0].tolist() == [0, 0, 0, 1, 1, 0] and got["centroid"][0].tolist() == [2 / 3, 1 / 3, 0.0]
        assert np.allclose(got["eigenvalues"][0], [1 / 3, 1 / 9, 0.0], rtol=0, atol=T_U * gg.U) and got["eigenvalues"][0, 2] == 0.0
        assert np.allclose(got["axes"][0, 0], [r2, r2, 0], rtol=0, atol=T_U * gg.U) and got["axes"][0, 2].tolist() == [0, 0, 1]
        assert np.allclose(np.abs(got["axes"][0, 1]), [r2, r2, 0], rtol=0, atol=T_U * gg.U)
        assert got["stats"].tolist() == [1, 0, 1, 0]
        assert got["cell_box"][1:].tolist() == [[0, 0, 0, -1, -1, -1]] * 2 and not got["box"][1:].any() and not got["extent"][1:].any()
    assert v["box"][0, :3].tolist() == g.data[:, :3].min(dim=0).values.tolist()


def test_one_voxel_and_no_voxel():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    g = grid.grid_subsample(torch.tensor([[0.3, -1.0, 2.0, 5.0], [0.31, -1.0, 2.0, 1.0]], device=dev), None, voxel=0.1)
    seg, (v, r) = check(g, what="one voxel")
    assert v["moments"][0].tolist() == [1] + [0] * 9 and r["moments"][0].tolist() == [2] + [0] * 9
    for got in (v, r):
        assert got["stats"].tolist() == [1, 1, 1, 0] and got["cell_box"][0].tolist() == [0] * 6 and not got["extent"].any()
        assert not got["eigenvalues"].any() and got["axes"][0].tolist() == np.eye(3).tolist() and not got["axes"][1].any()
        assert np.array_equal(got["box"][0, :3], got["box"][0, 3:]) and got["box"][0].tolist() == g.data[0, :3].tolist() * 2
    check(g, np.array([5], np.int32), 5, 6, "one voxel out of range")        # in no segment: S = 0
    g = grid.grid_subsample(torch.full((3, 3), float("nan"), device=dev), None, voxel=0.1)     # nothing emitted
    _, (v, _) = check(g, what="nothing emitted")
    assert v["stats"].tolist() == [0, 0, 0, 0] and v["cell_box"].tolist() == [[0, 0, 0, -1, -1, -1]] * 3
    geo = g.trim().segments().geometry()                  # M == 0: nothing is launched
    assert geo.cell_box.shape == (0, 6) and geo.axes.shape == (0, 3, 3) and geo.stats.tolist() == [0, 0, 0, 0]
    assert geo.num_segments() == 0 and geo.trim().moments.shape == (0, 10)


# ---------------------------------------------------------------------------- 2: runs, none, contended, through every step
def test_the_checkerboards():
    g, cells = lattice(np.ones((17, 16, 8), bool), rows_per_cell=2)          # 2176 voxels: 34 waves' steps, the last ragged
    lab = (cells.sum(axis=1) % 2).astype(np.int32)
    seg, (v, _) = check(g, lab, 2, 6, "checkerboard at 6: no run")
    assert v["stats"].tolist() == [2176, 2176, 2176, 0] and np.array_equal(v["cell_box"][:, :3], cells)
    seg, (v, _) = check(g, lab, 2, 26, "checkerboard at 26: runs of one, two segments")
    assert v["stats"][0] == 2 and v["moments"][:2, 0].tolist() == [1088, 1088]
    seg, (v, _) = check(g, np.zeros(2176, np.int32), 1, 6, "one label: one run")
    assert v["stats"].tolist() == [1, 0, 0, 0] and v["cell_box"][0].tolist() == [0, 0, 0, 16, 15, 7]
    assert v["centroid"][0].tolist() == [8.0, 7.5, 3.5]


def pieces(M, lengths):
    """Labels 0, 1, 2 in turn over pieces of consecutive voxels of the given lengths; the rest is one more piece."""
    lab = np.zeros(M, np.int32)
    at = 0
    for k, n in enumerate(lengths):
        lab[at:at + n] = k % 3
        at += n
    lab[at:] = len(lengths) % 3
    assert at < M
    return lab


def test_slabs_that_end_around_a_waves_64_voxels():
    # M < 2^16: a wave takes one step of 64 voxels.  Boundaries at 63 | 127 (= 2 * 64 - 1) | 192 (= 3 * 64) | 257, then 64-voxel
    # pieces that start one behind a step, and single voxels at a step's first and last lane.
    g, cells = lattice(np.ones((17, 16, 8), bool))
    lab = pieces(2176, [63, 64, 65, 65, 64, 64, 63, 1, 63, 1, 127, 129])
    seg, (v,) = check(g, lab, 3, 6, "pieces around 64", weights=("voxels",))
    assert v["stats"][0] >= 13


def test_one_segment_of_65536_voxels_and_slabs_around_a_chunk():
    # M = 2^16: a wave takes 4 steps, a chunk of 256 voxels, and carries the open run from step to step
    g, cells = lattice(np.ones((128, 128, 4), bool))
    seg, (v,) = check(g, np.zeros(65536, np.int32), 1, 6, "one segment of 65536", weights=("voxels",))
    assert v["stats"].tolist() == [1, 0, 0, 0] and v["moments"][0, 0] == 65536 and v["cell_box"][0].tolist() == [0, 0, 0, 127, 127, 3]
    assert v["centroid"][0].tolist() == [63.5, 63.5, 1.5]
    assert v["moments"][0, 4] == 4 * 128 * sum(i * i for i in range(128))
    lab = pieces(65536, [63, 64, 65, 63, 1, 255, 256, 257, 255, 1, 256, 1, 1023, 1025, 192, 64, 64, 128, 1])
    check(g, lab, 3, 6, "pieces around 64 and 256", weights=("rows",))


# ----------------------------------------------------------------------------------------- 3: ranks and a tilted plate
def test_a_line_a_plane_and_a_cube():
    for shape, rank in (((40, 1, 1), 1), ((1, 9, 11), 2), ((8, 8, 8), 3)):
        g, cells = lattice(np.ones(shape, bool))
        seg, (v,) = check(g, what="rank %d" % rank, weights=("voxels",))
        lam = v["eigenvalues"][0]
        want = sorted(((n * n - 1) / 12 for n in shape), reverse=True)
        assert np.allclose(lam, want, rtol=0, atol=T_U * gg.U * max(sum(want), 1))
        assert (lam[rank:] == 0).all() and v["stats"].tolist() == [1, 0, int(rank < 3), 0]      # an axis-aligned flat: exact
    assert lam[0] == lam[1] == lam[2] == 5.25 and v["extent"][0].tolist() == [-3.5] * 3 + [3.5] * 3


def test_a_thin_diagonal_plate():
    occ = np.zeros((24, 10, 25), bool)
    for i in range(24):
        occ[i, :, i] = occ[i, :, i + 1] = True
    g, cells = lattice(occ, rows_per_cell=2)
    seg, (v, _) = check(g, what="diagonal plate")
    lam, ax = v["eigenvalues"][0], v["axes"][0]
    assert v["stats"][0] == 1 and lam[0] > 90 and 8 < lam[1] < 9 and lam[2] < 0.2
    assert abs(abs(ax[2] @ np.array([1, 0, -1]) / np.sqrt(2)) - 1) < 1e-3 and abs(ax[1, 1]) > 0.999      # the plate's normal
    assert v["extent"][0, 5] - v["extent"][0, 2] < 1.0 < 30 < v["extent"][0, 3] - v["extent"][0, 0]


# --------------------------------------------------------------------------------------------------- 4: random labels
@pytest.fixture(scope="module")
def dense():
    return lattice(np.ones((12, 12, 12), bool), rows_per_cell=2)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_random_labels_of_13_classes(dense, connectivity):
    g, cells = dense
    lab = np.random.default_rng(1300 + connectivity).integers(0, 13, cells.shape[0]).astype(np.int32)
    seg, (v, r) = check(g, lab, 13, connectivity, "13 classes at %d" % connectivity)
    assert np.array_equal(r["moments"][:, 0], 2 * v["moments"][:, 0]) and v["stats"][0] > 13


def test_filler_rows_a_cut_short_labels_and_labels_out_of_range():
    occ = np.random.default_rng(5).random((9, 8, 7)) < 0.6
    occ[0, 0, 0] = True
    V = int(occ.sum())
    g, cells = lattice(occ, rows_per_cell=2, trim=False)                    # M = 2 V rows, V of them filler
    assert g.voxel_count.shape[0] == 2 * V and int(g.stats[0]) == V
    rng = np.random.default_rng(6)
    seg, (v, _) = check(g, connectivity=18, what="untrimmed, no labels")
    S = v["stats"][0]
    assert v["cell_box"][S:].tolist() == [[0, 0, 0, -1, -1, -1]] * (2 * V - S) and not v["moments"][S:].any()
    for L in (2 * V, V - 5, 1, 0):
        lab = rng.integers(-1, 4, L).astype(np.int32)                       # -1 and 3 are out of range at num_class 3
        check(g, lab, 3, 26, "untrimmed, L = %d" % L, weights=("rows",))
    cut = V - 40
    gc, _ = lattice(occ, rows_per_cell=2, trim=False, max_voxels=cut)       # ne = cut = M, read on the device
    assert int(gc.stats[0]) == cut
    check(gc, rng.integers(0, 3, cut).astype(np.int32), 3, 6, "cut")
    # a segmentation whose words the geometry must not trust: ne below the segmented voxels, and words outside [0, S)
    import torch
    seg = g.segments(torch.from_numpy(rng.integers(0, 3, V).astype(np.int32)).to(g.data.device), 3, 26)
    geo_all = host(seg.geometry())
    g.stats[0] = cut                                                        # the voxels from cut on are members of nothing now
    seg.segment[5] = int(seg.stats[0])                                      # = S: outside
    seg.segment[6] = -3
    geo = seg.geometry()
    got = host(geo)
    want = gg.geometry_ref(g.data.cpu().numpy(), g.voxel_cell.cpu().numpy(), g.voxel_count.cpu().numpy(),
                           seg.segment.cpu().numpy(), int(seg.stats[0]), cut, 0, got["eigenvalues"], got["axes"])
    same(got, want, "ne below the segmentation's")
    assert not np.array_equal(got["moments"], geo_all["moments"]) and max(gg.figures(got["moments"], got["stats"][0],
                                                                                     got["eigenvalues"], got["axes"])) <= T_U
    g.stats[0] = V


# ------------------------------------------------------------------------------------------------ 5: the representatives
def test_center_and_mean_representatives_and_the_two_zeros():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    rows = np.array([[-0.0, 0.125, 0.125], [0.0, 0.5, 0.125], [0.375, 0.125, 0.125], [0.0, 0.75, 0.125]], F)
    g = grid.grid_subsample(torch.from_numpy(rows).to(dev), None, voxel=0.25, mode="center").trim()
    assert g.voxel_cell.tolist() == [[0, 0, 0], [0, 1, 0], [0, 2, 0], [1, 0, 0]]
    assert np.array_equal(g.data.cpu().numpy().view(np.uint32), rows[[0, 1, 3, 2]].view(np.uint32))       # center: rows as they are
    seg, (v,) = check(g, np.array([0, 0, 0, 1], np.int32), 2, 6, "two zeros", weights=("voxels",))
    box = v["box"][0]
    assert box[0] == 0 and np.signbit(box[0]) and box[3] == 0 and not np.signbit(box[3])       # -0.0 is below +0.0
    assert box.tolist()[1:3] == [0.125, 0.125] and box.tolist()[4:] == [0.75, 0.125] and v["stats"].tolist() == [2, 1, 2, 0]
    cloud = np.random.default_rng(9).random((3000, 4)).astype(F) * F(2.0) - F(1.0)
    lab = None
    for mode in ("center", "mean"):
        g = grid.grid_subsample(torch.from_numpy(cloud).to(dev), None, voxel=0.125, mode=mode).trim()
        lab = (g.voxel_cell[:, 0] // 5 + g.voxel_cell[:, 2] // 7).to(torch.int32).cpu().numpy() % 4
        seg, (v, r) = check(g, lab.astype(np.int32), 4, 18, "a cloud, mode " + mode)
        S = v["stats"][0]
        # every representative lies in its cell, so box lies in the cell box mapped to space (one float32 ulp for the division)
        lo = cloud[:, :3].min(axis=0)
        low = lo + v["cell_box"][:S, :3] * F(0.125)
        high = lo + (v["cell_box"][:S, 3:] + 1) * F(0.125)
        assert (v["box"][:S, :3] >= low - 1e-6).all() and (v["box"][:S, 3:] <= high + 1e-6).all()
        assert r["moments"][:S, 0].sum() == 3000


# ------------------------------------------------------------------------------------------------------- 6: many clouds
def room_cloud(n, seed):
    from pointwise_amd import synth
    xyz = synth.room_like(1, n, seed, (3.2, 2.4, 3.0))[0]
    return np.concatenate([xyz, np.random.default_rng(seed).random((n, 1))], axis=1).astype(F)


def test_two_rooms_that_overlap_in_space():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    a, b = room_cloud(3000, 7401), room_cloud(2500, 7402)
    both = torch.from_numpy(np.concatenate([a, b])).to(dev)
    start = torch.tensor([0, 3000, 5500], dtype=torch.int32, device=dev)
    g = grid.grid_subsample_rooms(both, start, None, voxel=0.1).trim()
    lab = (g.data[:, 2] > 1.2).to(torch.int32).cpu().numpy().astype(np.int32)
    vs = g.voxel_start.cpu().numpy()
    seg, (v, r) = check(g, lab, 2, 26, "two rooms")
    base = 0
    for k, cloud in enumerate((a, b)):                   # boxes per room lattice: what the room alone gives
        one = grid.grid_subsample(torch.from_numpy(cloud).to(dev), None, voxel=0.1).trim()
        s1, (v1, r1) = check(one, lab[vs[k]:vs[k + 1]], 2, 26, "room %d alone" % k)
        n = v1["stats"][0]
        for got, mine in ((v, v1), (r, r1)):
            for key in ("cell_box", "box", "moments", "centroid", "eigenvalues", "axes", "extent"):
                assert np.array_equal(bits(got[key][base:base + n]), bits(mine[key][:n])), (k, key)
        base += n
    assert base == v["stats"][0] and (v["cell_box"][:base, :3].min(axis=0) == 0).all()


# ------------------------------------------------------------------------------------- 7: reuse, reproducibility, streams
def test_out_reuse_two_runs_a_side_stream_and_absorb(dense):
    import torch
    g, cells = dense
    dev = g.voxel_count.device
    lab = torch.from_numpy(np.random.default_rng(77).integers(0, 5, cells.shape[0]).astype(np.int32)).to(dev)
    many = g.segments(lab, 5, 6)
    geo = many.geometry("rows")
    first, _ = check_geometry(g, many, "rows", "many segments", geo=geo)
    few = g.segments((lab > 2).to(torch.int32), 2, 26)
    assert few.num_segments() < many.num_segments()
    again = few.geometry("rows", out=geo)                # stale rows of the call before become filler
    assert again is geo
    got, _ = check_geometry(g, few, "rows", "out= reuse", geo=geo)
    S = got["stats"][0]
    assert got["cell_box"][S:].tolist() == [[0, 0, 0, -1, -1, -1]] * (cells.shape[0] - S) and first["moments"][S:].any()
    same(host(few.geometry("rows")), got, "a second run", EXACT + ("eigenvalues", "axes"))
    same(host(many.geometry("rows")), first, "two runs", EXACT + ("eigenvalues", "axes"))
    many.absorb(4)                                        # the geometry still describes the segmentation as segmented
    same(host(many.geometry("rows")), first, "after absorb", EXACT + ("eigenvalues", "axes"))
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = g.segments(lab, 5, 6).geometry("rows")
    side.synchronize()
    same(host(third), first, "side stream", EXACT + ("eigenvalues", "axes"))
