"""GPU tests (-m gpu) of GridSubsample.segments / clean_labels and GridSegments.absorb on conv3p_grid_segments and
conv3p_grid_absorb_segments: every output, the stats included, bit for bit against tests/grid_segments_ref.py on the
device's own neighbour table (tests/test_grid_interp.py checks the table) -- the hand cases and checkerboards of
tests/test_grid_segments_host.py; a snake and a comb, whose roots merge late; random labels on a dense lattice at the three
connectivities; one segment of 65 536 voxels; slabs of 2^20 voxels known in closed form; a sparse room with real voxel counts; filler rows, a max_voxels cut, L < ne,
labels out of range, no labels, one voxel, no voxel; two rooms that overlap in space; the absorb on all of these;
reproducibility and a side stream."""
import numpy as np
import pytest

from tests import grid_segments_ref as gs

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ("segment", "root", "size", "rows", "label", "stats")


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


def host(seg):
    return {k: getattr(seg, k).cpu().numpy() for k in OUTPUTS}


def same(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


def check(g, labels=None, num_class=None, connectivity=26, what="", absorb=()):
    """segments() against the reference, then absorb(min_size, drop) for every pair of `absorb` -> (device, reference)."""
    import torch
    lab_t = torch.from_numpy(labels).to(g.voxel_count.device) if labels is not None else None
    seg = g.segments(lab_t, num_class, connectivity)
    neigh, count, ne = g.neighbors().cpu().numpy(), g.voxel_count.cpu().numpy(), int(g.stats[0])
    M = neigh.shape[0]
    L = labels.shape[0] if labels is not None else 0
    got = host(seg)
    want = gs.segments_ref(neigh, labels, L, count, ne, num_class, connectivity)
    same(got, want, what)
    S = seg.num_segments()
    assert S == want["stats"][0] and int(want["stats"][1:4].sum()) == M and seg.trim().root.shape == (S,)
    for min_size, drop in absorb:
        out = seg.absorb(min_size, drop)
        ref = gs.absorb_ref(neigh, labels, L, want, ne, num_class, connectivity, min_size, drop)
        tag = "%s: absorb(%d, %s)" % (what, min_size, drop)
        same({"labels": out.cpu().numpy(), "seg_label": seg.absorbed_label.cpu().numpy(), "stats": seg.absorb_stats.cpu().numpy()},
             ref, tag)
        st = ref["stats"]
        assert st[0] == st[1] + st[2] and st[0] == (want["size"][:S] < min_size).sum(), tag
    return got, want


# ------------------------------------------------------------------------------------------------ 1: cases known by hand
def test_the_hand_cases():
    occ = np.zeros((2, 2, 1), bool)
    occ[0, 0, 0] = occ[1, 0, 0] = occ[1, 1, 0] = True
    g, _ = lattice(occ, rows_per_cell=3)
    for c in (6, 18, 26):
        got, _ = check(g, connectivity=c, what="an L at %d" % c, absorb=((2, True), (4, True), (4, False)))
        assert got["segment"].tolist() == [0, 0, 0] and got["stats"].tolist() == [1, 3, 0, 0, 3, 9, 0, 0]
    for cell, counts in (((1, 1, 0), [2, 1, 1]), ((1, 1, 1), [2, 2, 1])):
        occ = np.zeros((2, 2, 2), bool)
        occ[0, 0, 0] = occ[cell] = True
        g, _ = lattice(occ)
        assert [check(g, connectivity=c, what="a diagonal pair")[0]["stats"][0] for c in (6, 18, 26)] == counts
    # a line of labels: split by class, out-of-range labels in no segment, a tie to the lowest class, an orphan
    g, _ = lattice(np.ones((7, 1, 1), bool))
    got, _ = check(g, np.array([2, 2, 2, 3, 1, 1, 1], np.int32), 4, 6, "a tie", absorb=((2, False),))
    assert g.clean_labels(_t(g, [2, 2, 2, 3, 1, 1, 1]), 4, 2, connectivity=6).tolist() == [2, 2, 2, 1, 1, 1, 1]
    g, _ = lattice(np.ones((6, 1, 1), bool))
    check(g, np.array([0, 0, 0, 2, 1, 1], np.int32), 3, 6, "a small neighbour", absorb=((3, False), (3, True), (1, True)))
    assert g.clean_labels(_t(g, [0, 0, 0, 2, 1, 1]), 3, 3, connectivity=6, drop_orphans=True).tolist() == [0, 0, 0, 0, -1, -1]
    got, _ = check(g, np.array([1, 1, 0, 1, 5, -1], np.int32), 2, 6, "labels out of range", absorb=((2, False), (1, False)))
    assert got["segment"].tolist() == [0, 0, 1, 2, -1, -1]


def _t(g, values):
    import torch
    return torch.tensor(values, dtype=torch.int32, device=g.voxel_count.device)


def test_the_checkerboards():
    g, cells = lattice(np.ones((17, 16, 8), bool))       # 2176 voxels: past one tile of the numbering's scan
    lab = (cells.sum(axis=1) % 2).astype(np.int32)
    got, _ = check(g, lab, 2, 6, "checkerboard at 6", absorb=((2, False), (2, True)))
    assert got["stats"][0] == 2176 and np.array_equal(got["segment"], np.arange(2176)) and (got["size"] == 1).all()
    for c in (18, 26):
        got, _ = check(g, lab, 2, c, "checkerboard at %d" % c, absorb=((4, False),))
        assert got["stats"][0] == 2 and np.array_equal(got["segment"], lab)


# --------------------------------------------------------------------------------- 2: shapes whose roots merge late
def snake(n=24):
    """A one-voxel-wide path folded back and forth through n x n x 3: layer 0 runs along j and turns at alternating ends,
    layer 2 does the same along i, and one cell of layer 1 joins the two.  Voxel numbers along it rise and fall."""
    occ = np.zeros((n, n, 3), bool)
    occ[0::2, :, 0] = True
    for i in range(1, n - 1, 2):
        occ[i, n - 1 if (i // 2) % 2 == 0 else 0, 0] = True
    occ[:, 0::2, 2] = True
    for j in range(1, n - 1, 2):
        occ[n - 1 if (j // 2) % 2 == 0 else 0, j, 2] = True
    occ[n - 2, n - 1, 1] = occ[n - 2, n - 1, 2] = True   # from the end of layer 0's last row up to layer 2's last column
    return occ


@pytest.mark.parametrize("n", [24, 64])                  # 600 voxels: one tile of the union-find in LDS; 4160: five tiles
@pytest.mark.parametrize("connectivity", [6, 26])
def test_a_snake_is_one_segment(connectivity, n):
    g, cells = lattice(snake(n))
    got, want = check(g, connectivity=connectivity, what="snake", absorb=((5, True),))
    M = cells.shape[0]
    assert got["stats"][0] == 1 and (got["segment"] == 0).all() and got["size"][0] == M and got["root"][0] == 0
    # with labels along it: pieces of one class each, and a clean-up that joins nothing across classes
    lab = ((cells[:, 0] // 6 + cells[:, 1] // 6) % 3).astype(np.int32)
    check(g, lab, 3, connectivity, "labelled snake", absorb=((3, False), (12, True)))


@pytest.mark.parametrize("connectivity", [6, 18])
def test_a_comb_with_the_spine_at_the_high_end(connectivity):
    occ = np.zeros((24, 23, 2), bool)
    occ[:, 0::2, 0] = True                               # teeth along i, the slowest axis
    occ[23, :, 0] = True                                 # the spine: the highest voxel numbers
    g, cells = lattice(occ)
    got, _ = check(g, connectivity=connectivity, what="comb")
    assert got["stats"][0] == 1 and got["size"][0] == cells.shape[0]
    occ[23, 5, 0] = False                                # a gap in the spine at 6: two combs
    g, cells = lattice(occ)
    got, _ = check(g, connectivity=6, what="cut comb", absorb=((60, True),))
    assert got["stats"][0] == 2 and got["size"][0] + got["size"][1] == cells.shape[0]


# --------------------------------------------------------------------------------------------------- 3: random labels
@pytest.fixture(scope="module")
def dense():
    return lattice(np.ones((12, 12, 12), bool), rows_per_cell=2)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("num_class", [3, 13])
def test_random_labels_on_a_dense_lattice(dense, num_class, connectivity):
    g, cells = dense
    lab = np.random.default_rng(num_class * 100 + connectivity).integers(0, num_class, cells.shape[0]).astype(np.int32)
    got, want = check(g, lab, num_class, connectivity, "random %d classes at %d" % (num_class, connectivity),
                      absorb=((2, False), (4, False), (9, True)))
    assert np.array_equal(got["label"][got["segment"]], lab) and (got["rows"][:got["stats"][0]] == 2 * got["size"][:got["stats"][0]]).all()


def test_one_segment_of_65536_voxels():
    g, cells = lattice(np.ones((128, 128, 4), bool))
    lab = np.zeros(65536, np.int32)
    got, _ = check(g, lab, 1, 6, "slab", absorb=((70000, False),))
    assert got["stats"].tolist() == [1, 65536, 0, 0, 65536, 65536, 0, 0] and (got["segment"] == 0).all()


def test_slabs_of_a_million_voxels_in_closed_form():
    # 2^20 voxels: where a wave of the size adds takes 16 steps of consecutive voxels.  Slabs of 20 cells along the slowest
    # axis, classes 0, 1, 2 in turn, at connectivity 6: segment k is slab k, whatever the reference would take to say so.
    import torch
    n = (128, 128, 64)
    g, cells = lattice(np.ones(n, bool))
    M, per = cells.shape[0], 20 * n[1] * n[2]
    slab = cells[:, 0] // 20
    seg = g.segments(torch.from_numpy((slab % 3).astype(np.int32)).to(g.voxel_count.device), 3, 6)
    got = host(seg)
    S = 7
    sizes = np.array([per] * 6 + [M - 6 * per], np.int32)
    assert M == 1 << 20 and got["stats"].tolist() == [S, M, 0, 0, per, per, 0, 0]
    assert np.array_equal(got["segment"], slab) and np.array_equal(got["root"][:S], np.arange(S) * per)
    assert np.array_equal(got["size"][:S], sizes) and np.array_equal(got["rows"][:S], sizes)
    assert got["label"][:S].tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert (got["root"][S:] == -1).all() and not got["size"][S:].any() and not got["rows"][S:].any() and (got["label"][S:] == -1).all()
    out = seg.absorb(per, drop_orphans=True).cpu().numpy()                # the last slab is smaller: it hears slab 5, class 2
    assert np.array_equal(out, np.where(slab == 6, 2, slab % 3)) and seg.absorb_stats.tolist() == [1, 1, 0, M - 6 * per]


# ---------------------------------------------------------------------------------------------------------- 4: a room
def room_cloud(n=6000, seed=7301):
    from pointwise_amd import synth
    xyz = synth.room_like(1, n, seed, (3.2, 2.4, 3.0))[0]
    return np.concatenate([xyz, np.random.default_rng(seed).random((n, 1))], axis=1).astype(F)


def test_a_sparse_room_with_real_counts_and_outlier_removal():
    import torch
    from pointwise_amd import grid
    data = room_cloud()
    data[11, 1] = np.nan
    g = grid.grid_subsample(torch.from_numpy(data).to(_dev()), None, voxel=0.08).trim()
    got, want = check(g, connectivity=26, what="room, geometric", absorb=((4, True), (4, False)))
    S = got["stats"][0]
    assert S > 1 and got["rows"][:S].sum() == data.shape[0] - 1 and got["stats"][5] == got["rows"].max() > got["stats"][4]
    out = g.segments().absorb(4, drop_orphans=True).cpu().numpy()
    small = got["size"][got["segment"]] < 4
    assert small.any() and (out[small] == -1).all() and (out[~small] == 0).all()        # floating clusters are dropped
    assert g.segments().absorb_stats is None
    rows = g.project(g.segments().segment).cpu().numpy()                                  # a segment number per raw row
    inv = g.inverse.cpu().numpy()
    assert rows[11] == -1 and np.array_equal(rows[inv >= 0], got["segment"][inv[inv >= 0]])
    lab = (g.data[:, 2] > 1.5).to(torch.int32).cpu().numpy() + 2 * (g.data[:, 0] > 1.6).to(torch.int32).cpu().numpy()
    check(g, lab.astype(np.int32), 4, 18, "room, four classes", absorb=((3, False), (20, True)))


# --------------------------------------------------------------------------------------------------------- 5: the edges
def test_filler_rows_a_cut_and_short_labels():
    occ = np.random.default_rng(5).random((9, 8, 7)) < 0.6
    occ[0, 0, 0] = True
    V = int(occ.sum())
    g, cells = lattice(occ, rows_per_cell=2, trim=False)                    # M = 2 V rows, V of them filler
    assert g.voxel_count.shape[0] == 2 * V and int(g.stats[0]) == V
    rng = np.random.default_rng(6)
    got, _ = check(g, connectivity=18, what="untrimmed, geometric", absorb=((3, True),))
    assert got["stats"][3] == V and (got["segment"][V:] == -1).all()
    for L in (2 * V, V, V - 5, 1, 0):
        lab = rng.integers(-1, 4, L).astype(np.int32)                       # -1 and 3 are out of range at num_class 3
        check(g, lab, 3, 26, "untrimmed, L = %d" % L, absorb=((3, False), (3, True)))
    cut = V - 40
    gc, _ = lattice(occ, rows_per_cell=2, trim=False, max_voxels=cut)       # ne = cut = M, read on the device
    assert int(gc.stats[0]) == cut and int(gc.stats[1]) == V
    check(gc, rng.integers(0, 3, cut).astype(np.int32), 3, 6, "cut", absorb=((2, False),))
    # ne < M: the same voxels as `g` holds, but the stats say that fewer were emitted
    g.stats[0] = cut
    got, _ = check(g, rng.integers(0, 3, V).astype(np.int32), 3, 26, "ne below the table's voxels", absorb=((4, True),))
    assert got["stats"][3] == 2 * V - cut and (got["segment"][cut:] == -1).all()


def test_one_voxel_and_no_voxel():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    g = grid.grid_subsample(torch.tensor([[0.3, -1.0, 2.0, 5.0]], device=dev), None, voxel=0.1)
    got, _ = check(g, what="one voxel", absorb=((1, True), (2, True), (2, False)))
    assert got["segment"].tolist() == [0] and got["stats"].tolist() == [1, 1, 0, 0, 1, 1, 0, 0]
    check(g, np.array([4], np.int32), 5, 6, "one labelled voxel", absorb=((2, False),))
    check(g, np.array([5], np.int32), 5, 6, "one voxel out of range", absorb=((2, False),))
    g = grid.grid_subsample(torch.full((3, 3), float("nan"), device=dev), None, voxel=0.1)     # nothing emitted
    got, _ = check(g, what="nothing emitted", absorb=((2, True),))
    assert got["stats"].tolist() == [0, 0, 0, 3, 0, 0, 0, 0] and (got["segment"] == -1).all() and (got["root"] == -1).all()
    check(g, np.array([0, 1], np.int32), 2, 26, "nothing emitted, labels", absorb=((2, False),))
    t = g.trim()                                          # no rows at all: nothing is launched
    seg = t.segments()
    assert seg.segment.shape == (0,) and seg.num_segments() == 0 and seg.absorb(3).shape == (0,)
    assert seg.absorb_stats.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------- 6: many clouds
def test_two_rooms_that_overlap_in_space():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    a, b = room_cloud(3000, 7401), room_cloud(2500, 7402)
    both = torch.from_numpy(np.concatenate([a, b])).to(dev)
    start = torch.tensor([0, 3000, 5500], dtype=torch.int32, device=dev)
    g = grid.grid_subsample_rooms(both, start, None, voxel=0.1).trim()
    vs = g.voxel_start.cpu().numpy()
    lab = (g.data[:, 2] > 1.2).to(torch.int32).cpu().numpy().astype(np.int32)
    for labels, nc, what in ((None, None, "geometric"), (lab, 2, "two classes")):
        got, _ = check(g, labels, nc, 26, "two rooms, " + what, absorb=((3, True),))
        S = got["stats"][0]
        room_of_voxel = g.voxel_room.cpu().numpy()
        assert (room_of_voxel[got["root"][:S]][got["segment"]] == room_of_voxel).all()      # no segment holds two rooms
        assert (np.diff(room_of_voxel[got["root"][:S]]) >= 0).all()                         # numbered room after room
        base = 0
        for r, cloud in enumerate((a, b)):
            one = grid.grid_subsample(torch.from_numpy(cloud).to(dev), None, voxel=0.1).trim()
            part = labels[vs[r]:vs[r + 1]] if labels is not None else None
            mine, _ = check(one, part, nc, 26, "room %d alone, %s" % (r, what))
            s = mine["stats"][0]
            assert np.array_equal(got["segment"][vs[r]:vs[r + 1]], np.where(mine["segment"] >= 0, mine["segment"] + base, -1))
            assert np.array_equal(got["root"][base:base + s], mine["root"][:s] + vs[r])
            for k in ("size", "rows", "label"):
                assert np.array_equal(got[k][base:base + s], mine[k][:s])
            base += s
        assert base == S


# ------------------------------------------------------------------------------------- 7: reuse, reproducibility, streams
def test_out_reuse_two_calls_and_a_side_stream(dense):
    import torch
    g, cells = dense
    dev = g.voxel_count.device
    lab = torch.from_numpy(np.random.default_rng(77).integers(0, 5, cells.shape[0]).astype(np.int32)).to(dev)
    first = g.segments(lab, 5, 18)
    a = host(first)
    la = first.absorb(4).clone()
    sa, ta = first.absorbed_label.clone(), first.absorb_stats.clone()
    other = g.segments(torch.zeros_like(lab), 5, 18, out=first)             # the same object, other labels, then back
    assert other is first and first.num_segments() == 1
    again = g.segments(lab, 5, 18, out=first)
    same(host(again), a, "out= reuse")
    buf = torch.full_like(la, 99)
    lb = again.absorb(4, out=buf)
    assert lb is buf and torch.equal(lb, la) and torch.equal(again.absorbed_label, sa) and torch.equal(again.absorb_stats, ta)
    assert torch.equal(g.clean_labels(lab, 5, 4, connectivity=18), la)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = g.segments(lab, 5, 18)
        lc = third.absorb(4)
    side.synchronize()
    same(host(third), a, "side stream")
    assert torch.equal(lc, la) and torch.equal(third.absorb_stats, ta)
