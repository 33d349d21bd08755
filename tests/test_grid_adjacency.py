"""GPU tests (-m gpu) of GridSegments.adjacency / merge and SegmentAdjacency.merge on conv3p_grid_segment_adjacency and
conv3p_grid_merge_segments: every output, the stats included, bit for bit against tests/grid_adjacency_ref.py on the
device's own neighbour table and segmentation (tests/test_grid_interp.py and tests/test_grid_segments.py check those) -- the
hand cases, the checkerboard and the slabs of tests/test_grid_adjacency_host.py; a star whose centre has 1024 neighbours;
random labels at the three connectivities; one segment of 65 536 voxels; two slabs of 131 072 voxels, the contended edge;
filler rows, a max_voxels cut, segment words out of range, one voxel, no voxel; two rooms that overlap in space; the
merge, the merged object's geometry and its own adjacency; reproducibility and a side stream."""
import numpy as np
import pytest

from tests import grid_adjacency_ref as ga
from tests import grid_segments_ref as gs
from tests.test_grid_geometry import check_geometry, lattice

pytestmark = pytest.mark.gpu
ADJ = ("start", "src", "dst", "contacts", "voxels", "offset", "twin", "border", "stats")
SEG = ("segment", "root", "size", "rows", "label", "stats")


def host(obj, keys):
    return {k: getattr(obj, k).cpu().numpy() for k in keys}


def same(got, want, what):
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s: %s" % (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


def segment(g, labels=None, num_class=None, connectivity=26):
    import torch
    lab_t = torch.from_numpy(np.asarray(labels, np.int32)).to(g.voxel_count.device) if labels is not None else None
    return g.segments(lab_t, num_class, connectivity)


def check_adj(g, seg, connectivity=None, max_edges=None, what="", adj=None):
    """seg.adjacency against the reference on the device's own table and segment words -> (device outputs, the object)."""
    adj = seg.adjacency(connectivity, max_edges) if adj is None else adj
    M = seg.segment.shape[0]
    assert adj.shape == (M, 2 * M if max_edges is None else max_edges)
    want = ga.adjacency_ref(g.neighbors().cpu().numpy(), seg.segment.cpu().numpy(), int(seg.stats[0]), int(g.stats[0]),
                            seg._source[4] if connectivity is None else connectivity, adj.shape[1])
    got = host(adj, ADJ)
    same(got, want, what)
    E = adj.num_edges()
    assert adj.overflowed() == (E < 0) and adj.edges_bound() == want["stats"][1] and adj.trim().src.shape == (max(E, 0),)
    return got, adj


def check_merge(seg, pair_a, pair_b, select=None, what="", merged=None):
    """seg.merge against the reference on the device's own segmentation -> (device outputs, the object)."""
    merged = seg.merge(pair_a, pair_b, select) if merged is None else merged
    want = ga.merge_ref(host(seg, SEG), pair_a.cpu().numpy(), pair_b.cpu().numpy(), None if select is None else select.cpu().numpy())
    got = host(merged, SEG + ("seg_map", "merge_stats"))
    same(got, want, what)
    assert merged.num_segments() == want["merge_stats"][0]
    return got, merged


# ------------------------------------------------------------------------------------------------ 1: cases known by hand
def test_the_hand_cases():
    g, _ = lattice(np.ones((2, 1, 1), bool))
    got, _ = check_adj(g, segment(g, [0, 1], 2, 6), what="two voxels")
    assert got["src"][:2].tolist() == [0, 1] and got["offset"][:2].tolist() == [[1, 0, 0], [-1, 0, 0]] and got["twin"][:2].tolist() == [1, 0]
    assert got["border"].tolist() == [[1, 0, 5, 1], [1, 0, 5, 1]] and got["stats"].tolist() == [2, 2, 2, 2, 1, 1, 0, 0]
    assert got["start"].tolist() == [0, 1, 2] and got["src"][2:].tolist() == [-1, -1]
    g, _ = lattice(np.ones((6, 1, 1), bool))
    seg = segment(g, [1, 1, 0, 1, 5, -1], 2, 6)
    got, _ = check_adj(g, seg, what="the line at 6")
    assert got["stats"][0] == 4 and got["border"][:3].tolist() == [[1, 0, 9, 2], [2, 0, 4, 1], [1, 1, 4, 1]]
    got, _ = check_adj(g, seg, 26, what="the line at 26")
    assert got["border"][:3, 2].tolist() == [49, 24, 24]
    for cap in (4, 3, 0):
        got, adj = check_adj(g, seg, 18, cap, "the line, max_edges %d" % cap)
        assert adj.num_edges() == (4 if cap == 4 else -1) and adj.edges_bound() == 4
    occ = np.zeros((2, 2, 2), bool)
    occ[0, 0, 0] = occ[1, 1, 1] = True
    g, _ = lattice(occ)
    seg = segment(g, [0, 0], 1, 6)                       # one label, two segments at 6 ...
    assert seg.num_segments() == 2
    assert [check_adj(g, seg, c, what="a corner pair")[0]["stats"][0] for c in (6, 18, 26)] == [0, 0, 2]    # ... that touch at 26
    assert seg.adjacency(26).offset[:2].tolist() == [[1, 1, 1], [-1, -1, -1]]


@pytest.mark.parametrize("connectivity,edges", [(6, 11984), (18, 33972), (26, 47412)])
def test_the_checkerboard_overflows_the_default_and_fits_its_bound(connectivity, edges):
    g, cells = lattice(np.ones((17, 16, 8), bool))       # 2176 voxels: past one tile of 1024 and one scan tile of 2048
    seg = segment(g, cells.sum(axis=1) % 2, 2, 6)
    assert seg.num_segments() == 2176
    got, adj = check_adj(g, seg, connectivity, what="checkerboard, default max_edges")
    assert adj.shape[1] == 4352 and adj.overflowed() and got["stats"].tolist() == [-1, edges, 2176, edges, 0, 0, 1, 0]
    got, adj = check_adj(g, seg, connectivity, adj.edges_bound(), "checkerboard, the retry")
    assert got["stats"].tolist() == [edges, edges, 2176, edges, connectivity, 1, 0, 0] and (got["contacts"] == 1).all()
    check_adj(g, seg, connectivity, edges + 1000, "checkerboard, room to spare")


@pytest.mark.parametrize("connectivity,contacts", [(6, 4096), (18, 20224), (26, 36100)])
def test_two_thin_slabs(connectivity, contacts):
    g, cells = lattice(np.ones((64, 64, 2), bool))
    got, _ = check_adj(g, segment(g, cells[:, 2], 2, 26), connectivity, what="thin slabs")
    assert got["stats"].tolist() == [2, 8192, 2, 2 * contacts, 1, contacts, 0, 0]
    assert got["offset"][:2].tolist() == [[0, 0, contacts], [0, 0, -contacts]] and got["voxels"][:2].tolist() == [4096, 4096]


def test_a_star():
    g, cells = lattice(np.ones((32, 32, 2), bool))       # a plane of class 0 under a checkerboard of classes 1 and 2
    lab = np.where(cells[:, 2] == 0, 0, 1 + (cells[:, 0] + cells[:, 1]) % 2)
    seg = segment(g, lab, 3, 6)
    assert seg.num_segments() == 1025
    got, _ = check_adj(g, seg, 6, 6016, "star at 6")
    assert got["stats"][0] == 6016 and got["stats"][4] == 1024 and got["border"][0].tolist() == [1024, 0, 1152, 1024]
    assert got["start"][:2].tolist() == [0, 1024]
    got, adj = check_adj(g, seg, 26, 17672, "star at 26")
    assert got["stats"][:2].tolist() == [9860, 17672] and adj.trim().dst.shape == (9860,)


# ------------------------------------------------------------------------------------------------------- 2: larger fields
@pytest.mark.parametrize("made_at,connectivity", [(26, 6), (6, 18), (18, 26), (26, 26)])
def test_random_labels(made_at, connectivity):
    g, cells = lattice(np.ones((24, 24, 24), bool))
    lab = np.random.default_rng(5).integers(0, 13, cells.shape[0])
    seg = segment(g, lab, 13, made_at)
    got, _ = check_adj(g, seg, connectivity, 26 * cells.shape[0], "random labels")
    if (made_at, connectivity) == (26, 26):
        assert got["stats"][0] == 102438 and got["stats"][2] == 4117


def test_one_segment_of_65536_voxels():
    g, cells = lattice(np.ones((64, 32, 32), bool))
    got, _ = check_adj(g, segment(g), 26, 1000, "one segment")
    assert got["stats"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and not got["start"].any()
    assert got["border"][0, :2].tolist() == [0, 0] and got["border"][0, 3] == 65536 - 62 * 30 * 30      # the box's shell


def test_two_thick_slabs_the_contended_edge():
    g, cells = lattice(np.ones((128, 128, 16), bool))    # 262 144 voxels
    got, _ = check_adj(g, segment(g, cells[:, 2] // 8, 2, 26), 26, 64, "thick slabs")
    c = (3 * 128 - 2) ** 2
    assert got["stats"].tolist() == [2, 2 * 128 * 128, 2, 2 * c, 1, c, 0, 0] and got["contacts"][:2].tolist() == [c, c]


# --------------------------------------------------------------------------------------------------------- 3: the edges
def test_filler_rows_a_cut_and_words_out_of_range():
    import torch
    occ = np.random.default_rng(5).random((9, 8, 7)) < 0.6
    occ[0, 0, 0] = True
    V = int(occ.sum())
    rng = np.random.default_rng(8)
    g, _ = lattice(occ, rows_per_cell=2, trim=False)     # M = 2 V rows, V of them filler
    seg = segment(g, rng.integers(-1, 4, 2 * V), 3, 18)
    got, _ = check_adj(g, seg, 26, what="untrimmed")
    assert not got["border"][V:].any() and got["border"][:, 1].any()
    cut = V - 40
    gc, _ = lattice(occ, rows_per_cell=2, trim=False, max_voxels=cut)
    check_adj(gc, segment(gc, rng.integers(0, 3, cut), 3, 6), 18, what="cut")
    g.stats[0] = cut                                     # ne below the table's voxels: those past it are members of nothing
    check_adj(g, seg, 26, what="ne below the voxels")
    g.stats[0] = V
    # any array with values in [-1, S) is legal, and words outside [0, S) make a voxel a member of nothing
    S = seg.num_segments()
    words = rng.integers(-1, S, 2 * V)
    words[::7] = np.resize(np.array([S, S + 5, -7, 2 ** 30, -2 ** 31, 2 ** 31 - 1, -1]), words[::7].size)
    seg.segment.copy_(torch.from_numpy(words.astype(np.int32)))
    check_adj(g, seg, 26, 26 * 2 * V, what="words out of range")
    seg.stats[0] = 2 * V + 9                             # S is held to M
    check_adj(g, seg, 6, 26 * 2 * V, what="S past M")


def test_one_voxel_and_no_voxel():
    import torch
    from pointwise_amd import grid
    from tests.test_grid_geometry import _dev
    dev = _dev()
    g = grid.grid_subsample(torch.tensor([[0.3, -1.0, 2.0, 5.0]], device=dev), None, voxel=0.1)
    seg = g.segments()
    got, adj = check_adj(g, seg, what="one voxel")
    assert got["stats"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and got["border"].tolist() == [[0, 0, 26, 1]] and got["start"].tolist() == [0, 0]
    check_adj(g, seg, 6, 0, "one voxel, no rows")
    got, _ = check_merge(seg, adj.src, adj.dst, what="one voxel")
    assert got["merge_stats"].tolist() == [1, 1, 0, 0]
    g = grid.grid_subsample(torch.full((3, 3), float("nan"), device=dev), None, voxel=0.1)     # nothing emitted
    seg = g.segments()
    got, adj = check_adj(g, seg, what="nothing emitted")
    assert not got["stats"].any() and not got["border"].any()
    check_merge(seg, adj.src, adj.dst, what="nothing emitted")
    seg = g.trim().segments()                            # no rows at all: nothing is launched
    adj = seg.adjacency()
    assert adj.start.tolist() == [0] and adj.src.shape == (0,) and adj.num_edges() == 0 and not adj.overflowed()
    assert adj.merge().num_segments() == 0 and adj.merge().merge_stats.tolist() == [0, 0, 0, 0]


def test_two_rooms_that_overlap_in_space_share_no_edge():
    import torch
    from pointwise_amd import grid
    from tests.test_grid_geometry import _dev
    from tests.test_grid_segments import room_cloud
    dev = _dev()
    both = torch.from_numpy(np.concatenate([room_cloud(3000, 7401), room_cloud(2500, 7402)])).to(dev)
    g = grid.grid_subsample_rooms(both, torch.tensor([0, 3000, 5500], dtype=torch.int32, device=dev), None, voxel=0.1).trim()
    lab = ((g.data[:, 2] > 1.2).to(torch.int32) + 2 * (g.data[:, 0] > 1.6).to(torch.int32)).cpu().numpy()
    seg = segment(g, lab, 4, 18)
    got, adj = check_adj(g, seg, 26, what="two rooms")
    E, S = adj.num_edges(), seg.num_segments()
    voxel_room = g.voxel_room.cpu().numpy()
    room = voxel_room[seg.root.cpu().numpy()[:S]]        # of every segment
    assert E > 0 and (room[got["src"][:E]] == room[got["dst"][:E]]).all() and len(set(room[got["src"][:E]])) == 2
    got, merged = check_merge(seg, adj.src, adj.dst, what="two rooms")        # everything that touches: no group holds two rooms
    assert (room == voxel_room[got["root"][got["seg_map"][:S]]]).all()


# --------------------------------------------------------------------------------------------------------------- 4: merge
def test_the_merge_cases():
    import torch
    g, _ = lattice(np.ones((7, 1, 1), bool))
    seg = segment(g, [2, 0, 0, 1, 1, 1, 3], 4, 6)
    dev = seg.segment.device

    def t(values, dtype=torch.int32):
        return torch.tensor(values, dtype=dtype, device=dev)

    got, _ = check_merge(seg, t([0, 1]), t([1, 2]), what="the label of the largest member")
    assert got["segment"].tolist() == [0, 0, 0, 0, 0, 0, 1] and got["label"][:2].tolist() == [1, 3] and got["merge_stats"].tolist() == [2, 4, 2, 1]
    got, _ = check_merge(seg, t([3]), t([0]), what="a tie, and one direction")
    assert got["label"][:3].tolist() == [2, 0, 1] and got["seg_map"][:4].tolist() == [0, 1, 2, 0]
    got, merged = check_merge(seg, t([-1, 4, 3, 0, 7]), t([0, 0, 3, 2 ** 30, -5]), what="filler and out of range")
    same(host(merged, SEG), host(seg, SEG), "nothing active")
    assert got["seg_map"].tolist() == [0, 1, 2, 3, -1, -1, -1]
    check_merge(seg, t([0, 1, 2]), t([1, 2, 3]), t([1, 0, 5]), what="select int32")
    got, _ = check_merge(seg, t([0, 1, 2]), t([1, 2, 3]), t([False, False, True], torch.bool), what="select bool")
    assert got["merge_stats"].tolist() == [3, 4, 1, 1]
    same(host(seg.merge(t([]), t([])), SEG), host(seg, SEG), "no pair")
    with pytest.raises(ValueError, match="absorb works on what segments"):
        seg.merge(t([]), t([])).absorb(2)
    # trim() carries what merge() added; segments(out=) into a merged object makes it a plain segmentation again
    merged = seg.merge(t([0, 1]), t([1, 2]))
    cut = merged.trim()
    assert cut.seg_map is merged.seg_map and cut.merge_stats is merged.merge_stats and cut.root.shape == (2,)
    with pytest.raises(ValueError, match="not on its trim"):
        cut.absorb(2)
    lab = t([2, 0, 0, 1, 1, 1, 3])
    again = g.segments(lab, 4, 6, out=merged)
    assert again is merged and again.seg_map is None and again.merge_stats is None and again.trim().seg_map is None
    same(host(again, SEG), host(seg, SEG), "segments(out=) over a merged object")
    assert torch.equal(again.absorb(2), seg.absorb(2))
    back = seg.merge(t([0, 1]), t([1, 2]), out=again)                       # and a merged one once more
    assert back.seg_map.tolist()[:4] == [0, 0, 0, 1] and back.merge_stats.tolist() == [2, 4, 2, 1]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_every_edge_merged_gives_the_geometric_components(connectivity):
    rng = np.random.default_rng(connectivity)
    occ = rng.random((20, 18, 16)) < 0.4
    occ[0, 0, 0] = True
    g, cells = lattice(occ, rows_per_cell=2)
    lab = rng.integers(-1, 4, cells.shape[0])
    seg = segment(g, lab, 4, connectivity)
    got, adj = check_adj(g, seg, None, 26 * cells.shape[0], "before the merge")
    none, _ = check_merge(seg, adj.src, adj.dst, adj.src < -1, what="none selected")
    same({k: none[k] for k in SEG}, host(seg, SEG), "none selected is the identity")
    got, merged = check_merge(seg, adj.src, adj.dst, what="all edges")
    want = host(segment(g, np.where(lab >= 0, 0, -1), 1, connectivity), SEG)
    for k in ("segment", "root", "size", "rows"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["stats"][:6], want["stats"][:6]) and got["stats"][0] < seg.num_segments()
    half, _ = check_merge(seg, adj.src, adj.dst, adj.src < adj.dst, what="one direction")
    same(half, {**got, "merge_stats": half["merge_stats"]}, "one direction is enough")
    # the merged object is a segmentation like any other
    for weight in ("voxels", "rows"):
        check_geometry(g, merged, weight, "merged")
    got2, adj2 = check_adj(g, merged, 26, what="the merged object's own adjacency")
    assert adj2.num_edges() == (0 if connectivity == 26 else got2["stats"][0])
    rows = g.project(merged.segment).cpu().numpy()
    inv = g.inverse.cpu().numpy()
    assert np.array_equal(rows, np.where(inv >= 0, got["segment"][np.maximum(inv, 0)], -1))
    again = adj.merge(out=merged)                        # SegmentAdjacency.merge, into the same object
    assert again is merged
    same(host(again, SEG + ("seg_map", "merge_stats")), got, "out= reuse")
    check_merge(merged, adj2.src, adj2.dst, what="a merge of a merge")


def test_an_alternating_line_becomes_one_group():
    g, _ = lattice(np.ones((4096, 1, 1), bool))
    seg = segment(g, np.arange(4096) % 2, 2, 6)
    got, adj = check_adj(g, seg, what="alternating line")
    assert got["stats"].tolist() == [8190, 8190, 4096, 8190, 2, 1, 0, 0]
    got, _ = check_merge(seg, adj.src, adj.dst, what="alternating line")
    assert got["stats"].tolist() == [1, 4096, 0, 0, 4096, 4096, 0, 0] and got["merge_stats"].tolist() == [1, 4096, 8190, 1]


# ------------------------------------------------------------------------------------- 5: reuse, reproducibility, streams
def test_out_reuse_two_calls_and_a_side_stream():
    import torch
    g, cells = lattice(np.ones((20, 20, 20), bool))
    dev = g.voxel_count.device
    seg = segment(g, np.random.default_rng(77).integers(0, 5, cells.shape[0]), 5, 18)
    a, first = check_adj(g, seg, 26, 26 * 8000, "first call")
    m, _ = check_merge(seg, first.src, first.dst, first.contacts > 9, what="first merge")
    other = segment(g, np.zeros(cells.shape[0]), 5, 18).adjacency(26, 26 * 8000, out=first)      # the same object, then back
    assert other is first and first.num_edges() == 0
    again = seg.adjacency(26, 26 * 8000, out=first)
    same(host(again, ADJ), a, "out= reuse")
    b = host(seg.adjacency(26, 26 * 8000), ADJ)
    same(b, a, "a second call")
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = seg.adjacency(26, 26 * 8000)
        merged = third.merge(third.contacts > 9)
    side.synchronize()
    same(host(third, ADJ), a, "side stream")
    same(host(merged, SEG + ("seg_map", "merge_stats")), m, "side stream, merge")
