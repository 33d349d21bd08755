"""GPU tests (-m gpu) of SegmentAdjacency.agglomerate on conv3p_grid_agglomerate_segments: every output word, the stats
included, bit for bit against tests/grid_agglomerate_ref.py on the device's own segmentation and adjacency
(tests/test_grid_adjacency.py checks those), and against the device's own merge() on the log and adjacency() of the
result -- random classes at the three connectivities with a tight table and a roomy one; a field past one scan tile and
two sort tiles; a chain across every tile; one segment with a thousand small neighbours; the cut of the rounds; smooth,
merged and many-clouds segmentations; an adjacency that overflowed; trimmed inputs; out= reuse; reproducibility."""
import numpy as np
import pytest

from tests import grid_agglomerate_ref as ar
from tests.test_grid_adjacency import ADJ, SEG, host, same, segment
from tests.test_grid_geometry import lattice

pytestmark = pytest.mark.gpu
MERGED = SEG + ("seg_map", "merge_stats")
GRAPH = ("start", "src", "dst", "contacts", "offset", "twin")
WEIGHTS = {"voxels": 0, "rows": 1}


def outputs(res):
    got = {"seg_map": res.segments.seg_map, "merge_stats": res.segments.merge_stats, "agg_stats": res.stats,
           "voxel_label": res.voxel_label}
    got.update({k: getattr(res.segments, k) for k in SEG})
    got.update({k: getattr(res, k) for k in ar.LOG_KEYS + GRAPH})
    return {k: v.cpu().numpy() for k, v in got.items()}


def check(seg, adj, what, converges=True, devices=True, res=None, **kw):
    """adj.agglomerate(**kw) against the reference on the device's own segmentation and adjacency, and (devices) against
    the device's merge() on the log and adjacency() of the result -> (device outputs, the object)."""
    res = adj.agglomerate(**kw) if res is None else res
    ref_kw = {**kw, "weight": WEIGHTS[kw.get("weight", "voxels")], "same_label": int(kw.get("same_label", False))}
    want = ar.agglomerate_ref(host(seg, SEG), host(adj, ADJ), **ref_kw)
    if converges:                                        # the reference reaches the fixed point within max_rounds
        assert want["agg_stats"][5] == 0 and want["agg_stats"][6] == 0, what
    got = outputs(res)
    assert set(got) == set(ar.ALL_KEYS)
    same(got, want, what)
    s = want["agg_stats"]
    assert (res.num_groups(), res.num_rounds(), res.converged()) == (s[0], s[2], s[5] == 0 and s[6] == 0), what
    assert s[3] == seg.num_segments() - s[0], what       # H6: a spanning forest
    t = res.trim()
    assert t.log_a.shape == (s[3],) and t.src.shape == (s[7],) and t.offset.shape == (s[7], 3) and t.segments is res.segments
    merged = res.segments
    assert merged._merged and merged.num_segments() == s[0]
    if devices:
        same(host(merged, MERGED), host(seg.merge(res.log_a, res.log_b), MERGED), what + ": merge() on the log")
        again = merged.adjacency(connectivity=adj.connectivity, max_edges=adj.shape[1])
        same({k: got[k] for k in GRAPH}, host(again, GRAPH), what + ": adjacency() of the result")
        assert again.num_edges() == s[7]
    return got, res


def field(shape, labels, made_at, connectivity, max_edges=None, rows_per_cell=1):
    g, cells = lattice(np.ones(shape, bool), rows_per_cell=rows_per_cell)
    seg = segment(g, labels(cells) if callable(labels) else labels, 13, made_at)
    adj = seg.adjacency(connectivity, 26 * cells.shape[0] if max_edges is None else max_edges)
    assert not adj.overflowed()
    return g, seg, adj


# ------------------------------------------------------------------------------------------------ 1: cases known by hand
def test_the_hand_cases():
    _, seg, adj = field((2, 1, 1), [0, 1], 6, 6)
    got, _ = check(seg, adj, "two voxels", min_size=2)
    assert got["log_a"].tolist() == [0, -1] and got["log_b"].tolist() == [1, -1] and got["agg_stats"].tolist() == [1, 2, 1, 1, 0, 0, 0, 0]
    lab = {(0, 0): 0, (1, 0): 2, (2, 0): 2, (0, 1): 1, (1, 1): 1, (2, 1): 1}
    _, seg, adj = field((3, 2, 1), lambda cells: np.array([lab[(x, y)] for x, y, _ in cells]), 6, 6)
    got, _ = check(seg, adj, "two rounds", min_size=100, min_contacts=2)
    assert got["log_a"][:2].tolist() == [1, 0] and got["log_round"][:2].tolist() == [0, 1] and got["agg_stats"].tolist() == [1, 3, 2, 2, 1, 0, 0, 0]
    got, _ = check(seg, adj, "two rounds, cut at one", converges=False, min_size=100, min_contacts=2, max_rounds=1)
    assert got["agg_stats"].tolist() == [2, 3, 1, 1, 2, 2, 0, 2] and got["offset"][:2].tolist() == [[1, 1, 0], [-1, -1, 0]]
    occ = np.zeros((2, 2, 2), bool)
    occ[0, 0, 0] = occ[1, 0, 0] = occ[1, 1, 1] = True
    g, _ = lattice(occ)
    seg = segment(g, [0, 1, 0], 2, 6)
    got, _ = check(seg, seg.adjacency(26), "same_label across a corner", min_size=2, same_label=True)
    assert got["log_a"][:2].tolist() == [0, -1] and got["log_b"][0] == 2 and got["agg_stats"].tolist() == [2, 3, 1, 1, 1, 0, 0, 2]
    got, _ = check(seg, seg.adjacency(6), "same_label at the segments' connectivity", min_size=2, same_label=True)
    assert got["agg_stats"].tolist() == [3, 3, 0, 0, 3, 0, 0, 2]


# --------------------------------------------------------------------------------------------------- 2: (a) - (e)
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_random_classes_with_a_tight_table_and_the_default(connectivity):
    g, seg, adj = field((12, 12, 12), ar.random_classes, 6, connectivity)
    E = adj.num_edges()
    tight = seg.adjacency(connectivity, E)                                      # max_edges exactly E: 2 E + 64 slots
    assert tight.num_edges() == E and tight.shape == (1728, E)
    # (at 6 nearly every contact count is 1: a larger min_contacts leaves the fixed point beyond the default rounds)
    for kw in (dict(min_size=8), dict(min_size=16, min_contacts=1 if connectivity == 6 else 2), dict(min_size=2),
               dict(min_size=5, weight="rows")):
        a, _ = check(seg, tight, "tight %s" % kw, **kw)
        b, _ = check(seg, adj, "roomy %s" % kw, devices=False, **kw)
        for k in ar.ALL_KEYS:
            if k not in GRAPH[1:]:                       # the edge arrays differ in their rows of filler alone
                assert np.array_equal(a[k], b[k]), k
    dflt = seg.adjacency(connectivity)                                          # 2 M rows: where they do not fit, H1
    fits = not dflt.overflowed()
    got, _ = check(seg, dflt, "default max_edges", converges=fits, devices=fits, min_size=8)
    assert got["agg_stats"][6] == (0 if fits else 1)
    got, _ = check(seg, tight, "nothing small", min_size=1)                     # H10
    same({k: got[k] for k in GRAPH}, host(tight, GRAPH), "nothing small: the input graph")
    same({k: got[k] for k in SEG}, host(seg, SEG), "nothing small: the input segmentation")


def test_a_field_past_the_scan_tile_and_the_sort_tile():
    g, seg, adj = field((16, 16, 16), ar.random_classes, 6, 6)
    assert seg.num_segments() > 2048 and adj.num_edges() > 8192
    got, _ = check(seg, adj, "16^3", min_size=8)
    assert got["agg_stats"][2] >= 2
    check(seg, adj.trim(), "16^3, rows", min_size=12, weight="rows")


def test_a_chain_across_every_tile():
    g, seg, adj = field((4096, 1, 1), lambda cells: cells[:, 0] % 2, 6, 6)
    assert seg.num_segments() == 4096 and adj.num_edges() == 8190
    got, _ = check(seg, adj, "alternating line", min_size=4096)
    assert got["agg_stats"].tolist() == [1, 4096, 1, 4095, 0, 0, 0, 0] and got["stats"].tolist() == [1, 4096, 0, 0, 4096, 4096, 0, 0]
    # 0 and 1 are mutual, logged by 0; every other piece goes to its left neighbour, the lowest number on a tie
    assert np.array_equal(got["log_a"][:4095], np.r_[0, np.arange(2, 4096)]) and got["log_a"][4095] == -1 and not got["segment"].any()
    assert np.array_equal(got["log_b"][:4095], np.r_[1, np.arange(1, 4095)])
    got, _ = check(seg, adj, "alternating line, pairs", min_size=2)
    assert got["agg_stats"][:4].tolist() == [1, 4096, 1, 4095]                   # every piece is small at the start: one chain again


def test_one_segment_with_a_thousand_small_neighbours():
    def specks(cells):
        odd = (cells[:, 0] % 2 == 1) & (cells[:, 1] % 2 == 1) & (cells[:, 2] != 1)
        return np.where(odd, 1 + (cells[:, 0] // 2 + cells[:, 1] // 2) % 2, 0)
    g, seg, adj = field((48, 48, 3), specks, 6, 26)
    assert seg.num_segments() == 1153 and int(adj.stats[4]) == 1152             # the slab's degree
    got, _ = check(seg, adj, "specks", min_size=8)
    assert got["agg_stats"].tolist() == [1, 1153, 1, 1152, 0, 0, 0, 0] and (got["log_b"][:1152] == 0).all() and not got["voxel_label"].any()
    got, _ = check(seg, adj, "specks, same label", min_size=8, same_label=True)
    assert got["agg_stats"].tolist() == [1153, 1153, 0, 0, 1152, 0, 0, adj.num_edges()]


def noisy_slabs(cells):
    return ar.redrawn_slabs(cells, share=0.15)


def test_the_cut_of_the_rounds():
    g, seg, adj = field((24, 24, 6), noisy_slabs, 6, 6)
    kw = dict(min_size=8, min_contacts=3)
    full, res = check(seg, adj, "8 rounds", max_rounds=8, **kw)
    assert full["agg_stats"][2] == 3                                            # three rounds merge, the fourth finds nothing
    import torch
    for k in (1, 2):
        got, cut = check(seg, adj, "%d round(s)" % k, converges=False, max_rounds=k, **kw)
        want = host(seg.merge(res.log_a, res.log_b, (res.log_round >= 0) & (res.log_round < k)), MERGED)      # H10
        same({x: got[x] for x in MERGED}, want, "the cut at %d" % k)
        n = int((full["log_round"] >= 0).sum() - (full["log_round"] >= k).sum())
        assert got["agg_stats"][3] == n and all(np.array_equal(got[x][:n], full[x][:n]) for x in ar.LOG_KEYS)
        assert not cut.converged() and torch.equal(cut.log_a[n:], torch.full_like(cut.log_a[n:], -1))
    check(seg, adj, "32 rounds", max_rounds=32, **kw)


# ------------------------------------------------------------------------------------------- 3: (f), (g): other inputs
def test_a_smooth_and_a_merged_segmentation():
    import torch
    g, cells = lattice(np.ones((14, 13, 6), bool), rows_per_cell=2)
    dev = g.voxel_count.device
    rng = np.random.default_rng(21)
    lab = torch.from_numpy(noisy_slabs(cells)).to(dev)
    feat = torch.from_numpy(rng.integers(0, 2, (cells.shape[0], 1)).astype(np.float32)).to(dev)
    smooth = g.segments(lab, 13, 26, features=feat, max_difference=0.25)
    assert smooth._smooth and smooth.num_segments() > g.segments(lab, 13, 26).num_segments()
    adj = smooth.adjacency(26, 26 * cells.shape[0])
    check(smooth, adj, "smooth", min_size=6)
    got, _ = check(smooth, adj, "smooth, same label", min_size=6, same_label=True)     # patches of one class fold together
    assert got["agg_stats"][3] > 0
    merged = adj.merge(adj.contacts > 6)
    assert merged.num_segments() < smooth.num_segments()
    adj2 = merged.adjacency(18, 26 * cells.shape[0])
    got, res = check(merged, adj2, "merged", min_size=12, weight="rows")
    check(merged, adj2, "merged, same label", min_size=12, same_label=True)
    again = res.segments.adjacency(18, 26 * cells.shape[0])                     # and the result is an input like any other
    check(res.segments, again, "the result, agglomerated again", min_size=40)
    rows = g.project(res.voxel_label).cpu().numpy()
    inv = g.inverse.cpu().numpy()
    assert np.array_equal(rows, np.where(inv >= 0, got["voxel_label"][np.maximum(inv, 0)], -1))


def test_two_rooms_that_overlap_in_space_do_not_merge():
    import torch
    from pointwise_amd import grid
    from tests.test_grid_geometry import _dev
    from tests.test_grid_segments import room_cloud
    dev = _dev()
    both = torch.from_numpy(np.concatenate([room_cloud(3000, 7401), room_cloud(2500, 7402)])).to(dev)
    g = grid.grid_subsample_rooms(both, torch.tensor([0, 3000, 5500], dtype=torch.int32, device=dev), None, voxel=0.1).trim()
    M = g.data.shape[0]
    lab = np.random.default_rng(4).integers(0, 4, M)
    seg = segment(g, lab, 4, 18)
    adj = seg.adjacency(26, 26 * M)
    got, res = check(seg, adj, "two rooms", min_size=8)
    S = seg.num_segments()
    voxel_room = g.voxel_room.cpu().numpy()
    room = voxel_room[seg.root.cpu().numpy()[:S]]                               # of every segment
    assert (room == voxel_room[got["root"][got["seg_map"][:S]]]).all() and got["agg_stats"][0] < S
    P = int(got["agg_stats"][3])
    assert (room[got["log_a"][:P]] == room[got["log_b"][:P]]).all() and len(set(room[got["log_a"][:P]])) == 2


# ----------------------------------------------------------------------- 4: (h) - (k): overflow, trim, reuse, two runs
def test_an_adjacency_that_overflowed_is_the_identity_and_the_flag():
    g, seg, adj = field((12, 12, 12), ar.random_classes, 6, 18)
    E = adj.num_edges()
    over = seg.adjacency(18, E - 1)
    assert over.overflowed()
    got, res = check(seg, over, "overflow", converges=False, devices=False, min_size=8)
    S = seg.num_segments()
    assert got["agg_stats"].tolist() == [S, S, 0, 0, int((seg.size[:S] < 8).sum()), 0, 1, 0] and not res.converged()
    same({k: got[k] for k in SEG}, host(seg, SEG), "overflow: the identity")
    assert (got["src"] == -1).all() and not got["start"].any() and (got["log_a"] == -1).all()
    assert res.trim().src.shape == (0,) and res.trim().log_a.shape == (0,)


def test_untrimmed_objects_and_trims():
    g, cells = lattice(np.ones((10, 9, 8), bool), rows_per_cell=2, trim=False)  # M = 2 V rows, V of them filler
    V = cells.shape[0] // 2
    lab = np.random.default_rng(8).integers(-1, 5, 2 * V)                       # -1: in no segment
    seg = segment(g, lab, 5, 6)
    adj = seg.adjacency(18, 52 * V)
    assert adj.shape == (2 * V, 52 * V) and 0 < adj.num_edges() < 52 * V
    a, _ = check(seg, adj, "untrimmed", min_size=8)
    assert (a["voxel_label"][lab[:2 * V] < 0] == -1).all() and (a["voxel_label"][V:] == -1).all()
    b, _ = check(seg, adj.trim(), "adj.trim()", min_size=8)
    for k in ar.ALL_KEYS:
        if k not in GRAPH[1:]:
            assert np.array_equal(a[k], b[k]), k
    E2 = int(a["agg_stats"][7])
    assert all(np.array_equal(a[k][:E2], b[k][:E2]) for k in GRAPH[1:])


def test_out_reuse_two_runs_and_a_side_stream():
    import torch
    g, seg, adj = field((12, 12, 12), ar.random_classes, 6, 26)
    dev = seg.segment.device
    first, res = check(seg, adj, "first", min_size=8, min_contacts=2)
    other = segment(g, np.random.default_rng(9).integers(0, 3, 1728), 13, 6)    # other data, the same shapes
    adj_o = other.adjacency(26, adj.shape[1])
    _, res_o = check(other, adj_o, "other data", devices=False, res=adj_o.agglomerate(3, out=res), min_size=3)
    assert res_o is res
    back = adj.agglomerate(8, min_contacts=2, out=res)
    assert back is res
    same(outputs(back), first, "out= reuse: every word rewritten")
    same(outputs(adj.agglomerate(8, min_contacts=2)), first, "a second run")
    with pytest.raises(ValueError, match="out was made"):
        res.segments.adjacency(26, adj.shape[1]).agglomerate(8, out=res)        # not into the segmentation it reads
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = seg.adjacency(26, adj.shape[1]).agglomerate(8, min_contacts=2)
    side.synchronize()
    same(outputs(third), first, "side stream")


def test_no_voxel_and_one_voxel():
    import torch
    from pointwise_amd import grid
    from tests.test_grid_geometry import _dev
    dev = _dev()
    g = grid.grid_subsample(torch.tensor([[0.3, -1.0, 2.0, 5.0]], device=dev), None, voxel=0.1)
    seg = g.segments()
    got, _ = check(seg, seg.adjacency(), "one voxel", min_size=8)
    assert got["agg_stats"].tolist() == [1, 1, 0, 0, 1, 0, 0, 0] and got["voxel_label"].tolist() == [0]
    check(seg, seg.adjacency(6, 0), "one voxel, no edge rows", min_size=8)
    seg = grid.grid_subsample(torch.full((3, 3), float("nan"), device=dev), None, voxel=0.1).trim().segments()
    res = seg.adjacency().agglomerate(8)                 # no rows at all: nothing is launched
    assert res.start.tolist() == [0] and res.log_a.shape == (0,) and res.num_groups() == 0 and res.converged()
    assert res.segments.merge_stats.tolist() == [0, 0, 0, 0] and res.segments.num_segments() == 0
