"""GPU tests (-m gpu) of the ring fallback of the interpolated projection, GridSubsample.interpolate(rings=, return_ring=)
on conv3p_grid_interpolate_rings_f32 / _i64: labels, scores, ring, interp_stats and ring_stats bit for bit against
tests/grid_interp_rings_ref.py on the clouds of tests/grid_interp_rings_cases.py -- two slabs with a gap of 1 .. 7 cells;
a lattice with holes over k, the classes, both score types, both subsampling modes and rings 1, 2, 3, 8; exact ties at
ring 2 and fewer candidates than k; the corner cell and lower bounds that land in the next column; a single voted voxel;
no row in the fallback, no vote at all, no voxel at all, cut voxels and NaN rows; many clouds; lists of 0 .. 5 rows and
one longer than a pass of the ring kernel's grid; reproducibility and out=."""
import numpy as np
import pytest

from tests import grid_interp_ref as gi
from tests import grid_interp_rings_cases as cases
from tests import grid_interp_rings_ref as rr

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


def host(g):
    """What the reference reads of a subsampling -> the keyword-free arguments behind data, and the rooms' keywords."""
    rooms = {}
    if getattr(g, "voxel_room", None) is not None:
        rooms = dict(voxel_room=g.voxel_room.cpu().numpy(), voxel_start=g.voxel_start.cpu().numpy())
    return (g.inverse.cpu().numpy(), g.data.cpu().numpy(), g.voxel_cell.cpu().numpy(), int(g.stats[0])), rooms


def on_device(scores, dev, entry="f32"):
    """float32 (M, C) numpy -> a tensor; int64 (M, C) numpy -> a SceneScores holding those sums."""
    import torch
    from pointwise_amd import scene
    if entry == "f32":
        return torch.from_numpy(scores).to(dev)
    s = scene.SceneScores(scores.shape[0], scores.shape[1], dev)
    s.scores.copy_(torch.from_numpy(scores).to(dev))
    return s


def same(got, want, what):
    lab, sc, ring, g = got
    for name, a, b in (("labels", lab, want[0]), ("scores", sc, want[1]), ("ring", ring, want[2]),
                       ("interp_stats", g.interp_stats, want[3]), ("ring_stats", g.ring_stats, want[4])):
        gi.assert_same(a.cpu().numpy(), b, "%s: %s" % (what, name))


def check(g, d, scores, k, rings, valid=None, what="", entry="f32"):
    """interpolate(rings=, return_scores, return_ring) against the reference, every output -> the reference's (labels,
    scores, ring, stats, ring_stats).  valid: int32 (M) numpy; None with int64 scores: the SceneScores' own labels."""
    import torch
    s = on_device(scores, d.device, entry)
    vt = None if valid is None else torch.from_numpy(valid).to(d.device)
    if valid is None and entry == "i64":
        valid = s.labels().cpu().numpy()
    args, rooms = host(g)
    want = rr.interpolate_rings_ref(d.cpu().numpy(), *args, scores, k=k, rings=rings, valid_labels=valid, **rooms)
    lab, sc, ring = g.interpolate(d, s, k=k, valid_labels=vt, return_scores=True, rings=rings, return_ring=True)
    same((lab, sc, ring, g), want, "%s, rings = %d" % (what, rings))
    return want


def scores_for(nv, C, seed, entry="f32"):
    rng = np.random.default_rng(seed)
    if entry == "f32":
        return rng.standard_normal((nv, C)).astype(F)
    return rng.integers(1, 1 << 31, size=(nv, C), dtype=np.int64)


# ----------------------------------------------------------------------------------------------- 1. two slabs with a gap
@pytest.mark.parametrize("gap", range(1, 8))
def test_two_slabs_with_a_gap_are_bridged_at_ring_gap_plus_one_and_not_before(gap):
    import torch
    data = cases.slabs(gap, 10 + gap)
    d, g = subsample(data, voxel=cases.VOXEL, mode=MODES[gap % 2])
    g = g.trim() if gap % 2 else g
    args, _ = host(g)
    nv = args[3]
    valid = cases.near_is_unvoted(args[2], nv)
    near = args[2][args[0], 0] == 0
    M = g.data.shape[0]
    valid = np.concatenate([valid, np.full(M - nv, -1, np.int32)])
    assert near.sum() == 48 and (~near).sum() == 64
    if gap == 3:                                         # the votes of a SceneScores on the far side, its labels the default
        from pointwise_amd import scene
        s = scene.SceneScores(M, 13, d.device)
        far = torch.from_numpy(np.nonzero(valid >= 0)[0].astype(np.int32)).to(d.device)
        s.add(torch.from_numpy(scores_for(far.numel(), 13, 3) * 4).to(d.device), far)
        scores, valid_in, entry = s.scores.cpu().numpy(), None, "i64"
        assert np.array_equal(s.labels().cpu().numpy() >= 0, valid >= 0)
    else:
        scores, valid_in, entry = scores_for(M, 13, gap), valid, "f32"
    lab, _, ring, stats, ring_stats = check(g, d, scores, 3, gap + 1, valid_in, "gap %d" % gap, entry)
    assert (ring[near] == gap + 1).all() and (ring[~near] == 1).all() and (lab >= 0).all()
    assert ring_stats.tolist() == [48, 64] + [48 if r == gap + 1 else 0 for r in range(2, 9)] and stats.tolist() == [112, 0, 0]
    lab, _, ring, stats, ring_stats = check(g, d, scores, 3, gap, valid_in, "gap %d, too few rings" % gap, entry)
    assert (lab[near] == -1).all() and (ring[near] == 0).all() and stats.tolist() == [64, 0, 48]
    assert ring_stats.tolist() == [48, 64] + [0] * 7


# ------------------------------------------------------------------------------------------- 2. a lattice with holes
#          k    C   entry  mode
CONFIGS = ((1, 1, "f32", "mean"), (1, 13, "i64", "center"), (1, 128, "f32", "center"), (3, 1, "i64", "mean"),
           (3, 13, "f32", "mean"), (3, 128, "i64", "center"), (8, 1, "f32", "center"), (8, 13, "i64", "mean"),
           (8, 128, "f32", "mean"), (8, 128, "i64", "center"))


@pytest.mark.parametrize("k,C,entry,mode", CONFIGS)
def test_a_lattice_with_holes_over_k_classes_score_types_modes_and_rings(k, C, entry, mode):
    import torch
    data = cases.lattice(6, 21)
    data[5, 1] = np.nan
    d, g = subsample(data, voxel=cases.VOXEL, mode=mode)
    g = g.trim() if k == 3 else g
    M, nv = g.data.shape[0], int(g.stats[0])
    assert nv == 216
    valid = np.concatenate([cases.some_voted(nv, 0.2, 22), np.full(M - nv, -1, np.int32)])
    scores = scores_for(M, C, 23, entry)
    s, vt = on_device(scores, d.device, entry), torch.from_numpy(valid).to(d.device)
    plain = g.interpolate(d, s, k=k, valid_labels=vt, return_scores=True)       # today's call
    plain_stats = g.interp_stats.clone()
    first = (plain[0] >= 0).cpu().numpy()
    assert 0 < first.sum() < data.shape[0] - 1
    for rings in (1, 2, 3, 8):
        lab, sc, ring, stats, ring_stats = check(g, d, scores, k, rings, valid, "k = %d, C = %d, %s, %s" % (k, C, entry, mode), entry)
        gi.assert_same(lab[first], plain[0].cpu().numpy()[first], "rule 6: labels")     # untouched, whatever rings is
        gi.assert_same(sc[first], plain[1].cpu().numpy()[first], "rule 6: scores")
        assert np.array_equal(ring == 1, first) and stats[1] == 1
        if rings == 1:                                   # the new entry at rings = 1 is the plain call
            gi.assert_same(lab, plain[0].cpu().numpy(), "rings = 1: labels")
            gi.assert_same(sc, plain[1].cpu().numpy(), "rings = 1: scores")
            gi.assert_same(stats, plain_stats.cpu().numpy(), "rings = 1: stats")
            assert ring_stats[1] == stats[0] and ring_stats[0] == stats[2] > 0
    assert ring_stats[2] > 0 and stats[2] == 0
    only = g.interpolate(d, s, k=k, valid_labels=vt, rings=8)                   # labels alone: no score row is written
    gi.assert_same(only.cpu().numpy(), lab, "labels alone")
    gi.assert_same(g.interp_stats.cpu().numpy(), stats, "labels alone: stats")


# --------------------------------------------------------------------------------------------------------- 3. exact ties
def test_exact_ties_at_ring_two_follow_the_voxel_number_and_fewer_candidates_than_k():
    data = cases.centres(5)
    d, g = subsample(data, voxel=0.25, mode="center")
    g = g.trim()
    args, _ = host(g)
    nv = args[3]
    assert nv == 125
    faces = [[0, 2, 2], [4, 2, 2], [2, 0, 2], [2, 4, 2], [2, 2, 0], [2, 2, 4]]  # ring 2 of the middle cell, all at d2 = 1/4
    valid = cases.cells_valid(args[2], nv, faces)
    scores = scores_for(nv, 13, 31)
    middle = int(np.nonzero((data[:, :3] == F(0.625)).all(axis=1))[0][0])
    for k in (1, 3, 8):
        lab, sc, ring, _, _ = check(g, d, scores, k, 4, valid, "ties, k = %d" % k)
        assert ring[middle] == 2 and (lab >= 0).all()
        want = scores[np.nonzero(valid >= 0)[0][:k]].astype(np.float64).mean(axis=0)    # the lowest voxel numbers
        assert np.abs(sc[middle] - want).max() < 1e-5
    valid = cases.cells_valid(args[2], nv, faces[:2])
    lab, sc, ring, _, _ = check(g, d, scores, 8, 2, valid, "two candidates, k = 8")
    assert ring[middle] == 2 and np.abs(sc[middle] - scores[valid >= 0].astype(np.float64).mean(axis=0)).max() < 1e-5


# ----------------------------------------------------------------------------------------------------- 4. the corner cell
def test_the_corner_cell_and_lower_bounds_that_land_in_the_next_column():
    data = cases.corner(41)
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    args, _ = host(g)
    assert args[2][:3].tolist() == [[0, 0, 0], [0, 3, 1], [3, 0, 1]] and args[3] == 3
    M = g.data.shape[0]
    valid = np.concatenate([[-1, 1, 1], np.full(M - 3, -1)]).astype(np.int32)
    own = args[0] == 0
    lab, _, ring, _, ring_stats = check(g, d, scores_for(M, 5, 42), 3, 8, valid, "corner")
    assert (ring[own] == 3).all() and (ring[~own] == 1).all() and ring_stats.tolist() == [4, 8, 0, 4, 0, 0, 0, 0, 0]
    lab, _, ring, _, _ = check(g, d, scores_for(M, 5, 42), 3, 2, valid, "corner")
    assert (lab[own] == -1).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_sparse_lattice_from_the_corner(mode):
    data = cases.sparse(7, 0.1, 43)
    d, g = subsample(data, voxel=cases.VOXEL, mode=mode)
    g = g.trim()
    nv = g.data.shape[0]
    for rings in (2, 5, 8):
        want = check(g, d, scores_for(nv, 13, 44), 3, rings, cases.some_voted(nv, 0.15, 45), "sparse")
    assert (want[4][2:] > 0).sum() >= 3


# ------------------------------------------------------------------------------------------------ 5. a single voted voxel
def test_a_single_voted_voxel_labels_every_row_at_its_chebyshev_distance():
    import torch
    data = cases.lattice(9, 51, per=1)
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    g = g.trim()
    cell, inv = g.voxel_cell.cpu().numpy(), g.inverse.cpu().numpy()
    nv = cell.shape[0]
    assert nv == 729
    valid = cases.cells_valid(cell, nv, [[0, 3, 8]])
    u = int(np.nonzero(valid >= 0)[0][0])
    scores = scores_for(nv, 13, 52)
    lab, ring = g.interpolate(d, torch.from_numpy(scores).to(d.device), k=3, valid_labels=torch.from_numpy(valid).to(d.device),
                              rings=8, return_ring=True)
    dist = np.abs(cell[inv] - cell[u]).max(axis=1)
    assert dist.max() == 8 and (lab.cpu().numpy() == scores[u].argmax()).all()
    assert np.array_equal(ring.cpu().numpy(), np.maximum(dist, 1))
    assert g.interp_stats.tolist() == [729, 0, 0] and g.ring_stats.tolist() == [int((dist > 1).sum())] + np.bincount(
        np.maximum(dist, 1), minlength=9)[1:].tolist()


# ------------------------------------------------------------------------------------- 6. no row enters the fallback, ...
@pytest.mark.parametrize("mode", MODES)
def test_all_voted_none_voted_no_voxels_cut_voxels_and_nan_rows(mode):
    import torch
    from tests import grid_ref as gr
    data, _ = gr.cloud(1500, 6, 71, extent=(1.0, 1.0, 0.6))
    data[[3, 999], [0, 2]] = [np.nan, np.inf]
    d, g = subsample(data, voxel=cases.VOXEL, mode=mode, max_voxels=200)        # untrimmed, the voxels past 200 cut
    inv, nv = g.inverse.cpu().numpy(), int(g.stats[0])
    assert nv == 200 < int(g.stats[1]) and (inv < 0).sum() > 500
    scores = scores_for(200, 13, 73)
    lab, sc, ring, stats, ring_stats = check(g, d, scores, 3, 8, None, "all voted")
    plain = g.interpolate(d, torch.from_numpy(scores).to(d.device), k=3, return_scores=True)
    gi.assert_same(plain[0].cpu().numpy(), lab, "all voted: the plain call's labels")
    gi.assert_same(plain[1].cpu().numpy(), sc, "all voted: the plain call's scores")
    assert ring_stats[0] == 0 and ring_stats[1] == stats[0] == (inv >= 0).sum() and stats[1] == (inv < 0).sum()
    lab, sc, ring, stats, ring_stats = check(g, d, scores, 3, 8, cases.some_voted(200, 0.1, 72), "cut voxels")
    assert (ring[inv < 0] == 0).all() and ring_stats[2:].sum() > 0 and (lab[[3, 999]] == -1).all()
    lab, sc, ring, stats, ring_stats = check(g, d, scores, 3, 8, np.full(200, -1, np.int32), "none voted")
    assert (lab == -1).all() and ring_stats.tolist() == [int(stats[2])] + [0] * 8 and stats[0] == 0 and not sc.any()
    lab, sc, ring, stats, ring_stats = check(g, d, np.zeros((0, 13), F), 3, 8, None, "no voxels")
    assert (lab == -1).all() and stats.tolist() == [0, 1500, 0] and not ring_stats.any()
    check(g, d, scores[:120], 3, 8, cases.some_voted(120, 0.1, 74), "fewer score rows than voxels")


# ------------------------------------------------------------------------------------------------------- 7. many clouds
@pytest.mark.parametrize("mode", MODES)
def test_rooms_that_overlap_share_nothing_trimmed_and_untrimmed(mode):
    import torch
    from pointwise_amd import grid
    dev = _dev()
    a, b = cases.lattice(5, 61), cases.lattice(5, 62)
    data = np.concatenate([a, b])
    start = np.array([0, a.shape[0], data.shape[0]], np.int32)
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample_rooms(d, torch.from_numpy(start).to(dev), None, voxel=cases.VOXEL, mode=mode)
    vs, nv, M = g.voxel_start.cpu().numpy(), int(g.stats[0]), g.data.shape[0]
    assert vs.tolist() == [0, 125, 250] and nv == 250 < M
    valid = np.full(M, -1, np.int32)
    valid[125:250][cases.some_voted(125, 0.05, 63) >= 0] = 4                    # votes in room 1 only
    scores = scores_for(M, 13, 64)
    lab, sc, ring, stats, ring_stats = check(g, d, scores, 3, 8, valid, "rooms")
    assert (lab[:start[1]] == -1).all() and (ring[:start[1]] == 0).all() and (lab[start[1]:] >= 0).all()
    t = g.trim()
    want = check(t, d, scores[:nv], 3, 8, valid[:nv], "rooms, trimmed")
    for x, y in zip(want, (lab, sc, ring, stats, ring_stats)):
        gi.assert_same(x, y, "trimmed and untrimmed")
    db = d[start[1]:].contiguous()                       # room 1 alone: the single call, its voxels shifted by voxel_start
    one = grid.grid_subsample(db, None, voxel=cases.VOXEL, mode=mode).trim()
    l1, s1, r1 = one.interpolate(db, torch.from_numpy(scores[125:250].copy()).to(dev), k=3, rings=8, return_scores=True,
                                 valid_labels=torch.from_numpy(valid[125:250].copy()).to(dev), return_ring=True)
    for name, x, y in (("labels", l1, lab), ("scores", s1, sc), ("ring", r1, ring)):
        gi.assert_same(x.cpu().numpy(), y[start[1]:], "room 1 alone: " + name)


# -------------------------------------------------------------------------------------------- 8. edges of the geometry
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
def test_lists_of_a_few_rows(n):
    data = cases.slabs(1, 80 + n, near_rows=max(n, 1), near_cells=1)
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    g = g.trim()
    args, _ = host(g)
    valid = cases.near_is_unvoted(args[2], args[3]) if n else None              # n = 0: every voxel is voted
    lab, _, ring, stats, ring_stats = check(g, d, scores_for(args[3], 13, 81), 3, 2, valid, "a list of %d" % n)
    assert ring_stats[0] == ring_stats[2] == n and (lab >= 0).all() and data.shape[0] % 64


def test_a_list_longer_than_a_pass_of_the_ring_kernels_grid():
    data = cases.slabs(1, 91, near_rows=20, ny=15, nz=15)
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    g = g.trim()
    args, _ = host(g)
    valid = cases.near_is_unvoted(args[2], args[3])
    lab, _, ring, stats, ring_stats = check(g, d, scores_for(args[3], 13, 92), 3, 3, valid, "a long list")
    assert ring_stats[0] == ring_stats[2] == 4500 > 4096 and (lab >= 0).all() and data.shape[0] % 64


def test_more_rows_than_a_pass_of_the_list_kernels_grid():
    from tests import grid_ref as gr
    N = 262144 + 77                                      # 1024 workgroups of 256 rows, and the row loop behind them
    data, _ = gr.cloud(N, 3, 97, extent=(1.6, 1.2, 0.8))
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    g = g.trim()
    nv = g.data.shape[0]
    assert nv == 16 * 12 * 8
    lab, _, ring, stats, ring_stats = check(g, d, scores_for(nv, 2, 98), 1, 2, cases.some_voted(nv, 0.02, 99), "N = %d" % N)
    assert ring_stats[0] > 4096 and ring_stats[2] > 4096 and stats[2] > 0 and (ring[-77:] > 0).any()


# ----------------------------------------------------------------------------------------------------- 9. reproducibility
def test_two_calls_give_the_same_bits_and_out_is_written_in_place():
    import torch
    data = cases.lattice(6, 21)
    d, g = subsample(data, voxel=cases.VOXEL, mode="mean")
    nv = int(g.stats[0])
    M = g.data.shape[0]
    valid = torch.from_numpy(np.concatenate([cases.some_voted(nv, 0.1, 95), np.full(M - nv, -1, np.int32)])).to(d.device)
    scores = torch.from_numpy(scores_for(M, 13, 96)).to(d.device)
    a = g.interpolate(d, scores, k=3, valid_labels=valid, return_scores=True, rings=8, return_ring=True)
    first, first_rings = g.interp_stats.clone(), g.ring_stats.clone()
    workspace = g._ring_workspace.data_ptr()
    out = (torch.full_like(a[0], 7), torch.full_like(a[1], 7.0), torch.full_like(a[2], 7))
    b = g.interpolate(d, scores, k=3, valid_labels=valid, return_scores=True, rings=8, return_ring=True, out=out)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(b, out)) and g._ring_workspace.data_ptr() == workspace
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
    assert torch.equal(first, g.interp_stats) and torch.equal(first_rings, g.ring_stats) and int(first_rings[2:].sum()) > 0
    lab, ring = g.interpolate(d, scores, k=3, valid_labels=valid, rings=8, return_ring=True, out=(out[0].fill_(7), out[2].fill_(7)))
    assert lab.data_ptr() == out[0].data_ptr() and torch.equal(lab, a[0]) and torch.equal(ring, a[2])
    plain = g.interpolate(d, scores, k=3, valid_labels=valid)                   # the default call still is the plain one
    assert torch.equal((plain >= 0), (a[2] == 1)) and int(g.interp_stats[0]) == int(first_rings[1])
