"""CPU tests (not gpu) of the ring fallback of the interpolated projection: tests/grid_interp_rings_ref.py (columns by
binary search) against its brute force (the Chebyshev distance to every emitted voxel) on the clouds of
tests/grid_interp_rings_cases.py, the properties of rules 6-9 that need no device, the new argument checks of
GridSubsample.interpolate (raised before the device check: the objects here live on the CPU), and the status list of the
C entries through the library."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_interp_ref as gi
from tests import grid_interp_rings_cases as cases
from tests import grid_interp_rings_ref as rr
from tests import grid_ref as gr
from tests import grid_rooms_ref as grr

F = np.float32
NAMES = ("labels", "scores", "ring", "stats", "ring_stats")


def both(data, sub, scores, k, rings, valid, rooms=False):
    """The reference and the brute force, compared -> the reference's outputs."""
    nv = int(sub["stats"][0])
    extra = dict(voxel_room=sub["voxel_room"], voxel_start=sub["voxel_start"]) if rooms else {}
    args = (data, sub["inverse"], sub["data"], sub["voxel_cell"], nv, scores)
    want = rr.interpolate_rings_ref(*args, k=k, rings=rings, valid_labels=valid, **extra)
    brute = rr.interpolate_rings_brute(*args, k=k, rings=rings, valid_labels=valid, **extra)
    for name, a, b in zip(NAMES, want, brute):
        gi.assert_same(a, b, "rings = %d: %s" % (rings, name))
    lab, sc, ring, stats, ring_stats = want
    N = data.shape[0]
    assert stats.sum() == N and ring_stats[1:].sum() == stats[0] == (lab >= 0).sum() and not ring_stats[rings + 1:].any()
    assert ring_stats[0] == stats[2] + ring_stats[2:].sum() and np.array_equal(ring > 0, lab >= 0) and ring.max() <= rings
    assert np.array_equal(np.bincount(ring[ring > 0], minlength=9)[1:], ring_stats[1:]) and not sc[lab < 0].any()
    return want


def scores_for(nv, C, seed):
    return np.random.default_rng(seed).standard_normal((nv, C)).astype(F)


@pytest.mark.parametrize("gap", range(1, 8))
def test_two_slabs_with_a_gap(gap):
    data = cases.slabs(gap, 10 + gap)
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode="mean")
    nv = int(sub["stats"][0])
    valid = cases.near_is_unvoted(sub["voxel_cell"], nv)
    near = sub["voxel_cell"][sub["inverse"], 0] == 0
    assert near.sum() == 48 and (~near).sum() == 64
    lab, _, ring, stats, ring_stats = both(data, sub, scores_for(nv, 13, gap), 3, gap + 1, valid)
    assert (ring[near] == gap + 1).all() and (ring[~near] == 1).all() and (lab >= 0).all()
    assert ring_stats.tolist() == [48, 64] + [48 if r == gap + 1 else 0 for r in range(2, 9)]
    lab, _, ring, stats, ring_stats = both(data, sub, scores_for(nv, 13, gap), 3, gap, valid)
    assert (lab[near] == -1).all() and (ring[near] == 0).all() and stats.tolist() == [64, 0, 48]
    assert ring_stats.tolist() == [48, 64] + [0] * 7


@pytest.mark.parametrize("mode", ["mean", "center"])
def test_a_lattice_with_holes_keeps_the_rows_of_the_plain_call(mode):
    data = cases.lattice(6, 21)
    data[5, 1] = np.nan
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode=mode)
    nv = int(sub["stats"][0])
    assert nv == 216
    valid = cases.some_voted(nv, 0.2, 22)
    scores = scores_for(nv, 13, 23)
    neigh = gi.neighbors_ref(sub["voxel_cell"], nv)
    plain = gi.interpolate_ref(data, sub["inverse"], sub["data"], neigh, scores, k=3, valid_labels=valid)
    first = None
    for rings in (1, 2, 3, 8):
        lab, sc, ring, stats, ring_stats = both(data, sub, scores, 3, rings, valid)
        if rings == 1:
            first = ring == 1
            for name, a, b in zip(("labels", "scores", "stats"), (lab, sc, stats), plain):
                gi.assert_same(a, b, "rings = 1 is the plain call: " + name)
            assert 0 < first.sum() < data.shape[0] - 1
        gi.assert_same(lab[first], plain[0][first], "rule 6: labels")          # untouched, whatever rings is
        gi.assert_same(sc[first], plain[1][first], "rule 6: scores")
        assert np.array_equal(ring == 1, first) and stats[1] == 1
    assert ring_stats[2] > 0 and stats[2] == 0 and ring_stats[0] == ring_stats[2:].sum()
    ints = (scores * 2.0 ** 30).astype(np.int64)                               # the fixed-point sums
    both(data, sub, ints, 8, 3, valid)


def test_exact_ties_follow_the_voxel_number_and_fewer_candidates_than_k():
    data = cases.centres(5)
    sub = gr.grid_subsample_ref(data, None, voxel=0.25, mode="center")
    nv = int(sub["stats"][0])
    assert nv == 125
    faces = [[0, 2, 2], [4, 2, 2], [2, 0, 2], [2, 4, 2], [2, 2, 0], [2, 2, 4]]  # ring 2 of the middle cell, all at d2 = 1/4
    valid = cases.cells_valid(sub["voxel_cell"], nv, faces)
    scores = scores_for(nv, 13, 31)
    middle = np.nonzero((data[:, :3] == F(0.625)).all(axis=1))[0]
    assert middle.size == 1
    for k in (1, 3, 8):
        lab, sc, ring, stats, _ = both(data, sub, scores, k, 4, valid)
        assert ring[middle[0]] == 2 and (lab >= 0).all()
        voted = np.sort(np.nonzero(valid >= 0)[0])[:k]                          # the lowest voxel numbers win the tie
        want = scores[voted].astype(np.float64).mean(axis=0)
        assert np.abs(sc[middle[0]] - want).max() < 1e-5
    valid = cases.cells_valid(sub["voxel_cell"], nv, faces[:2])
    lab, sc, ring, stats, _ = both(data, sub, scores, 8, 2, valid)
    two = scores[valid >= 0].astype(np.float64).mean(axis=0)                    # two candidates, k = 8
    assert ring[middle[0]] == 2 and np.abs(sc[middle[0]] - two).max() < 1e-5


def test_the_corner_cell_and_lower_bounds_that_land_in_the_next_column():
    data = cases.corner(41)
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode="mean")
    nv = int(sub["stats"][0])
    assert sub["voxel_cell"][:nv].tolist() == [[0, 0, 0], [0, 3, 1], [3, 0, 1]]
    valid = np.array([-1, 1, 1], np.int32)
    lab, _, ring, _, ring_stats = both(data, sub, scores_for(nv, 5, 42), 3, 8, valid)
    own = sub["inverse"] == 0
    assert (ring[own] == 3).all() and (ring[~own] == 1).all() and ring_stats.tolist() == [4, 8, 0, 4, 0, 0, 0, 0, 0]
    lab, _, ring, _, _ = both(data, sub, scores_for(nv, 5, 42), 3, 2, valid)
    assert (lab[own] == -1).all()
    data = cases.sparse(7, 0.1, 43)
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode="mean")
    nv = int(sub["stats"][0])
    for rings in (2, 5, 8):
        both(data, sub, scores_for(nv, 13, 44), 3, rings, cases.some_voted(nv, 0.15, 45))


def test_a_single_voted_voxel_labels_every_row_at_its_chebyshev_distance():
    data = cases.lattice(9, 51, per=1)
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode="mean")
    nv = int(sub["stats"][0])
    valid = cases.cells_valid(sub["voxel_cell"], nv, [[0, 3, 8]])
    scores = scores_for(nv, 13, 52)
    lab, _, ring, stats, _ = both(data, sub, scores, 3, 8, valid)
    u = int(np.nonzero(valid >= 0)[0][0])
    dist = np.abs(sub["voxel_cell"][sub["inverse"]] - sub["voxel_cell"][u]).max(axis=1)
    assert (lab == scores[u].argmax()).all() and np.array_equal(ring, np.maximum(dist, 1)) and dist.max() == 8


def test_rooms_that_overlap_share_nothing():
    a, b = cases.lattice(5, 61), cases.lattice(5, 62)
    data = np.concatenate([a, b])
    start = np.array([0, a.shape[0], data.shape[0]], np.int32)
    sub = grr.grid_subsample_rooms_ref(data, start, None, voxel=cases.VOXEL, mode="mean")
    nv = int(sub["stats"][0])
    vs = sub["voxel_start"]
    assert vs.tolist() == [0, 125, 250] and nv == 250
    valid = np.full(nv, -1, np.int32)
    valid[vs[1]:][cases.some_voted(125, 0.05, 63) >= 0] = 4                     # votes in room 1 only
    scores = scores_for(nv, 13, 64)
    lab, sc, ring, stats, ring_stats = both(data, sub, scores, 3, 8, valid, rooms=True)
    assert (lab[:start[1]] == -1).all() and (ring[:start[1]] == 0).all() and (lab[start[1]:] >= 0).all()
    one = gr.grid_subsample_ref(b, None, voxel=cases.VOXEL, mode="mean")
    alone = both(b, one, scores[vs[1]:], 3, 8, valid[vs[1]:])
    for name, x, y in zip(NAMES[:3], (lab, sc, ring), alone):
        gi.assert_same(x[start[1]:], y, "room 1 alone: " + name)


def test_cut_voxels_and_rows_without_a_voxel_and_no_votes_at_all():
    data, _ = gr.cloud(1500, 6, 71, extent=(1.0, 1.0, 0.6))
    data[[3, 999], [0, 2]] = [np.nan, np.inf]
    sub = gr.grid_subsample_ref(data, None, voxel=cases.VOXEL, mode="mean", max_voxels=200)
    nv = int(sub["stats"][0])
    assert nv == 200 < int(sub["stats"][1])
    valid = cases.some_voted(nv, 0.1, 72)
    lab, _, ring, stats, ring_stats = both(data, sub, scores_for(nv, 13, 73), 3, 8, valid)
    assert stats[1] == (sub["inverse"] < 0).sum() > 500 and (ring[sub["inverse"] < 0] == 0).all() and ring_stats[2:].sum() > 0
    lab, _, ring, stats, ring_stats = both(data, sub, scores_for(nv, 13, 73), 3, 8, np.full(nv, -1, np.int32))
    assert (lab == -1).all() and ring_stats.tolist() == [int(stats[2])] + [0] * 8 and stats[0] == 0
    lab, _, ring, stats, ring_stats = both(data, sub, scores_for(nv, 13, 73), 3, 8, None)          # every voxel voted
    assert ring_stats[0] == 0 and ring_stats[1] == stats[0] == (sub["inverse"] >= 0).sum()
    lab, _, ring, stats, ring_stats = both(data, sub, np.zeros((0, 13), F), 3, 8, None)            # M == 0
    assert (lab == -1).all() and stats.tolist() == [0, 1500, 0] and not ring_stats.any()


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_object(N=10, M=4, K=6, rooms=False):
    g = grid.GridRoomSubsample(N, 2, M, K, False, "cpu") if rooms else grid.GridSubsample(N, M, K, False, "cpu")
    return g, torch.zeros((N, K)), torch.zeros((M, 13))


def test_the_checks_pass_up_to_the_device_check():
    ring = torch.zeros(10, dtype=torch.int32)
    for rooms in (False, True):
        g, data, scores = cpu_object(rooms=rooms)
        for kw in (dict(rings=1), dict(rings=8), dict(rings=2, return_ring=True), dict(return_ring=True, out=(ring.clone(), ring)),
                   dict(rings=3, return_scores=True, return_ring=True, out=(ring.clone(), torch.zeros((10, 13)), ring)),
                   dict(rings=3, out=ring), dict(rings=3, return_scores=True, out=(ring, torch.zeros((10, 13))))):
            with pytest.raises(Conv3pError, match="no CPU path"):
                g.interpolate(data, scores, **kw)


@pytest.mark.parametrize("what,msg", [
    ("rings 0", "rings must be"), ("rings 9", "rings must be"), ("rings float", "rings must be"), ("rings bool", "rings must be"),
    ("rings None", "rings must be"), ("return_ring int", "return_ring must be"), ("return_ring None", "return_ring must be"),
    ("out single", "out must be"), ("out pair of three", "out must be"), ("out three of pair", "out must be"),
    ("out ring dtype", "out ring must be"), ("out ring shape", "out ring must be"), ("out ring strided", "out ring must be"),
    ("out ring in scores' place", "out scores must be"),
    ("cell dtype", "voxel_cell must be"), ("cell shape", "voxel_cell must be"), ("stats dtype", "stats must be"),
    ("room dtype", "voxel_room must be"), ("start dtype", "voxel_start must be"),
])
def test_interpolate_refuses_the_new_arguments_before_any_device_work(what, msg):
    g, data, scores = cpu_object(rooms=what.startswith(("room", "start")))
    lab, ring, sc = torch.zeros(10, dtype=torch.int32), torch.zeros(10, dtype=torch.int32), torch.zeros((10, 13))
    kw = {}
    if what == "rings 0": kw["rings"] = 0
    elif what == "rings 9": kw["rings"] = 9
    elif what == "rings float": kw["rings"] = 2.0
    elif what == "rings bool": kw["rings"] = True
    elif what == "rings None": kw["rings"] = None
    elif what == "return_ring int": kw["return_ring"] = 1
    elif what == "return_ring None": kw["return_ring"] = None
    elif what == "out single": kw.update(return_ring=True, out=lab)
    elif what == "out pair of three": kw.update(return_ring=True, return_scores=True, out=(lab, sc))
    elif what == "out three of pair": kw.update(return_ring=True, out=(lab, sc, ring))
    elif what == "out ring dtype": kw.update(return_ring=True, out=(lab, ring.long()))
    elif what == "out ring shape": kw.update(return_ring=True, out=(lab, torch.zeros(9, dtype=torch.int32)))
    elif what == "out ring strided": kw.update(return_ring=True, out=(lab, torch.zeros(20, dtype=torch.int32)[::2]))
    elif what == "out ring in scores' place": kw.update(return_ring=True, return_scores=True, out=(lab, ring, sc))
    else:
        kw["rings"] = 2
        if what == "cell dtype": g.voxel_cell = g.voxel_cell.long()
        elif what == "cell shape": g.voxel_cell = torch.zeros((3, 3), dtype=torch.int32)
        elif what == "stats dtype": g.stats = g.stats.long()
        elif what == "room dtype": g.voxel_room = g.voxel_room.long()
        elif what == "start dtype": g.voxel_start = g.voxel_start.long()
    with pytest.raises(Conv3pError, match=msg):
        g.interpolate(data, scores, **kw)


def test_the_new_symbols_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ("conv3p_grid_interpolate_rings_workspace_bytes", "conv3p_grid_interpolate_rings_f32", "conv3p_grid_interpolate_rings_i64")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.SYMBOLS[names[1]] == _lib.SYMBOLS[names[2]] and len(_lib.SYMBOLS[names[1]][1]) == 26
    size = _lib.load().conv3p_grid_interpolate_rings_workspace_bytes
    assert size(0) > 0 and size(1000) >= size(0) + 4000 and size(-1) == 0 and size(1 << 31) == 0


def test_the_c_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    names = ["data", "N", "K", "inverse", "voxel_data", "voxel_K", "neigh", "cell", "room", "start", "num_rooms", "grid_stats",
             "scores", "M", "C", "valid", "k", "rings", "labels", "out_scores", "out_ring", "stats", "ring_stats", "workspace",
             "workspace_bytes", "stream"]
    ok_args = [p, 4, 6, p, p, 6, p, p, None, None, 0, p, p, 2, 13, None, 3, 4, p, None, None, p, p, p, 1 << 20, None]

    def call(**ch):
        a = list(ok_args)
        for key, val in ch.items():
            a[names.index(key)] = val
        return a

    need = lib.conv3p_grid_interpolate_rings_workspace_bytes(4)
    for fn in (lib.conv3p_grid_interpolate_rings_f32, lib.conv3p_grid_interpolate_rings_i64):
        for ch in ({"N": -1}, {"M": -1}, {"K": 2}, {"voxel_K": 2}, {"C": 0}, {"C": 129}, {"k": 0}, {"k": 9}, {"rings": 0},
                   {"rings": 9}, {"rings": -1}, {"num_rooms": -1}, {"room": p}, {"start": p}, {"stats": None}, {"ring_stats": None},
                   {"data": None}, {"inverse": None}, {"labels": None}, {"voxel_data": None}, {"neigh": None}, {"scores": None},
                   {"cell": None}, {"grid_stats": None}, {"workspace": None}, {"workspace_bytes": 0},
                   {"workspace_bytes": need - 1}):
            assert fn(*call(**ch)) == _lib.ERR_INVALID_ARGUMENT, ch
        assert fn(*call(N=1 << 31)) == _lib.ERR_UNSUPPORTED and fn(*call(M=1 << 31)) == _lib.ERR_UNSUPPORTED
        assert fn(*call(room=p, start=p, num_rooms=65537)) == _lib.ERR_UNSUPPORTED
        assert fn(*call(rings=9, num_rooms=65537, room=p, start=p)) == _lib.ERR_INVALID_ARGUMENT   # the order of the list
        assert fn(*call(N=1 << 31, workspace_bytes=0)) == _lib.ERR_UNSUPPORTED
