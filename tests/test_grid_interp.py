"""GPU tests (-m gpu) of the interpolated projection, GridSubsample.neighbors / interpolate on conv3p_grid_neighbors and
conv3p_grid_interpolate_f32 / _i64: every output bit for bit against tests/grid_interp_ref.py, in both subsampling modes
unless a test says otherwise -- the neighbour table on small, full, sparse, cut and flat lattices; the edges of the 4 rows
of a wave, of the 64 rows a workgroup takes a step, of the 32 768 rows the largest grid takes a pass (and of 1024 and 4096
rows) over k, the classes, the channels and both score types; exact
ties in the distance; a row on its representative; fewer candidates than k; invalid voxels; rows without a voxel; int64
sums past 2^24 and 2^40 and a SceneScores as it stands; many clouds; the identity with project; reproducibility."""
import numpy as np
import pytest

from tests import grid_interp_ref as gi
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


def host(g):
    """What the reference reads of a subsampling: its voxels' rows, inverse, cells and the emitted number."""
    return g.data.cpu().numpy(), g.inverse.cpu().numpy(), g.voxel_cell.cpu().numpy(), int(g.stats[0])


def check(g, d, scores, k, valid=None, what="", entry="f32"):
    """interpolate with and without scores against the reference -> the reference's (labels, scores, stats, chosen,
    ties).  scores: float32 (M, C) numpy, or with entry i64 int64 (M, C) numpy put into a SceneScores."""
    import torch
    from pointwise_amd import scene
    dev = d.device
    vd, inv, cell, nv = host(g)
    neigh = g.neighbors().cpu().numpy()
    gi.assert_same(neigh, gi.neighbors_ref(cell, nv, *rooms_of(g)), what + ": neighbours")
    vt = None if valid is None else torch.from_numpy(valid).to(dev)
    if entry == "i64":
        s = scene.SceneScores(scores.shape[0], scores.shape[1], dev)
        s.scores.copy_(torch.from_numpy(scores).to(dev))
        if valid is None:
            valid = s.labels().cpu().numpy()             # the default: voxels nobody voted for are no candidates
    else:
        s = torch.from_numpy(scores).to(dev)
    want = gi.interpolate_ref(d.cpu().numpy(), inv, vd, neigh, scores, k=k, valid_labels=valid, detail=True)
    lab, sc = g.interpolate(d, s, k=k, valid_labels=vt, return_scores=True)
    gi.assert_same(lab.cpu().numpy(), want[0], what + ": labels")
    gi.assert_same(sc.cpu().numpy(), want[1], what + ": scores")
    gi.assert_same(g.interp_stats.cpu().numpy(), want[2], what + ": stats")
    only = g.interpolate(d, s, k=k, valid_labels=vt)
    gi.assert_same(only.cpu().numpy(), want[0], what + ": labels alone")
    gi.assert_same(g.interp_stats.cpu().numpy(), want[2], what + ": stats, labels alone")
    return want


def rooms_of(g):
    if getattr(g, "voxel_room", None) is None:
        return ()
    return g.voxel_room.cpu().numpy(), g.voxel_start.cpu().numpy()


def own_voxel_cloud(N=4500, seed=11):
    """tests/test_grid.py's construction: every row its own voxel of a 20^3 lattice of step 0.1."""
    rng = np.random.default_rng(seed)
    cells = np.concatenate([[0], 1 + rng.permutation(20 * 20 * 20 - 1)[:N - 1]])
    ijk = np.stack([cells // 400, (cells // 20) % 20, cells % 20], axis=1)
    xyz = (ijk + 0.25 + 0.5 * rng.random((N, 3))) * 0.1
    xyz[0] = 0.0
    return np.concatenate([xyz, rng.random((N, 2))], axis=1).astype(F)


# ------------------------------------------------------------------------------------------------- the neighbour table
def table(g):
    vd, inv, cell, nv = host(g)
    neigh = g.neighbors().cpu().numpy()
    assert neigh.shape == (cell.shape[0], 27) and neigh.dtype == np.int32
    gi.assert_same(neigh, gi.neighbors_ref(cell, nv), "neighbours")
    gi.assert_same(neigh, gi.neighbors_brute(cell, nv), "neighbours, brute force")
    assert np.array_equal(neigh[:nv, 13], np.arange(nv)) and (neigh[nv:] == -1).all() and neigh.max() < max(nv, 1)
    return neigh, nv


@pytest.mark.parametrize("mode", MODES)
def test_the_table_of_one_row(mode):
    d, g = subsample(np.array([[0.3, -1.0, 2.0, 5.0]], F), voxel=0.1, mode=mode)
    neigh, nv = table(g)
    assert nv == 1 and neigh[0].tolist() == [-1] * 13 + [0] + [-1] * 13


@pytest.mark.parametrize("mode", MODES)
def test_a_full_block_of_cells(mode):
    rng = np.random.default_rng(21)
    ijk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = np.concatenate([(ijk + 0.1 + 0.8 * rng.random((125, 3))) * 0.2 for _ in range(3)])
    xyz[0] = 0.0
    d, g = subsample(rng.permutation(xyz).astype(F), voxel=0.2, mode=mode)
    neigh, nv = table(g)
    per = (neigh >= 0).sum(axis=1)
    assert nv == 125 and per[62] == 27 and sorted(neigh[62]) == sorted(
        (i * 5 + j) * 5 + l for i in (1, 2, 3) for j in (1, 2, 3) for l in (1, 2, 3))
    assert [per[c] for c in (0, 4, 20, 24, 100, 104, 120, 124)] == [8] * 8 and (per == 8).sum() == 8 and (per == 27).sum() == 27


@pytest.mark.parametrize("mode", MODES)
def test_a_sparse_lattice_and_the_cut_of_max_voxels(mode):
    data = own_voxel_cloud()
    d, g = subsample(data, voxel=0.1, mode=mode)
    neigh, nv = table(g)
    assert nv == 4500 and 2 < (neigh >= 0).sum(axis=1).mean() < 27
    t = g.trim()
    assert t.neighbors().data_ptr() == g.neighbors().data_ptr() and t.neighbors().shape == (4500, 27)   # a view is handed on
    d, cut = subsample(data, voxel=0.1, mode=mode, max_voxels=2250)             # half the voxels are cut
    neigh, nv = table(cut)
    assert nv == 2250 and int(cut.stats[1]) == 4500 and neigh.shape == (2250, 27)
    d, wide = subsample(data, voxel=0.1, mode=mode, max_voxels=6000)            # filler rows behind the emitted ones
    t = wide.trim()                                                             # trimmed before the table exists: its own
    neigh, nv = table(wide)
    assert nv == 4500 and neigh.shape == (6000, 27) and (neigh[4500:] == -1).all()
    assert getattr(t, "_neigh", None) is None
    gi.assert_same(t.neighbors().cpu().numpy(), neigh[:4500], "the trimmed object's table")


@pytest.mark.parametrize("mode", MODES)
def test_a_flat_lattice(mode):
    data, _ = gr.cloud(3000, 4, 31, extent=(2.0, 1.5, 0.05))
    d, g = subsample(data, voxel=0.1, mode=mode)
    neigh, nv = table(g)
    assert int(g.stats[4]) == 1 and (neigh.reshape(-1, 9, 3)[:, :, [0, 2]] == -1).all() and (neigh >= 0).sum(axis=1).max() == 9


# -------------------------------------------------------------------------------------- interpolation against the reference
#          k    C  K  mode      entry
CONFIGS = ((1, 1, 3, "mean", "f32"), (3, 13, 6, "center", "f32"), (8, 128, 6, "mean", "f32"), (3, 13, 3, "mean", "i64"),
           (8, 1, 6, "center", "i64"), (1, 128, 3, "center", "i64"), (3, 128, 6, "mean", "f32"), (8, 13, 6, "center", "f32"))


def some_scores(rng, M, C, entry):
    if entry == "f32":
        return rng.standard_normal((M, C)).astype(F)
    s = rng.integers(0, 1 << 31, size=(M, C), dtype=np.int64)    # sums of a few votes of at most 2^30 each
    s[rng.random(M) < 0.1] = 0                                    # voxels nobody voted for
    return s


@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 32767, 32768, 32833])
def test_the_edges_of_the_row_step_over_k_classes_channels_and_score_types(N):
    for n, (k, C, K, mode, entry) in enumerate(CONFIGS):
        if N > 10000 and n not in (1, 3):                # past one pass of the grid: the row loop, one config a score type
            continue
        rng = np.random.default_rng(1000 * N + n)
        data, _ = gr.cloud(N, K, 100 + N + n, extent=(1.0, 0.8, 0.5), origin=(-2.0, 3.0, 0.1))
        d, g = subsample(data, voxel=0.11, mode=mode)
        g = g.trim() if n % 2 else g
        M = g.data.shape[0]
        want = check(g, d, some_scores(rng, M, C, entry), k, what="N = %d, k = %d, C = %d, K = %d, %s, %s" % (N, k, C, K, mode, entry),
                     entry=entry)
        assert want[2][0] + want[2][2] == N and want[2][1] == 0
        if N > 1000 and entry == "f32":
            assert ((want[3] >= 0).sum(axis=1) == k).mean() > 0.9       # k voxels blended nearly everywhere


def test_exact_ties_follow_the_voxel_number():
    """mode center, voxel 0.25, every coordinate a multiple of 1/16, so every d2 is exact: a row at each cell's centre is
    its representative, and rows on the faces and edges between cells lie exactly midway between two or four of them."""
    n = 6
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    centres = (ijk + 0.5) * 0.25
    face = (ijk[ijk[:, 0] < n - 1] + [1.0, 0.5, 0.5]) * 0.25      # midway between the centres of cells i and i + 1
    edge = (ijk[(ijk[:, 0] < n - 1) & (ijk[:, 1] < n - 1)] + [1.0, 1.0, 0.5]) * 0.25   # midway between four
    xyz = np.concatenate([[[0.0, 0.0, 0.0]], centres, face, edge])
    assert np.array_equal(xyz * 16, np.round(xyz * 16))
    rng = np.random.default_rng(41)
    data = np.concatenate([xyz, rng.random((xyz.shape[0], 1))], axis=1)[rng.permutation(xyz.shape[0])].astype(F)
    d, g = subsample(data, voxel=0.25, mode="center")
    vd, inv, cell, nv = host(g)
    assert nv == n ** 3 and np.array_equal(vd[:nv, :3], ((cell[:nv] + 0.5) * 0.25).astype(F))   # the centres represent
    scores = rng.standard_normal((nv, 13)).astype(F)
    for k, least in ((1, 330), (2, 150), (3, 330), (4, 180)):
        want = check(g.trim(), d, scores, k, what="ties, k = %d" % k)
        assert int(want[4].sum()) >= least >= 100, (k, int(want[4].sum()))
    chosen = check(g, d, scores, 1, what="ties, k = 1")[3][:, 0]
    on_face = np.nonzero((data[:, :3] * 4 == np.round(data[:, :3] * 4)).any(axis=1) & (data[:, :3] > 0).all(axis=1))[0]
    assert on_face.size == 330 and (chosen[on_face] < inv[on_face]).all()     # the lower voxel, not the row's own


def test_a_row_on_its_representative_takes_the_floor_not_its_voxels_own_scores():
    data, _ = gr.cloud(3000, 6, 51, extent=(0.3, 0.3, 0.3))
    d, g = subsample(data, voxel=0.03, mode="center")
    vd, inv, cell, nv = host(g)
    on = np.nonzero((data[:, :3] == vd[inv][:, :3]).all(axis=1))[0]           # d2 = 0: the representatives themselves
    assert on.size == nv > 500
    scores = np.random.default_rng(52).standard_normal((nv, 13)).astype(F)
    want = check(g.trim(), d, scores, 3, what="d2 = 0")
    differ = (want[1][on].view(np.uint32) != scores[inv[on]].view(np.uint32)).any(axis=1)
    assert differ.sum() > 100                            # neighbours within 0.044 still move the blend: 1e10 + w > 1e10


@pytest.mark.parametrize("mode", MODES)
def test_fewer_candidates_than_k(mode):
    rng = np.random.default_rng(61)
    a = rng.random((40, 3)) * 0.09
    b = rng.random((30, 3)) * 0.09 + [0.5, 0.0, 0.3]     # an isolated voxel, and a pair of neighbours far from it
    c = rng.random((50, 3)) * [0.19, 0.09, 0.09] + [0.0, 0.7, 0.0]
    data = np.concatenate([[[0.0, 0.0, 0.0]], a, b, c]).astype(F)
    d, g = subsample(data, voxel=0.1, mode=mode)
    want = check(g.trim(), d, rng.standard_normal((int(g.stats[0]), 13)).astype(F), 8, what="k = 8")
    per = (want[3] >= 0).sum(axis=1)
    assert int(g.stats[0]) == 4 and set(per.tolist()) == {1, 2} and (per[:71] == 1).all() and want[2].tolist() == [121, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_invalid_voxels_are_no_candidates(mode):
    data, _ = gr.cloud(2000, 6, 71, extent=(3.0, 3.0, 3.0))
    data[5, 0], data[77, 2] = np.nan, np.inf
    d, g = subsample(data, voxel=0.1, mode=mode)
    vd, inv, cell, nv = host(g)
    valid = np.where(np.arange(nv) % 3 == 0, -1, 4).astype(np.int32)          # a third of the voxels
    want = check(g.trim(), d, np.random.default_rng(72).standard_normal((nv, 13)).astype(F), 3, valid=valid, what="valid_labels")
    lab, stats, chosen = want[0], want[2], want[3]
    assert stats.tolist() == [int((lab >= 0).sum()), 2, int((lab < 0).sum()) - 2] and (stats > 0).all()
    assert (valid[chosen[chosen >= 0]] >= 0).all()
    bad = np.nonzero((inv >= 0) & (valid[np.maximum(inv, 0)] < 0))[0]         # rows of an invalid voxel ...
    neigh = g.neighbors().cpu().numpy()
    others = ((neigh[inv[bad]] >= 0) & (valid[np.maximum(neigh[inv[bad]], 0)] >= 0)).any(axis=1)
    assert others.any() and not others.all()
    assert (lab[bad[others]] >= 0).all() and (lab[bad[~others]] == -1).all()  # ... labelled from neighbours where one exists


@pytest.mark.parametrize("mode", MODES)
def test_rows_without_a_voxel(mode):
    data, _ = gr.cloud(3000, 6, 81, extent=(1.0, 1.0, 0.6))
    data[[3, 999, 2000], [0, 1, 2]] = [np.nan, -np.inf, np.inf]
    d, g = subsample(data, voxel=0.1, mode=mode, max_voxels=300)              # untrimmed, the voxels past 300 cut
    vd, inv, cell, nv = host(g)
    assert nv == 300 < int(g.stats[1]) and (inv < 0).sum() > 1000
    scores = np.random.default_rng(82).standard_normal((300, 13)).astype(F)
    want = check(g, d, scores, 3, what="inverse = -1")
    assert want[2][1] == (inv < 0).sum() and (want[0][inv < 0] == -1).all() and not want[1][inv < 0].any()
    assert (want[0][[3, 999, 2000]] == -1).all()
    want = check(g, d, scores[:200], 3, what="fewer score rows than voxels")   # voxels 200.. are neither own nor candidate
    assert want[2][1] == ((inv < 0) | (inv >= 200)).sum() and want[3].max() < 200


@pytest.mark.parametrize("mode", MODES)
def test_int64_sums_past_2_24_and_2_40(mode):
    rng = np.random.default_rng(91)
    data, _ = gr.cloud(2500, 6, 92, extent=(1.0, 0.8, 0.5))
    d, g = subsample(data, voxel=0.11, mode=mode)
    nv = int(g.stats[0])
    s = rng.integers(1 << 24, 1 << 26, size=(nv, 13), dtype=np.int64) | 1     # odd: float32 must round them
    s[::2] = rng.integers(1 << 40, 1 << 45, size=s[::2].shape, dtype=np.int64) | 1
    s[5::50] = (np.int64(1) << 40) + (np.int64(1) << 16)                       # exactly halfway: to even
    s[7::50] = (np.int64(1) << 40) + 3 * (np.int64(1) << 16)
    assert (s.astype(F).astype(np.int64) != s).mean() > 0.9
    check(g.trim(), d, s, 3, what="int64 sums", entry="i64")


def test_a_scenescores_filled_by_two_calls_goes_in_as_it_stands():
    import torch
    from pointwise_amd import scene
    dev = _dev()
    rng = np.random.default_rng(95)
    data, _ = gr.cloud(2500, 6, 96, extent=(1.0, 0.8, 0.5))
    d, g = subsample(data, voxel=0.11, mode="mean")
    g = g.trim()
    vd, inv, cell, nv = host(g)
    s = scene.SceneScores(nv, 13, dev)
    for part in range(2):                                # overlapping votes; a tenth of the voxels is never voted for
        index = rng.integers(0, nv, size=(6, 256)).astype(np.int32)
        index[index % 10 == 3] = -1
        s.add(torch.from_numpy(rng.standard_normal((6, 256, 13)).astype(F) * 3).to(dev), torch.from_numpy(index).to(dev))
    valid = s.labels().cpu().numpy()
    assert 0 < (valid < 0).sum() < nv // 4 and int(s.scores.max()) > 1 << 30
    want = gi.interpolate_ref(data, inv, vd, g.neighbors().cpu().numpy(), s.scores.cpu().numpy(), k=3, valid_labels=valid)
    lab, sc = g.interpolate(d, s, k=3, return_scores=True)
    gi.assert_same(lab.cpu().numpy(), want[0], "SceneScores: labels")
    gi.assert_same(sc.cpu().numpy(), want[1], "SceneScores: scores")
    gi.assert_same(g.interp_stats.cpu().numpy(), want[2], "SceneScores: stats")
    proj = g.project(s.labels()).cpu().numpy()
    assert ((proj >= 0) <= (want[0] >= 0)).all() and (want[0] >= 0).sum() > (proj >= 0).sum()


# ------------------------------------------------------------------------------------------------------------ many clouds
SIZES = (3000, 2800, 40, 3100)


def raw_rooms():
    from pointwise_amd import synth
    rng = np.random.default_rng(4200)
    parts = []
    for k, n in enumerate(SIZES):                        # the rooms overlap in space: each starts at its own origin
        xyz = synth.room_like(1, n, 4201 + k, (3.2 - 0.4 * k, 2.4 + 0.3 * k, 3.0))[0]
        parts.append(np.concatenate([xyz, rng.random((n, 3))], axis=1).astype(F))
    parts[2][:, 0] = np.nan                              # a room of non-finite rows only: it has no voxels
    data = np.concatenate(parts)
    data[17, 0], data[2500, 2], data[8899 - 3100 + 3140, 0] = np.nan, np.inf, np.nan
    return data, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)


@pytest.mark.parametrize("mode", MODES)
def test_many_clouds_share_nothing_and_equal_their_single_calls(mode):
    import torch
    from pointwise_amd import grid
    dev = _dev()
    data, start = raw_rooms()
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample_rooms(d, torch.from_numpy(start).to(dev), None, voxel=0.08, mode=mode)
    vd, inv, cell, nv = host(g)
    room, vstart = rooms_of(g)
    assert vstart[2] == vstart[3] and nv == vstart[4] > 1500 and g.data.shape[0] == data.shape[0]   # untrimmed
    neigh = g.neighbors().cpu().numpy()
    gi.assert_same(neigh, gi.neighbors_brute(cell, nv, room), "rooms: neighbours, brute force")
    hit = neigh >= 0
    assert np.array_equal(room[neigh[hit]], np.broadcast_to(room[:, None], neigh.shape)[hit])       # no entry crosses a room
    scores = np.random.default_rng(4300).standard_normal((nv, 13)).astype(F)
    want = check(g, d, scores, 3, what="rooms")
    room_of_row = np.repeat(np.arange(len(SIZES)), SIZES)
    chosen = want[3]
    assert np.array_equal(room[chosen[chosen >= 0]], np.broadcast_to(room_of_row[:, None], chosen.shape)[chosen >= 0])
    assert (want[0][start[2]:start[3]] == -1).all() and want[2][1] == 40 + 3
    lab, sc = g.interpolate(d, torch.from_numpy(scores).to(dev), k=3, return_scores=True)
    lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
    for r in range(len(SIZES)):                          # each room's slice is the single call on the room, voxels shifted
        a, b, va, vb = int(start[r]), int(start[r + 1]), int(vstart[r]), int(vstart[r + 1])
        dr = d[a:b].contiguous()
        one = grid.grid_subsample(dr, None, voxel=0.08, mode=mode)
        assert int(one.stats[0]) == vb - va
        n1 = one.neighbors().cpu().numpy()[:vb - va]
        gi.assert_same(neigh[va:vb], np.where(n1 >= 0, n1 + va, -1).astype(np.int32), "room %d: neighbours" % r)
        l1, s1 = one.interpolate(dr, torch.from_numpy(scores[va:vb].copy()).to(dev), k=3, return_scores=True)
        gi.assert_same(lab[a:b], l1.cpu().numpy(), "room %d: labels" % r)
        gi.assert_same(sc[a:b], s1.cpu().numpy(), "room %d: scores" % r)
    t = g.trim()                                         # the trimmed many-clouds object takes a view of the table
    assert t.neighbors().data_ptr() == g.neighbors().data_ptr() and t.neighbors().shape == (nv, 27)
    gi.assert_same(t.interpolate(d, torch.from_numpy(scores).to(dev), k=3).cpu().numpy(), lab, "rooms, trimmed")


# ------------------------------------------------------------------------------------------- identity and reproducibility
@pytest.mark.parametrize("mode", MODES)
def test_one_neighbour_of_rows_that_are_their_own_voxels_is_the_projection(mode):
    import torch
    data = own_voxel_cloud()
    d, g = subsample(data, voxel=0.1, mode=mode)
    scores = torch.from_numpy(np.random.default_rng(111).standard_normal((4500, 13)).astype(F)).to(d.device)
    got = g.interpolate(d, scores, k=1)
    assert torch.equal(got, g.project(scores.argmax(dim=1).to(torch.int32))) and int(g.interp_stats[0]) == 4500


def test_two_calls_and_a_side_stream_are_bitwise_equal():
    import torch
    data, _ = gr.cloud(4097, 6, 121, extent=(1.0, 0.8, 0.5))
    data[11, 1] = np.nan
    d, g = subsample(data, voxel=0.11, mode="mean")
    scores = torch.from_numpy(np.random.default_rng(122).standard_normal((int(g.stats[0]), 13)).astype(F)).to(d.device)
    a = g.interpolate(d, scores, k=3, return_scores=True)
    first = g.interp_stats.clone()
    b = g.interpolate(d, scores, k=3, return_scores=True, out=(torch.full_like(a[0], 7), torch.full_like(a[1], 7.0)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(first, g.interp_stats) and first.tolist() == [4096, 1, 0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _, g2 = subsample(data, voxel=0.11, mode="mean")
        c = g2.interpolate(d, scores, k=3, return_scores=True)             # the table too is built on the side stream
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
    assert torch.equal(g.neighbors(), g2.neighbors()) and torch.equal(first, g2.interp_stats)
