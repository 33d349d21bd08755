"""GPU tests (-m gpu) of GridSubsample.segments(normals= / features=) on conv3p_grid_segments_smooth and of
GridSegments.pool on conv3p_grid_segment_pool_f32 / _i64: every output and both stats bit for bit against
tests/grid_smooth_ref.py, which is fed the device's own neighbour table and, for the pool, the device's own segments.

Smooth segments: the floor and wall of tests/test_grid_smooth_host.py; a dense 17 x 16 x 8 lattice (three tiles of the
union-find in LDS, past one tile of the numbering's scan) with normals striped along the slowest axis (refused pairs
cross tiles), along the fastest (refused pairs inside a tile) and identical everywhere (equal to segments() word for
word); flags and non-finite normals; a dot product one ulp below the threshold; signed normals; curvature; features with
F = 1 and 16, a column slice, a NaN and a difference equal to the bound; labels with normals; L < ne, filler rows, one
voxel, no voxel; two rooms that overlap; a snake cut into known pieces; two calls and a side stream.  Pool: C = 1, 13,
128; one segment of 4160 voxels and three of 65 536 (runs carried across steps and chunks); singleton segments; rows as
weights; L < ne; NaN and large rows; a real SceneScores; the bits of the mean past 2^53; ties, zero rows, S = 0, merge()."""
import numpy as np
import pytest

from tests import grid_smooth_ref as sm

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ("segment", "root", "size", "rows", "label", "stats", "smooth_stats")
POOL = ("sums", "weights", "mean", "label", "voxel_label", "stats")
UP, SIDE, FRONT = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


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


def host(obj, names):
    return {k: (getattr(obj, k).cpu().numpy() if getattr(obj, k) is not None else None) for k in names}


def same(got, want, what):
    for k in want:
        if want[k] is None:
            assert got[k] is None, "%s: %s" % (what, k)
            continue
        a, b = got[k], want[k]
        if a.dtype == np.float64:                        # the bits, so that -0.0 and 0.0 differ
            a, b = a.view(np.int64), b.view(np.int64)
        assert got[k].dtype == want[k].dtype and np.array_equal(a, b), "%s: %s" % (what, k)


def dev_normals(g, normals, flags=None, curvature=None):
    """numpy normals (M, 3) -> a bare tensor, or with flags / curvature a GridNormals that holds them."""
    import torch
    from pointwise_amd import grid
    dev = g.voxel_count.device
    t = torch.from_numpy(np.ascontiguousarray(normals, dtype=F)).to(dev)
    if flags is None and curvature is None:
        return t
    M = t.shape[0]
    n = grid.GridNormals(M, False, dev)
    n.normals.copy_(t)
    n.flags.copy_(torch.from_numpy(np.zeros(M, np.int32) if flags is None else flags).to(dev))
    n.curvature.copy_(torch.from_numpy(np.zeros(M, F) if curvature is None else curvature).to(dev))
    return n


def check(g, what, labels=None, num_class=None, connectivity=26, normals=None, flags=None, curvature=None, max_angle=None,
          signed=False, max_curvature=None, features=None, max_difference=None, embed=None):
    """segments(...) with the smooth keywords against the reference -> (the device object, its outputs on the host).  embed
    (width, first column): the features go in as a column slice of a wider tensor."""
    import torch
    dev = g.voxel_count.device
    lab_t = torch.from_numpy(labels).to(dev) if labels is not None else None
    kw = {}
    if normals is not None:
        kw.update(normals=dev_normals(g, normals, flags, curvature if max_curvature is not None else None), max_angle=max_angle,
                  signed=signed, max_curvature=max_curvature)
    if features is not None:
        f = torch.from_numpy(np.ascontiguousarray(features, dtype=F)).to(dev)
        if embed is not None:
            wide = torch.full((f.shape[0], embed[0]), 1e9, dtype=torch.float32, device=dev)
            wide[:, embed[1]:embed[1] + f.shape[1]] = f
            f = wide[:, embed[1]:embed[1] + f.shape[1]]
            assert not f.is_contiguous() or f.shape[0] <= 1
        kw.update(features=f, max_difference=max_difference)
    seg = g.segments(lab_t, num_class, connectivity, **kw)
    neigh, count, ne = g.neighbors().cpu().numpy(), g.voxel_count.cpu().numpy(), int(g.stats[0])
    rule = {}
    if normals is not None:
        rule.update(normals=normals, flags=flags, min_cos=sm.min_cos_of(max_angle), signed=signed)
        if max_curvature is not None:
            rule.update(curvature=curvature, max_curvature=max_curvature)
    if features is not None:
        rule.update(features=features, max_difference=max_difference)
    want = sm.smooth_segments_ref(neigh, labels, labels.shape[0] if labels is not None else 0, count, ne, num_class, connectivity,
                                  **rule)
    got = host(seg, OUTPUTS)
    same(got, want, what)
    st = got["smooth_stats"]
    assert st[0] == st[1:6].sum() and st[7] == 0, what
    return seg, got


def check_pool(g, seg, values, what, weight="voxels", return_mean=True, embed=None):
    """seg.pool(values) against the reference on the device's own segments -> the reference's dict."""
    import torch
    dev = g.voxel_count.device
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    if embed is not None:
        wide = torch.zeros((v.shape[0], embed[0]), dtype=v.dtype, device=dev)
        wide[:, embed[1]:embed[1] + v.shape[1]] = v
        v = wide[:, embed[1]:embed[1] + v.shape[1]]
    pool = seg.pool(v, weight=weight, return_mean=return_mean)
    want = sm.pool_ref(values, seg.segment.cpu().numpy(), int(seg.stats[0]), g.voxel_count.cpu().numpy(), int(g.stats[0]),
                       {"voxels": 0, "rows": 1}[weight], return_mean)
    same(host(pool, POOL), want, what)
    S = seg.num_segments()
    assert pool.num_segments() == S and pool.trim().sums.shape == (S, values.shape[1]), what
    assert np.array_equal(want["voxel_label"], np.where(seg.segment.cpu().numpy() >= 0, want["label"][seg.segment.cpu().numpy()], -1))
    return want


# ------------------------------------------------------------------------------------------------ smooth: hand cases
@pytest.mark.parametrize("connectivity,at30,at45", [(6, (101, 93), (101, 101)), (26, (195, 165), (195, 185))])
def test_a_floor_and_a_wall_that_meet_in_a_crease(connectivity, at30, at45):
    occ, nrm = sm.hand_case()
    g, cells = lattice(occ)
    first_floor = int(np.nonzero(cells[:, 0] > 0)[0][0])
    _, got = check(g, "30 degrees", connectivity=connectivity, normals=nrm, max_angle=30)
    assert got["stats"][0] == 3 and got["size"][:3].tolist() == [4, 28, 28] and got["segment"][:3].tolist() == [0, 1, 1]
    assert got["segment"][first_floor] == 2 and tuple(got["smooth_stats"][:2]) == at30
    seg, got = check(g, "45 degrees: equality joins", connectivity=connectivity, normals=nrm, max_angle=45)
    assert got["stats"][0] == 1 and got["size"][0] == 60 and tuple(got["smooth_stats"][:2]) == at45
    assert seg.trim().smooth_stats is seg.smooth_stats
    with pytest.raises(ValueError, match="smooth segmentation"):
        seg.absorb(2)
    plain = g.segments(connectivity=connectivity, out=seg)                       # the same object, plain again
    assert plain.smooth_stats is None and plain.absorb(2).shape == (60,)


def test_a_dot_product_one_ulp_below_the_threshold_is_not_joined():
    # min_cos of 60 degrees is float32(0.5000000000000001) = 0.5; (1, 0, 0) . (d, 0, 0) = d exactly
    g, _ = lattice(np.ones((4, 1, 1), bool))
    below = np.nextafter(F(0.5), F(0))
    assert sm.min_cos_of(60) == F(0.5) and below < F(0.5)
    nrm = np.array([SIDE, (0.5, 0, 0), SIDE, (below, 0, 0)], F)
    _, got = check(g, "one ulp", connectivity=6, normals=nrm, max_angle=60)
    assert got["segment"].tolist() == [0, 0, 0, 1] and got["smooth_stats"].tolist() == [3, 2, 0, 1, 0, 0, 0, 0]


def test_signed_normals_flags_curvature_and_labels_on_a_line():
    g, _ = lattice(np.ones((6, 1, 1), bool))
    down = (0.0, 0.0, -1.0)
    nrm = np.array([UP, UP, down, UP, UP, UP], F)
    assert check(g, "unsigned", connectivity=6, normals=nrm, max_angle=60)[1]["stats"][0] == 1
    _, got = check(g, "signed", connectivity=6, normals=nrm, max_angle=60, signed=True)
    assert got["segment"].tolist() == [0, 0, 1, 2, 2, 2]
    nrm = np.array([UP, UP, UP, UP, (np.nan, 0, 1), (np.inf, 0, 0)], F)
    flags = np.array([0, 2, 0, 0, 0, 0], np.int32)
    _, got = check(g, "flags and non-finite normals", connectivity=6, normals=nrm, flags=flags, max_angle=60)
    assert got["segment"].tolist() == [0, 1, 2, 2, 3, 4] and got["smooth_stats"].tolist() == [5, 1, 4, 0, 0, 0, 3, 0]
    curv = np.array([0.1, 0.25, 0.3, 0.1, np.nan, 0.1], F)
    _, got = check(g, "curvature", connectivity=6, normals=np.array([UP] * 6, F), max_angle=60, curvature=curv, max_curvature=0.25)
    assert got["segment"].tolist() == [0, 0, 1, 2, 3, 4] and got["smooth_stats"].tolist() == [5, 1, 0, 0, 4, 0, 0, 0]
    _, got = check(g, "curvature not asked", connectivity=6, normals=np.array([UP] * 6, F), flags=flags * 0, curvature=curv, max_angle=60)
    assert got["stats"][0] == 1
    lab = np.array([0, 0, 1, 1, 1, 7], np.int32)
    _, got = check(g, "labels first", lab, 2, 6, normals=np.array([UP, UP, UP, UP, SIDE, SIDE], F), max_angle=60)
    assert got["segment"].tolist() == [0, 0, 1, 1, 2, -1] and got["smooth_stats"].tolist() == [3, 2, 0, 1, 0, 0, 0, 0]


def test_features_of_one_and_sixteen_channels_slices_a_nan_and_equality():
    g, cells = lattice(np.ones((6, 5, 4), bool))
    M = cells.shape[0]
    rng = np.random.default_rng(21)
    one = (rng.integers(0, 4, (M, 1)) * 0.25).astype(F)                   # differences are multiples of 1/4: 0.25 IS the bound
    seg, got = check(g, "F = 1", features=one, max_difference=0.25)
    assert got["stats"][0] < M and got["smooth_stats"][5] > 0 and got["smooth_stats"][1] > 0
    check(g, "F = 1, a slice", connectivity=6, features=one, max_difference=0.25, embed=(6, 3))
    wide = (rng.integers(0, 3, (M, 16)) * 0.5).astype(F)
    wide[:, :15] = 0
    wide[rng.integers(0, M, 7), rng.integers(0, 15, 7)] = np.nan         # a NaN channel refuses every pair of its voxel
    _, got = check(g, "F = 16", connectivity=18, features=wide, max_difference=0.5)
    assert got["smooth_stats"][5] > 0 and got["smooth_stats"][1] > 0
    check(g, "F = 16, a slice", features=wide, max_difference=0.5, embed=(24, 8))
    rgb = (rng.integers(0, 2, (M, 3)) * 0.5).astype(F)
    nrm = np.where((cells[:, 0:1] // 3) % 2 == 0, F(UP), F(SIDE)).astype(F)
    _, got = check(g, "normals and features", connectivity=6, normals=nrm, max_angle=20, features=rgb, max_difference=0.25, embed=(6, 3))
    assert got["smooth_stats"][3] > 0 and got["smooth_stats"][5] > 0


# ------------------------------------------------------------------------------------- smooth: three tiles, two stripes
@pytest.fixture(scope="module")
def dense():
    return lattice(np.ones((17, 16, 8), bool), rows_per_cell=2)         # 2176 voxels: three local tiles, past one scan tile


def test_normals_striped_across_and_inside_the_tiles(dense):
    g, cells = dense
    assert cells.shape[0] == 2176
    for axis, period, what in ((0, 3, "across tiles"), (2, 2, "inside a tile")):
        nrm = np.where((cells[:, axis:axis + 1] // period) % 2 == 0, F(UP), F(SIDE)).astype(F)
        for c in (6, 26):
            _, got = check(g, "stripes %s at %d" % (what, c), connectivity=c, normals=nrm, max_angle=10)
            assert got["stats"][0] == cells[:, axis].max() // period + 1
            assert np.array_equal(got["segment"], cells[:, axis] // period) and got["smooth_stats"][3] > 0


def test_identical_normals_equal_the_plain_segments_word_for_word(dense):
    import torch
    g, cells = dense
    M = cells.shape[0]
    lab = np.random.default_rng(8).integers(0, 3, M).astype(np.int32)
    nrm = np.tile(F([0.6, 0.0, 0.8]), (M, 1))
    for labels, nc in ((None, None), (lab, 3)):
        for c in (6, 18, 26):
            seg, got = check(g, "identical normals at %d" % c, labels, nc, c, normals=nrm, max_angle=1)
            plain = g.segments(torch.from_numpy(labels).to(g.voxel_count.device) if labels is not None else None, nc, c)
            same(got, host(plain, OUTPUTS[:-1]), "against segments() at %d" % c)
            assert got["smooth_stats"][0] == got["smooth_stats"][1] > 0


def test_three_classes_combined_with_normals(dense):
    g, cells = dense
    lab = ((cells[:, 1] // 5) % 3).astype(np.int32)
    nrm = np.where((cells[:, 0:1] // 4) % 2 == 0, F(UP), F(FRONT)).astype(F)
    curv = (np.random.default_rng(9).random(cells.shape[0]) * 0.3).astype(F)
    seg, got = check(g, "classes and normals", lab, 3, 18, normals=nrm, max_angle=30, curvature=curv, max_curvature=0.27)
    S = got["stats"][0]
    assert S > 15 and np.array_equal(got["label"][got["segment"]], lab) and got["smooth_stats"][4] > 0
    assert (got["rows"][:S] == 2 * got["size"][:S]).all()


# ------------------------------------------------------------------------------------------------- smooth: the edges
def test_filler_rows_short_labels_one_voxel_and_no_voxel():
    import torch
    from pointwise_amd import grid
    occ = np.random.default_rng(5).random((9, 8, 7)) < 0.6
    occ[0, 0, 0] = True
    V = int(occ.sum())
    g, cells = lattice(occ, rows_per_cell=2, trim=False)                  # M = 2 V rows, V of them filler
    M = g.voxel_count.shape[0]
    assert M == 2 * V and int(g.stats[0]) == V
    rng = np.random.default_rng(6)
    nrm = np.zeros((M, 3), F)
    nrm[:, 2] = 1
    nrm[rng.random(M) < 0.3] = SIDE
    feat = (rng.integers(0, 3, (M, 2)) * 0.5).astype(F)
    _, got = check(g, "untrimmed", normals=nrm, max_angle=5)
    assert got["stats"][3] == V and (got["segment"][V:] == -1).all()
    for L in (2 * V, V - 5, 1, 0):
        lab = rng.integers(-1, 4, L).astype(np.int32)
        check(g, "untrimmed, L = %d" % L, lab, 3, 18, normals=nrm, max_angle=5, features=feat, max_difference=0.5)
    dev = _dev()
    one = grid.grid_subsample(torch.tensor([[0.3, -1.0, 2.0, 5.0]], device=dev), None, voxel=0.1)
    _, got = check(one, "one voxel", normals=np.array([UP], F), max_angle=0, features=np.array([[1.0]], F), max_difference=0)
    assert got["segment"].tolist() == [0] and got["smooth_stats"].tolist() == [0] * 8
    none = grid.grid_subsample(torch.full((3, 3), float("nan"), device=dev), None, voxel=0.1)     # nothing emitted
    _, got = check(none, "nothing emitted", normals=np.zeros((3, 3), F), max_angle=10)
    assert got["stats"].tolist() == [0, 0, 0, 3, 0, 0, 0, 0] and not got["smooth_stats"].any()
    t = none.trim()                                       # no rows at all: nothing is launched
    seg = t.segments(normals=torch.zeros((0, 3), device=dev), max_angle=10)
    assert seg.segment.shape == (0,) and seg.num_segments() == 0 and seg.smooth_stats.tolist() == [0] * 8
    pool = seg.pool(torch.zeros((0, 4), device=dev))
    assert pool.sums.shape == (0, 4) and pool.stats.tolist() == [0, 0, 0, 0]


def room_cloud(n=6000, seed=7301):
    from pointwise_amd import synth
    xyz = synth.room_like(1, n, seed, (3.2, 2.4, 3.0))[0]
    return np.concatenate([xyz, np.random.default_rng(seed).random((n, 3))], axis=1).astype(F)


def test_two_rooms_that_overlap_in_space():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    a, b = room_cloud(3000, 7401), room_cloud(2500, 7402)
    both = torch.from_numpy(np.concatenate([a, b])).to(dev)
    start = torch.tensor([0, 3000, 5500], dtype=torch.int32, device=dev)
    g = grid.grid_subsample_rooms(both, start, None, voxel=0.1).trim()
    nrm = g.normals()                                                            # the device's own normals
    n, f, c = nrm.normals.cpu().numpy(), nrm.flags.cpu().numpy(), nrm.curvature.cpu().numpy()
    seg, got = check(g, "two rooms", normals=n, flags=f, curvature=c, max_angle=25, max_curvature=0.2)
    S = got["stats"][0]
    room_of_voxel = g.voxel_room.cpu().numpy()
    assert S > 2 and (room_of_voxel[got["root"][:S]][got["segment"]] == room_of_voxel).all()
    assert (np.diff(room_of_voxel[got["root"][:S]]) >= 0).all() and got["smooth_stats"][6] == (f != 0).sum()
    again = g.segments(normals=nrm, max_angle=25, max_curvature=0.2)            # the GridNormals object itself
    same(host(again, OUTPUTS), got, "the GridNormals object")
    check_pool(g, seg, g.data.cpu().numpy()[:, 3:6], "two rooms: mean colour", weight="rows")


def snake(n=64):
    """tests/test_grid_segments.py's snake: a one-voxel-wide path folded through n x n x 3."""
    occ = np.zeros((n, n, 3), bool)
    occ[0::2, :, 0] = True
    for i in range(1, n - 1, 2):
        occ[i, n - 1 if (i // 2) % 2 == 0 else 0, 0] = True
    occ[:, 0::2, 2] = True
    for j in range(1, n - 1, 2):
        occ[n - 1 if (j // 2) % 2 == 0 else 0, j, 2] = True
    occ[n - 2, n - 1, 1] = occ[n - 2, n - 1, 2] = True
    return occ


@pytest.fixture(scope="module")
def the_snake():
    return lattice(snake())


def test_a_snake_cut_into_known_pieces(the_snake):
    g, cells = the_snake
    M = cells.shape[0]
    assert M == 4160
    # the normal turns wherever i crosses a multiple of 16 in layer 0 and wherever j does in layer 2: the rows of layer 0
    # run along j, so a band of 16 rows i is one piece of the path (8 rows and their turns); the joint is layer 2's.  Three
    # directions in turn: the bands that touch -- k and k + 1 within a layer, and 3 and 7 at the joint -- always differ.
    band = np.where(cells[:, 2] == 0, cells[:, 0] // 16, 4 + cells[:, 1] // 16)
    band[cells[:, 2] == 1] = 7                            # the joining cell goes with layer 2's last band
    nrm = np.array([UP, SIDE, FRONT], F)[band % 3]
    _, got = check(g, "cut snake", connectivity=6, normals=nrm, max_angle=10)
    assert got["stats"][0] == 8
    assert all(len(set(band[got["segment"] == s])) == 1 for s in range(8)) and sorted(got["size"][:8]) == sorted(np.bincount(band))
    _, got = check(g, "whole snake", connectivity=26, normals=np.tile(F(UP), (M, 1)), max_angle=10)
    assert got["stats"][0] == 1 and got["size"][0] == M


def test_two_calls_out_reuse_and_a_side_stream(dense):
    import torch
    g, cells = dense
    dev = g.voxel_count.device
    rng = np.random.default_rng(31)
    nrm = torch.from_numpy(np.where(rng.random((cells.shape[0], 1)) < 0.5, F(UP), F(SIDE)).astype(F)).to(dev)
    feat = torch.from_numpy((rng.integers(0, 2, (cells.shape[0], 3)) * 0.5).astype(F)).to(dev)
    kw = dict(normals=nrm, max_angle=12, features=feat, max_difference=0.25)
    first = g.segments(connectivity=18, **kw)
    a = host(first, OUTPUTS)
    pa = host(first.pool(feat, weight="rows"), POOL)
    other = g.segments(connectivity=18, out=first, normals=nrm, max_angle=180)
    assert other is first and first.num_segments() == 1
    again = g.segments(connectivity=18, out=first, **kw)
    same(host(again, OUTPUTS), a, "out= reuse")
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        third = g.segments(connectivity=18, **kw)
        pool = third.pool(feat, weight="rows")
    side.synchronize()
    same(host(third, OUTPUTS), a, "side stream")
    same(host(pool, POOL), pa, "side stream, pool")
    buf = first.pool(feat[:, :1])
    assert first.pool(feat[:, 1:2], out=buf) is buf


# -------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("C", [1, 13, 128])
def test_pool_over_random_segments(dense, C):
    import torch
    g, cells = dense
    M = cells.shape[0]
    rng = np.random.default_rng(40 + C)
    lab = torch.from_numpy(rng.integers(0, 4, M).astype(np.int32)).to(g.voxel_count.device)
    seg = g.segments(lab, 4, 6)
    values = (rng.random((M, C)) * 2 - 1).astype(F)
    values[rng.integers(0, M, 9), rng.integers(0, C, 9)] = np.nan         # these rows do not contribute
    values[rng.integers(0, M, 9), rng.integers(0, C, 9)] = 256.5
    values[rng.integers(0, M, 9), rng.integers(0, C, 9)] = -np.inf
    values[rng.integers(0, M, 9), rng.integers(0, C, 9)] = -256.0         # this one does
    want = check_pool(g, seg, values, "C = %d" % C)
    assert 0 < want["stats"][1] <= 27 and want["stats"][0] + want["stats"][1] == M
    check_pool(g, seg, values, "C = %d, rows" % C, weight="rows", return_mean=False)
    check_pool(g, seg, values[:M - 700], "C = %d, L < ne" % C)
    if C == 13:
        check_pool(g, seg, values, "a column slice", embed=(20, 4))
        check_pool(g, seg, (np.nan_to_num(values, nan=0.0, posinf=3.0, neginf=-3.0) * 2 ** 20).astype(np.int64), "int64")


def test_pool_one_long_segment_singletons_and_three_slabs(the_snake, dense):
    import torch
    g, cells = the_snake
    M = cells.shape[0]
    rng = np.random.default_rng(50)
    seg = g.segments(connectivity=6)
    assert seg.num_segments() == 1
    want = check_pool(g, seg, (rng.random((M, 13)) * 200).astype(F), "one segment of 4160 voxels")
    assert want["weights"][0] == M
    g, cells = dense                                      # a checkerboard at 6: every voxel ends a run
    lab = torch.from_numpy((cells.sum(axis=1) % 2).astype(np.int32)).to(g.voxel_count.device)
    seg = g.segments(lab, 2, 6)
    assert seg.num_segments() == cells.shape[0]
    check_pool(g, seg, (rng.random((cells.shape[0], 13)) - 0.5).astype(F), "singletons", weight="rows")
    g, cells = lattice(np.ones((128, 128, 4), bool))      # 65 536 voxels: a wave takes four steps of consecutive voxels
    lab = torch.from_numpy((cells[:, 0] // 50).astype(np.int32)).to(g.voxel_count.device)
    seg = g.segments(lab, 3, 6)
    assert seg.num_segments() == 3
    want = check_pool(g, seg, (rng.random((cells.shape[0], 13)) * 256).astype(F), "three slabs of 65 536 voxels")
    assert want["weights"][:3].tolist() == [50 * 512, 50 * 512, 28 * 512]


def test_pool_ties_zero_rows_no_segment_and_the_bits_of_the_mean():
    import torch
    g, _ = lattice(np.ones((8, 1, 1), bool))
    dev = g.voxel_count.device
    lab = torch.tensor([0, 0, 1, 1, 2, 2, 0, 0], dtype=torch.int32, device=dev)
    seg = g.segments(lab, 3, 6)
    assert seg.num_segments() == 4
    v = np.zeros((8, 3), F)
    v[0] = (0.5, 0.25, 0.0)
    v[1] = (0.0, 0.25, 0.5)                               # sums 0.5, 0.5, 0.5: the lowest class
    v[4] = (-1.0, -2.0, -3.0)                             # all negative: class 0, not -1
    v[6] = (1.0, 2.0, 2.0)
    v[7] = (np.nan, 0.0, 0.0)                             # does not contribute
    want = check_pool(g, seg, v, "ties and zeros")
    assert want["label"][:4].tolist() == [0, -1, 0, 1] and want["voxel_label"].tolist() == [0, 0, -1, -1, 0, 0, 1, 1]
    assert want["stats"].tolist() == [7, 1, 3, 1] and want["mean"][3].tolist() == [1.0, 2.0, 2.0]
    # int64: sums past 2^53 whose float64 conversion rounds, a wrapped sum, and odd weights
    big = np.zeros((8, 2), np.int64)
    big[0], big[1] = ((1 << 60) + 1, 3), ((1 << 60) + 2, 4)
    big[2], big[3] = ((1 << 62) + 1, -7), ((1 << 62) + 1, 1 << 40)
    big[4], big[5] = (-(1 << 55) - 1, 5), (-3, 5)
    want = check_pool(g, seg, big, "int64 past 2^53")
    assert abs(int(want["sums"][0, 0])) > 1 << 53 and want["sums"][1, 0] == -(1 << 63) + 2
    none = g.segments(torch.full((8,), 9, dtype=torch.int32, device=dev), 3, 6)        # S = 0: every row is filler
    want = check_pool(g, none, v, "no segment")
    assert want["stats"].tolist() == [0, 0, 0, 0] and (want["voxel_label"] == -1).all() and not want["sums"].any()


def test_pool_a_real_scenescores_on_a_merged_segmentation():
    import torch
    from pointwise_amd import grid, scene
    dev = _dev()
    data = room_cloud(5000, 7501)
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=0.1).trim()
    V = g.num_voxels()
    nrm = g.normals()
    seg = g.segments(normals=nrm, max_angle=20)
    adj = seg.adjacency()
    if adj.overflowed():
        adj = seg.adjacency(max_edges=adj.edges_bound())
    E = adj.num_edges()
    select = torch.zeros(adj.shape[1], dtype=torch.bool, device=dev)
    select[:E] = seg.size[adj.src[:E].long()] < 3
    merged = adj.merge(select)
    assert merged.num_segments() < seg.num_segments()
    rng = np.random.default_rng(60)
    scores = scene.SceneScores(V, 13, dev)
    votes = 3 * V
    index = torch.from_numpy(rng.integers(0, V, votes).astype(np.int32)).to(dev)
    scores.add(torch.from_numpy(rng.standard_normal((votes, 13)).astype(F) * 3).to(dev), index)
    pool = merged.pool(scores.scores)
    want = sm.pool_ref(scores.scores.cpu().numpy(), merged.segment.cpu().numpy(), merged.num_segments(), g.voxel_count.cpu().numpy(), V, 0)
    same(host(pool, POOL), want, "SceneScores on merge()")
    assert want["stats"][0] == V and want["stats"][2] + want["stats"][3] == merged.num_segments() and want["stats"][2] > 0
    rows = g.project(pool.voxel_label).cpu().numpy()                              # the patch's class for every raw row
    inv = g.inverse.cpu().numpy()
    assert np.array_equal(rows[inv >= 0], want["voxel_label"][inv[inv >= 0]]) and (rows[inv < 0] == -1).all()
    check_pool(g, merged, nrm.normals.cpu().numpy(), "mean normals on merge()", weight="rows")
