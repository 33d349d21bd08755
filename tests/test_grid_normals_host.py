"""CPU tests (not gpu) of the per-voxel normals: tests/grid_normals_ref.py against cases written out by hand and against
the geometry of a sphere, its R6 checker, every Python argument check of GridSubsample.normals / with_normals (each raises
before any device work: the objects here live on the CPU), the C entry's statuses, the new symbol in _lib's table and the
notes of the new kernel's code object."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_interp_ref as gi
from tests import grid_normals_ref as gn
from tests import grid_ref as gr

F = np.float32


# ------------------------------------------------------------------------------------- the reference against hand cases
def test_a_patch_on_a_plane_written_out_by_hand():
    # 3 x 3 representatives on z = 0.75, at the dyadic offsets (i, j) / 4 + 1 / 8: every step below is exact
    ij = np.stack(np.meshgrid(np.arange(3), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3 - 1)
    xyz = np.concatenate([ij * 0.25 + 0.125, np.full((9, 1), 0.75)], axis=1).astype(F)
    cell = np.concatenate([ij, np.zeros((9, 1), int)], axis=1).astype(np.int32)
    neigh = gi.neighbors_ref(cell, 9)
    samples, flags, mo, stats = gn.moments_ref(xyz, neigh, 9, min_neighbors=6)
    assert samples.tolist() == [4, 6, 4, 6, 9, 6, 4, 6, 4] and flags.tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 1]
    assert stats.tolist() == [5, 4, 0, 0]
    assert not mo[:, [5, 7, 8]].any() and not mo[:, 2].any()             # C_xz = C_yz = C_zz = 0 and m_z = 0, exactly
    # the centre: q = (+-1/4, 0)^2, m = 0, C_xx = C_yy = 6 (1/16) / 9, C_xy = 0
    assert mo[4].tolist() == [0, 0, 0, F(F(0.375) / F(9)), 0, 0, F(F(0.375) / F(9)), 0, 0]
    # voxel 1 = cell (0, 1): samples at x offsets {0, 0, 0, 1/4, 1/4, 1/4}, y offsets {-1/4, 0, 1/4} twice
    assert mo[1, 0] == F(F(0.75) / F(6)) and mo[1, 1] == 0 and mo[1, 3] == F(F(6 * 0.125 * 0.125) / F(6))
    r = gn.normals_ref(xyz, neigh, 9, 6)
    good = flags == 0
    assert np.array_equal(r["normals"][good], np.tile(np.array([0, 0, 1], F), (5, 1)))     # largest component positive
    assert not r["normals"][~good].any() and not r["curvature"].any()
    down = gn.normals_ref(xyz, neigh, 9, 6, viewpoint=[0.3, 0.3, -2.0])
    assert np.array_equal(down["normals"][good], np.tile(np.array([0, 0, -1], F), (5, 1)))
    with_3 = gn.moments_ref(xyz, neigh, 9, min_neighbors=3)
    assert (with_3[1] == 0).all() and with_3[3].tolist() == [9, 0, 0, 0]
    # filler rows behind the emitted voxels, and a cut: rows past ne hold R1's values and are nobody's sample
    wide = np.concatenate([xyz, np.full((2, 3), 7.0, F)])
    s2, f2, m2, st2 = gn.moments_ref(wide, np.concatenate([neigh, np.full((2, 27), -1, np.int32)]), 9, 6)
    assert np.array_equal(s2[:9], samples) and f2[9:].tolist() == [-1, -1] and not m2[9:].any() and st2.tolist() == [5, 4, 0, 2]
    s3, f3, m3, st3 = gn.moments_ref(xyz, neigh, 5, 3)
    assert s3.tolist() == [4, 5, 3, 4, 5, 0, 0, 0, 0] and f3.tolist() == [0, 0, 0, 0, 0, -1, -1, -1, -1] and st3.tolist() == [5, 0, 0, 4]


def test_a_single_voxel_and_a_degenerate_one():
    neigh = np.full((1, 27), -1, np.int32)
    neigh[0, 13] = 0
    samples, flags, mo, stats = gn.moments_ref(np.array([[0.3, -1.0, 2.0, 5.0]], F), neigh, 1, 3)
    assert samples.tolist() == [1] and flags.tolist() == [1] and not mo.any() and stats.tolist() == [0, 1, 0, 0]
    samples, flags, mo, stats = gn.moments_ref(np.array([[np.nan, -1.0, 2.0]], F), neigh, 1, 3)
    assert samples.tolist() == [0] and flags.tolist() == [1] and not mo.any()
    # three coincident representatives: n = 3, every moment 0, the trace is not positive
    xyz = np.ones((3, 3), F)
    neigh = np.full((3, 27), -1, np.int32)
    neigh[:, 13] = [0, 1, 2]
    neigh[0, 22], neigh[1, 4], neigh[1, 22], neigh[2, 4], neigh[0, 14], neigh[2, 12] = 1, 0, 2, 1, 2, 0
    samples, flags, mo, stats = gn.moments_ref(xyz, neigh, 3, 3)
    assert samples.tolist() == [3, 3, 3] and flags.tolist() == [2, 2, 2] and stats.tolist() == [0, 0, 3, 0]
    # differences that overflow: finite representatives, non-finite moments
    xyz = np.array([[3e38, 0, 0], [-3e38, 0, 0], [0, 0, 0]], F)
    assert gn.moments_ref(xyz, neigh, 3, 3)[1].tolist() == [2, 2, 2]


# -------------------------------------------------------------------------------------- the reference against geometry
def test_the_reference_normals_of_a_sphere_are_radial():
    """Case 4 of tests/test_grid_normals.py: 8000 rows on the unit sphere at voxel 0.1.  Bound: 0.35 rad at every
    flags-0 voxel.  Measured worst angle between the reference normal and the radial direction of the representative:
    0.0815 rad (mean), 0.0832 rad (center), 1488 voxels, all of them flags 0."""
    data = gn.sphere()
    for mode in ("mean", "center"):
        g = gr.grid_subsample_ref(data, None, voxel=0.1, mode=mode)
        nv = int(g["stats"][0])
        neigh = gi.neighbors_ref(g["voxel_cell"], nv)
        r = gn.normals_ref(g["data"], neigh, nv, 6, viewpoint=[0.0, 0.0, 0.0])
        good = r["flags"] == 0
        assert good.sum() > 1000
        p = g["data"][good, :3].astype(np.float64)
        radial = p / np.sqrt((p * p).sum(axis=1))[:, None]
        dot = (r["normals"][good] * radial).sum(axis=1)
        assert (dot < 0).all()                                           # turned towards the centre
        worst = np.arccos(np.minimum(np.abs(dot), 1.0)).max()
        print("sphere, %s: worst angle to the radial direction %.4f rad over %d voxels" % (mode, worst, good.sum()))
        assert worst <= 0.35
        compared, of, ratio = gn.compare_r5(r["normals"], r["curvature"], r["flags"], r["moments"], g["data"], [0.0, 0.0, 0.0],
                                            max_left_out=0.01)
        assert compared == of and ratio <= 1.0                           # the reference against itself: float32 rounding


# ----------------------------------------------------------------------------------------------------- the R6 checker
def test_the_orientation_checker():
    p = np.zeros((1, 3), F)
    up, w = np.array([[0.0, 0.6, 0.8]], F), np.array([[0.0, 0.0, 5.0]], F)
    assert gn.orientation_s(up, p, w)[0] == F(4.0)
    assert gn.orientation_ok(up, p, w)[0] and not gn.orientation_ok(-up, p, w)[0]           # s > 0 holds, s < 0 does not
    # s == 0: the viewpoint lies in the plane; the largest component decides, whatever the others' signs
    side = np.array([[5.0, 0.0, 0.0]], F)
    assert gn.orientation_s(up, p, side)[0] == 0
    assert gn.orientation_ok(up, p, side)[0] and not gn.orientation_ok(-up, p, side)[0]
    assert gn.orientation_ok(np.array([[-0.6, 0.0, 0.8]], F), p, np.array([[4.0, 0.0, 3.0]], F))[0]   # -2.4 + 2.4 = 0
    # a non-finite s (a viewpoint at infinity or a NaN row for "no viewpoint"): the axis rule again
    for far in ([[np.inf, 0.0, 0.0]], [[np.nan] * 3]):
        far = np.array(far, F)
        assert gn.orientation_ok(up, p, far)[0] and not gn.orientation_ok(-up, p, far)[0]
    # no viewpoint at all
    assert gn.orientation_ok(up)[0] and not gn.orientation_ok(-up)[0]
    assert gn.orientation_ok(np.array([[-0.1, 0.1, 0.99]], F))[0] and not gn.orientation_ok(np.array([[0.1, 0.1, -0.99]], F))[0]
    # ties in magnitude go to the lowest axis: (x, y) tied -> x decides; (y, z) tied -> y; all three -> x
    h = F(np.sqrt(0.5))
    assert gn.orientation_ok(np.array([[h, -h, 0.0]], F))[0] and not gn.orientation_ok(np.array([[-h, h, 0.0]], F))[0]
    assert gn.orientation_ok(np.array([[0.0, h, -h]], F))[0] and not gn.orientation_ok(np.array([[0.0, -h, h]], F))[0]
    t = F(np.sqrt(1.0 / 3.0))
    assert gn.orientation_ok(np.array([[t, -t, -t]], F))[0] and not gn.orientation_ok(np.array([[-t, t, t]], F))[0]
    # per-room viewpoints: a room outside [0, R) has none
    w = gn.viewpoints_of(np.array([[0, 0, 5], [0, 0, -5]], F), np.array([0, 1, 2, -1]), 4)
    n = np.array([[0, 0.6, 0.8], [0, 0.6, -0.8], [0, -0.6, -0.8], [0, 0.6, 0.8]], F)
    assert gn.orientation_ok(n, np.zeros((4, 3), F), w).tolist() == [True, True, False, True]
    # negation is exact: s of the negated vector is the negated s, to the bit
    rng = np.random.default_rng(5)
    n, pp, ww = (rng.standard_normal((1000, 3)).astype(F) for _ in range(3))
    assert np.array_equal(gn.orientation_s(-n, pp, ww), -gn.orientation_s(n, pp, ww))


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_object(M=4, K=6, rooms=False):
    return grid.GridRoomSubsample(10, 2, M, K, False, "cpu") if rooms else grid.GridSubsample(10, M, K, False, "cpu")


def test_the_checks_pass_up_to_the_device_check():
    for kw in ({}, {"viewpoint": (1.0, 2, 3.5)}, {"viewpoint": np.array([1.0, 2.0, 3.0])}, {"viewpoint": torch.zeros((1, 3))},
               {"min_neighbors": 3, "return_moments": True}, {"min_neighbors": 27, "out": grid.GridNormals(4, False, "cpu")},
               {"return_moments": True, "out": grid.GridNormals(4, True, "cpu")}):
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_object().normals(**kw)
    for vp in (torch.zeros((1, 3)), torch.zeros((2, 3)), [0.0, 0.0, 0.0], None):
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_object(rooms=True).normals(viewpoint=vp)


@pytest.mark.parametrize("what,msg", [
    ("min 2", "min_neighbors must be"), ("min 28", "min_neighbors must be"), ("min float", "min_neighbors must be"),
    ("min bool", "min_neighbors must be"), ("moments int", "return_moments must be"),
    ("vp two", "viewpoint must be"), ("vp four", "viewpoint must be"), ("vp nan", "viewpoint must be"),
    ("vp inf", "viewpoint must be"), ("vp huge", "viewpoint must be"), ("vp string", "viewpoint must be"),
    ("vp number", "viewpoint must be"), ("vp dtype", "viewpoint must be"), ("vp flat", "viewpoint must be"),
    ("vp columns", "viewpoint must be"), ("vp empty", "viewpoint must be"), ("vp strided", "viewpoint must be"),
    ("vp rows single", "needs a GridRoomSubsample"), ("vp rows rooms", "one per room"),
    ("out type", "out was made"), ("out shape", "out was made"), ("out moments", "out was made"),
    ("room dtype", "voxel_room must be"), ("room shape", "voxel_room must be"),
])
def test_normals_refuses_before_any_device_work(what, msg):
    g = cpu_object(rooms=what in ("vp rows rooms", "room dtype", "room shape"))
    kw = {}
    if what == "min 2": kw["min_neighbors"] = 2
    elif what == "min 28": kw["min_neighbors"] = 28
    elif what == "min float": kw["min_neighbors"] = 6.0
    elif what == "min bool": kw["min_neighbors"] = True
    elif what == "moments int": kw["return_moments"] = 1
    elif what == "vp two": kw["viewpoint"] = (1.0, 2.0)
    elif what == "vp four": kw["viewpoint"] = (1.0, 2.0, 3.0, 4.0)
    elif what == "vp nan": kw["viewpoint"] = (1.0, float("nan"), 3.0)
    elif what == "vp inf": kw["viewpoint"] = (1.0, 2.0, float("inf"))
    elif what == "vp huge": kw["viewpoint"] = (1.0, 2.0, 1e39)
    elif what == "vp string": kw["viewpoint"] = "abc"
    elif what == "vp number": kw["viewpoint"] = 3.0
    elif what == "vp dtype": kw["viewpoint"] = torch.zeros((1, 3), dtype=torch.float64)
    elif what == "vp flat": kw["viewpoint"] = torch.zeros(3)
    elif what == "vp columns": kw["viewpoint"] = torch.zeros((1, 4))
    elif what == "vp empty": kw["viewpoint"] = torch.zeros((0, 3))
    elif what == "vp strided": kw["viewpoint"] = torch.zeros((1, 6))[:, ::2]
    elif what == "vp rows single": kw["viewpoint"] = torch.zeros((2, 3))
    elif what == "vp rows rooms": kw["viewpoint"] = torch.zeros((3, 3))
    elif what == "out type": kw["out"] = torch.zeros((4, 3))
    elif what == "out shape": kw["out"] = grid.GridNormals(5, False, "cpu")
    elif what == "out moments": kw["out"] = grid.GridNormals(4, True, "cpu")
    elif what == "room dtype": g.voxel_room = g.voxel_room.long()
    elif what == "room shape": g.voxel_room = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(Conv3pError, match=msg):
        g.normals(**kw)


def test_with_normals_on_the_host():
    g = cpu_object()
    g.data.copy_(torch.arange(24.0).reshape(4, 6))
    nrm = grid.GridNormals(4, False, "cpu")
    nrm.normals.copy_(torch.arange(100.0, 112.0).reshape(4, 3))
    nrm.curvature.copy_(torch.arange(200.0, 204.0))
    a, b = g.with_normals(nrm), g.with_normals(nrm, curvature=True)
    assert a.shape == (4, 9) and b.shape == (4, 10) and a.is_contiguous() and b.is_contiguous() and a.dtype == torch.float32
    assert torch.equal(a[:, :6], g.data) and torch.equal(a[:, 6:], nrm.normals) and torch.equal(b[:, :9], a)
    assert torch.equal(b[:, 9], nrm.curvature)
    for bad, msg in ((dict(nrm=nrm.normals), "must be the GridNormals"), (dict(nrm=grid.GridNormals(5, False, "cpu")), "another subsampling"),
                     (dict(nrm=nrm, curvature=1), "curvature must be a bool")):
        with pytest.raises(Conv3pError, match=msg):
            g.with_normals(**bad)


# ---------------------------------------------------------------------------------------------------------- the C entry
def test_the_new_symbol_is_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "conv3p_grid_normals_f32" in _lib.SYMBOLS and hasattr(lib, "conv3p_grid_normals_f32")
    assert len(_lib.SYMBOLS["conv3p_grid_normals_f32"][1]) == 16
    assert _lib.load().conv3p_abi_version() == 5
    assert grid.GridNormals is __import__("pointwise_amd").GridNormals


def test_the_c_entry_refuses_bad_arguments_without_a_launch():
    f = _lib.load().conv3p_grid_normals_f32
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    names = ["voxel_data", "K", "neigh", "grid_stats", "voxel_room", "viewpoint", "V", "M", "min_neighbors", "normals",
             "curvature", "samples", "flags", "moments", "normal_stats", "stream"]
    ok_args = [p, 6, p, p, None, None, 0, 4, 6, p, p, p, p, None, p, None]

    def call(**ch):
        a = list(ok_args)
        for key, val in ch.items():
            a[names.index(key)] = val
        return f(*a)

    for ch in ({"M": -1}, {"K": 2}, {"K": 0}, {"min_neighbors": 2}, {"min_neighbors": 28}, {"min_neighbors": -1},
               {"viewpoint": p, "V": 0}, {"viewpoint": p, "V": -1}, {"viewpoint": p, "V": 2}, {"viewpoint": p, "V": 3},
               {"voxel_data": None}, {"neigh": None}, {"grid_stats": None}, {"normals": None}, {"curvature": None},
               {"samples": None}, {"flags": None}, {"normal_stats": None}):
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(viewpoint=p, voxel_room=p, V=1 << 31) == _lib.ERR_UNSUPPORTED
    # no voxels: nothing to do, whatever the pointers; the argument checks still come first
    assert call(M=0) == _lib.OK
    assert f(None, 3, None, None, None, None, 0, 0, 3, None, None, None, None, None, None, None) == _lib.OK
    assert call(M=0, K=2) == _lib.ERR_INVALID_ARGUMENT and call(M=0, viewpoint=p, V=2) == _lib.ERR_INVALID_ARGUMENT


def test_the_code_object_has_no_spill_and_no_private_segment():
    res = [r for r in build.kernel_resources() if "grid_normals_kernel" in r[0]]
    assert len(res) == 1
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
