"""CPU tests (not gpu) of the per-segment geometry (include/conv3p.h: conv3p_grid_segment_geometry, rules G1-G8):
tests/grid_geometry_ref.py against the L of three voxels worked out by hand and against a brute-force loop on random
lattices, the symbol in _lib's table (and no new size function), every Python argument check of GridSegments.geometry (each
raises before any device work: the objects here live on the CPU), the C entry's statuses and the notes of the new kernels'
code objects."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_geometry_ref as gg

F = np.float32
R2 = 1.0 / math.sqrt(2.0)


def ref(cells, segment, S, count=None, data=None, ne=None, weight=0):
    cells = np.asarray(cells, dtype=np.int32)
    M = cells.shape[0]
    data = (cells + 0.5).astype(F) if data is None else data
    return gg.geometry_ref(data, cells, np.ones(M, np.int32) if count is None else count, np.asarray(segment, np.int32), S,
                           M if ne is None else ne, weight)


# ------------------------------------------------------------------------------------------ the reference, by hand
def test_the_l_of_three_voxels():
    r = ref([(0, 0, 0), (1, 0, 0), (1, 1, 0)], [0, 0, 0], 1)
    assert r["cell_box"].tolist() == [[0, 0, 0, 1, 1, 0], [0, 0, 0, -1, -1, -1], [0, 0, 0, -1, -1, -1]]
    assert r["box"][0].tolist() == [0.5, 0.5, 0.5, 1.5, 1.5, 0.5] and not r["box"][1:].any()
    assert r["moments"][0].tolist() == [3, 2, 1, 0, 2, 1, 0, 1, 0, 0] and not r["moments"][1:].any()
    assert r["centroid"][0].tolist() == [2 / 3, 1 / 3, 0.0] and r["centroid"].dtype == np.float64
    assert np.allclose(r["eigenvalues"][0], [1 / 3, 1 / 9, 0.0], rtol=0, atol=4 * gg.U) and r["eigenvalues"][0, 2] == 0.0
    ax = r["axes"][0]
    assert np.allclose(ax[0], [R2, R2, 0.0], rtol=0, atol=4 * gg.U) and ax[2].tolist() == [0.0, 0.0, 1.0]
    # the second axis has two components of one magnitude: G7's tie makes the FIRST positive
    assert np.allclose(np.abs(ax[1]), [R2, R2, 0.0], rtol=0, atol=4 * gg.U) and ax[1][0] * ax[1][1] < 0
    assert gg.sign_rule([-R2, R2, 0.0]).tolist() == [R2, -R2, 0.0] and gg.sign_rule([R2, -R2, 0.0]).tolist() == [R2, -R2, 0.0]
    assert gg.sign_rule([0.0, -0.5, 0.5]).tolist() == [0.0, 0.5, -0.5] and gg.sign_rule([0.1, 0.2, -0.3]).tolist() == [-0.1, -0.2, 0.3]
    if abs(ax[1][0]) == abs(ax[1][1]):
        assert ax[1][0] > 0
    assert r["stats"].tolist() == [1, 0, 1, 0]
    # the extents along those axes: the cells about the centroid
    q = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0)], np.float64) - r["centroid"][0]
    p = q @ ax.T
    assert np.allclose(r["extent"][0], np.concatenate([p.min(axis=0), p.max(axis=0)]), rtol=0, atol=4 * gg.U)
    assert max(gg.figures(r["moments"], 1, r["eigenvalues"], r["axes"])) <= 8


def test_weights_members_and_filler():
    cells = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (5, 5, 5), (6, 5, 5)]
    count = np.array([2, 3, 5, 7, 11], np.int32)
    r = ref(cells, [0, 0, 0, 1, 7], 2, count=count, weight=1)                # 7 >= S: a member of nothing
    assert r["moments"][0].tolist() == [10, 8, 5, 0, 8, 5, 0, 5, 0, 0] and r["moments"][1].tolist() == [7] + [0] * 9
    assert r["cell_box"][1].tolist() == [5, 5, 5, 5, 5, 5] and r["centroid"][1].tolist() == [5.0, 5.0, 5.0]
    assert r["centroid"][0].tolist() == [0.8, 0.5, 0.0] and r["stats"].tolist() == [2, 1, 2, 0]
    assert not r["eigenvalues"][1].any() and r["axes"][1].tolist() == np.eye(3).tolist() and not r["extent"][1].any()
    assert r["cell_box"][2:].tolist() == [[0, 0, 0, -1, -1, -1]] * 3
    for k in ("box", "moments", "centroid", "eigenvalues", "axes", "extent"):
        assert not r[k][2:].any(), k
    # ne cuts the voxels from 3 on: segment 1 has no member and is filler, S stays
    r = ref(cells, [0, 0, 0, 1, 1], 2, ne=3)
    assert r["cell_box"][1].tolist() == [0, 0, 0, -1, -1, -1] and not r["moments"][1].any() and r["stats"].tolist() == [2, 0, 1, 0]


def test_the_order_of_the_bits():
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], F)
    k = gg.key32(x)
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(gg.unkey32(k).view(np.uint32), x.view(np.uint32))
    k = gg.key64(x.astype(np.float64))
    assert (k[1:] > k[:-1]).all() and np.array_equal(gg.unkey64(k).view(np.uint64), x.astype(np.float64).view(np.uint64))
    data = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, np.nan]], F)
    r = ref([(0, 0, 0), (1, 0, 0)], [0, 0], 1, data=data)
    assert np.signbit(r["box"][0, 0]) and not np.signbit(r["box"][0, 3]) and r["box"][0, 2] == 2.0 and np.isnan(r["box"][0, 5])


def brute(data, cells, count, segment, S, ne, weight):
    """G1-G5 and G8 by a loop over segments and members, Fractions where the reference has float64."""
    M = len(cells)
    out = []
    for s in range(S):
        mem = [v for v in range(min(ne, M)) if segment[v] == s]
        w = [int(count[v]) if weight else 1 for v in mem]
        if not mem or sum(w) == 0:
            out.append(None)
            continue
        lo = [min(int(cells[v][a]) for v in mem) for a in range(3)]
        hi = [max(int(cells[v][a]) for v in mem) for a in range(3)]
        d = [[int(cells[v][a]) - lo[a] for a in range(3)] for v in mem]
        mo = [sum(w)] + [sum(wi * di[a] for wi, di in zip(w, d)) for a in range(3)]
        mo += [sum(wi * di[a] * di[b] for wi, di in zip(w, d)) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        cen = [lo[a] + Fraction(mo[1 + a], mo[0]) for a in range(3)]
        box = [min(float(data[v][a]) for v in mem) for a in range(3)] + [max(float(data[v][a]) for v in mem) for a in range(3)]
        out.append((lo + hi, box, mo, cen, mem))
    return out


@pytest.mark.parametrize("seed,weight", [(1, 0), (2, 1), (3, 1)])
def test_the_reference_against_a_brute_force_loop(seed, weight):
    rng = np.random.default_rng(seed)
    occ = rng.random((7, 6, 5)) < 0.6
    cells = np.argwhere(occ).astype(np.int32) + rng.integers(0, 1000, 3).astype(np.int32)
    M = cells.shape[0]
    S = 9
    segment = rng.integers(-2, S + 2, M).astype(np.int32)                    # some in no segment
    segment[segment == 4] = 5                                                # segment 4 has no member: filler below S
    count = rng.integers(1, 40, M).astype(np.int32)
    data = ((cells + rng.random((M, 3))) * 0.25 - 3.0).astype(F)               # finite, no zeros: plain min / max is the order
    ne = M - 5
    r = gg.geometry_ref(data, cells, count, segment, S, ne, weight)
    want = brute(data, cells, count, segment, S, ne, weight)
    assert want[4] is None and r["cell_box"][4].tolist() == [0, 0, 0, -1, -1, -1] and not r["moments"][4].any()
    for s, w in enumerate(want):
        if w is None:
            continue
        box, fbox, mo, cen, mem = w
        assert r["cell_box"][s].tolist() == box and r["box"][s].tolist() == fbox and r["moments"][s].tolist() == mo
        assert np.allclose(r["centroid"][s], [float(c) for c in cen], rtol=0, atol=2 ** -40)
        # G8 in Fractions from the reference's own frame: the extremes are where the loop finds them
        ax = r["axes"][s]
        p = np.array([[sum((int(cells[v][a]) - float(r["centroid"][s][a])) * ax[k][a] for a in range(3)) for k in range(3)]
                      for v in mem])
        assert np.allclose(r["extent"][s], np.concatenate([p.min(axis=0), p.max(axis=0)]), rtol=0, atol=2 ** -40)
        assert (r["extent"][s][:3] <= 0).all() and (r["extent"][s][3:] >= 0).all()
    assert max(gg.figures(r["moments"], S, r["eigenvalues"], r["axes"])) <= 64
    for s in gg.live_rows(r["moments"], S):
        for k in range(3):
            assert np.array_equal(gg.sign_rule(r["axes"][s, k]), r["axes"][s, k])
    assert r["stats"][0] == S and r["stats"][1] == sum(1 for w in want if w is not None and w[0][:3] == w[0][3:])


def test_moments_wrap_modulo_two_to_the_64():
    cells = np.array([(0, 0, 0), (2 ** 20 - 1, 0, 0)], np.int32)
    count = np.array([1, 2 ** 30], np.int32)                                 # no subsampling has such a count
    r = ref(cells, [0, 0], 1, count=count, weight=1)
    exact = 2 ** 30 * (2 ** 20 - 1) ** 2
    assert exact >= 2 ** 63 and r["moments"][0, 4] == gg.to_int64(exact) and r["moments"][0, 1] == 2 ** 30 * (2 ** 20 - 1)
    assert (2 ** 20 - 1) ** 2 * 2 ** 24 < 2 ** 64


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_segments(M=4, rooms=False, K=6):
    g = grid.GridRoomSubsample(10, 2, M, K, False, "cpu") if rooms else grid.GridSubsample(10, M, K, False, "cpu")
    seg = grid.GridSegments(M, "cpu")
    seg._source = (g, None, 0, 1, 26)
    return seg


def test_the_checks_pass_up_to_the_device_check():
    for kw in ({}, {"weight": "voxels"}, {"weight": "rows"}, {"out": grid.SegmentGeometry(4, "cpu")}):
        for seg in (cpu_segments(), cpu_segments(rooms=True), cpu_segments(K=3)):
            with pytest.raises(Conv3pError, match="no CPU path"):
                seg.geometry(**kw)
    with pytest.raises(Conv3pError, match="no CPU path"):
        cpu_segments(0).geometry()


@pytest.mark.parametrize("kw,msg", [
    (dict(weight="voxel"), "weight must be"), (dict(weight=0), "weight must be"), (dict(weight=None), "weight must be"),
    (dict(weight=True), "weight must be"), (dict(weight=["rows"]), "weight must be"),
    (dict(out=torch.zeros(4, dtype=torch.int32)), "out was made"), (dict(out=grid.SegmentGeometry(5, "cpu")), "out was made"),
    (dict(out=grid.GridSegments(4, "cpu")), "out was made"),
])
def test_geometry_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_segments().geometry(**kw)


def test_geometry_needs_the_object_segments_returned_and_its_tensors():
    seg = cpu_segments()
    seg.stats[0] = 2
    with pytest.raises(Conv3pError, match="not on its trim"):
        seg.trim().geometry()
    with pytest.raises(Conv3pError, match="not on its trim"):
        grid.GridSegments(4, "cpu").geometry()
    seg = cpu_segments()
    seg._source[0].data = seg._source[0].data.double()
    with pytest.raises(Conv3pError, match="data must be"):
        seg.geometry()
    seg = cpu_segments()
    seg._source[0].voxel_cell = seg._source[0].voxel_cell[:3]
    with pytest.raises(Conv3pError, match="voxel_cell must be"):
        seg.geometry()
    seg = cpu_segments()
    seg.segment = seg.segment.long()
    with pytest.raises(Conv3pError, match="segment must be"):
        seg.geometry()


def test_the_result_object():
    geo = grid.SegmentGeometry(5, "cpu")
    shapes = dict(cell_box=(5, 6), box=(5, 6), moments=(5, 10), centroid=(5, 3), eigenvalues=(5, 3), axes=(5, 3, 3),
                  extent=(5, 6), stats=(4,))
    dtypes = dict(cell_box=torch.int32, box=torch.float32, moments=torch.int64, stats=torch.int32)
    for k, shape in shapes.items():
        t = getattr(geo, k)
        assert tuple(t.shape) == shape and t.dtype == dtypes.get(k, torch.float64) and t.is_contiguous(), k
    geo.stats[0] = 2
    t = geo.trim()
    assert geo.num_segments() == 2 and t.shape == (2,) and t.stats is geo.stats
    for k, shape in shapes.items():
        if k != "stats":
            assert tuple(getattr(t, k).shape) == (2,) + shape[1:] and getattr(t, k).data_ptr() == getattr(geo, k).data_ptr()
    assert grid.SegmentGeometry is __import__("pointwise_amd").SegmentGeometry


# -------------------------------------------------------------------------------------------------------- the C entry
NAMES = ["voxel_data", "K", "voxel_cell", "voxel_count", "segment", "seg_stats", "grid_stats", "M", "weight", "cell_box", "box",
         "moments", "centroid", "eigenvalues", "axes", "extent", "geometry_stats", "stream"]


def test_the_symbol_is_declared_and_exported_without_a_size_function():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = "conv3p_grid_segment_geometry"
    assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == len(NAMES) == 18
    assert _lib.SYMBOLS[name][1][NAMES.index("M")] is ctypes.c_int64 and _lib.SYMBOLS[name][0] is ctypes.c_int
    assert not [n for n in _lib.SYMBOLS if "geometry" in n and n != name]
    assert not [n for n in _lib.SYMBOLS if n.endswith("_bytes") and "geom" in n]
    assert _lib.load().conv3p_abi_version() == 5


def test_the_c_entry_refuses_bad_arguments_without_a_launch():
    f = _lib.load().conv3p_grid_segment_geometry
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    ok_args = [p, 6, p, p, p, p, p, 4, 0, p, p, p, p, p, p, p, p, None]

    def call(**ch):
        a = list(ok_args)
        for key, val in ch.items():
            a[NAMES.index(key)] = val
        return f(*a)

    for ch in [{"M": -1}, {"K": 2}, {"K": 0}, {"K": -3}, {"weight": 2}, {"weight": -1}] + \
              [{n: None} for n in NAMES if n not in ("K", "M", "weight", "stream")]:
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31) == _lib.ERR_UNSUPPORTED and call(K=65537) == _lib.ERR_UNSUPPORTED
    assert call(M=1 << 31, cell_box=None) == _lib.ERR_INVALID_ARGUMENT       # a NULL pointer is reported first
    # no voxels: nothing to do, whatever the pointers; the argument checks still come first
    assert call(M=0) == _lib.OK and call(M=0, K=65537) == _lib.OK
    nulls = [None if a == p else a for a in ok_args]
    nulls[NAMES.index("M")] = 0
    assert f(*nulls) == _lib.OK
    assert call(M=0, weight=2) == _lib.ERR_INVALID_ARGUMENT and call(M=0, K=2) == _lib.ERR_INVALID_ARGUMENT


def test_the_code_objects_have_no_spill_and_no_private_segment():
    names = ("geom_init_kernel", "geom_box_kernel", "geom_moments_kernel", "geom_frame_kernel", "geom_extent_kernel",
             "geom_finish_kernel")
    res = [r for r in build.kernel_resources() if any(n in r[0] for n in names)]
    assert len(res) == len(names)
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
