"""CPU tests (not gpu) of the smooth segments and the per-segment pool: tests/grid_smooth_ref.py on cases written out by
hand, the new symbols and their argument counts in _lib's table, every status of conv3p_grid_segments_smooth and
conv3p_grid_segment_pool_f32 / _i64 that returns before a launch (through ctypes), the Python argument checks of
GridSubsample.segments' six keywords and of GridSegments.pool (each raises before any device work: the objects here live on
the CPU), absorb() on a smooth result, and the notes of the new kernels' code objects."""
import ctypes
import math

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_segments_ref as gs
from tests import grid_smooth_ref as sm

F = np.float32
NAN = float("nan")


def run(neigh, connectivity=6, labels=None, num_class=None, **rule):
    M = neigh.shape[0]
    return sm.smooth_segments_ref(neigh, labels, 0 if labels is None else labels.shape[0], np.ones(M, np.int32), M, num_class,
                                  connectivity, **rule)


# ------------------------------------------------------------------------------------- the reference on hand cases
@pytest.mark.parametrize("connectivity,at30,at45", [(6, (101, 93), (101, 101)), (26, (195, 165), (195, 185))])
def test_a_floor_and_a_wall_that_meet_in_a_crease(connectivity, at30, at45):
    occ, nrm = sm.hand_case()
    neigh, cells = gs.lattice_table(occ)
    assert cells.shape[0] == 60
    r = run(neigh, connectivity, normals=nrm, min_cos=sm.min_cos_of(30))
    first_floor = int(np.nonzero(cells[:, 0] > 0)[0][0])
    assert r["stats"][0] == 3 and r["size"][:3].tolist() == [4, 28, 28]
    assert r["segment"][:3].tolist() == [0, 1, 1] and r["segment"][first_floor] == 2
    assert tuple(r["smooth_stats"][:2]) == at30 and r["smooth_stats"][3] == at30[0] - at30[1]
    # 45 degrees: the crease's dot product IS min_cos, and equality joins
    h = F(np.sqrt(0.5))
    assert sm.min_cos_of(45) == h == F(0.70710677) and (h * F(1) + F(0) * F(0)) + h * F(0) == h
    r = run(neigh, connectivity, normals=nrm, min_cos=sm.min_cos_of(45))
    assert r["stats"][0] == 1 and r["size"][0] == 60 and tuple(r["smooth_stats"][:2]) == at45
    # the threshold one ulp above the dot product: the crease joins neither side, as at 30 degrees
    r = run(neigh, connectivity, normals=nrm, min_cos=np.nextafter(h, F(1)))
    assert r["stats"][0] == 3 and r["size"][:3].tolist() == [4, 28, 28] and tuple(r["smooth_stats"][:2]) == at30


def test_a_line_of_voxels_under_every_rule():
    neigh, _ = gs.lattice_table(np.ones((6, 1, 1), bool))
    up, side = (0, 0, 1), (1, 0, 0)
    nrm = np.array([up, up, side, side, (0, 0, -1), (0, 0, -1)], F)
    r = run(neigh, normals=nrm, min_cos=F(0.5))
    assert r["segment"].tolist() == [0, 0, 1, 1, 2, 2] and r["smooth_stats"].tolist() == [5, 3, 0, 2, 0, 0, 0, 0]
    # unsigned: a flipped normal is the same surface; signed: it is not
    nrm = np.array([up, up, (0, 0, -1), up, up, up], F)
    assert run(neigh, normals=nrm, min_cos=F(0.5))["stats"][0] == 1
    r = run(neigh, normals=nrm, min_cos=F(0.5), signed=True)
    assert r["segment"].tolist() == [0, 0, 1, 2, 2, 2] and r["smooth_stats"][3] == 2
    # a flagged voxel and a non-finite normal: segments of their own, counted in [2] and [6]
    nrm = np.array([up, up, up, up, (NAN, 0, 1), up], F)
    flags = np.array([0, 2, 0, 0, 0, 0], np.int32)
    r = run(neigh, normals=nrm, flags=flags, min_cos=F(0.5))
    assert r["segment"].tolist() == [0, 1, 2, 2, 3, 4] and r["smooth_stats"].tolist() == [5, 1, 4, 0, 0, 0, 2, 0]
    assert r["stats"].tolist() == [5, 6, 0, 0, 2, 2, 0, 0]                 # a voxel without a normal is labelled all the same
    # curvature: both ends must be at most the bound, equality passes, a NaN fails; the angle is asked first
    nrm = np.array([up] * 6, F)
    curv = np.array([0.1, 0.25, 0.3, 0.1, NAN, 0.1], F)
    r = run(neigh, normals=nrm, min_cos=F(0.5), curvature=curv, max_curvature=F(0.25))
    assert r["segment"].tolist() == [0, 0, 1, 2, 3, 4] and r["smooth_stats"].tolist() == [5, 1, 0, 0, 4, 0, 0, 0]
    # features alone: every channel within the bound, equality passes, a NaN fails
    feat = np.array([[0, 0], [0.5, 0], [0.5, 0.75], [0.5, NAN], [0.5, 0], [1.0, 0.5]], F)
    r = run(neigh, features=feat, max_difference=F(0.5))
    assert r["segment"].tolist() == [0, 0, 1, 2, 3, 3] and r["smooth_stats"].tolist() == [5, 2, 0, 0, 0, 3, 0, 0]
    # labels first: a pair of two classes is no candidate
    lab = np.array([0, 0, 1, 1, 1, 7], np.int32)
    r = run(neigh, 6, lab, 2, normals=np.array([up] * 6, F), min_cos=F(0.5))
    assert r["segment"].tolist() == [0, 0, 1, 1, 1, -1] and r["smooth_stats"].tolist() == [3, 3, 0, 0, 0, 0, 0, 0]


def test_identical_normals_give_the_plain_segments():
    rng = np.random.default_rng(4)
    occ = rng.random((7, 6, 5)) < 0.7
    neigh, cells = gs.lattice_table(occ)
    M = cells.shape[0]
    lab = rng.integers(0, 3, M).astype(np.int32)
    count = rng.integers(1, 5, M).astype(np.int32)
    for c in (6, 18, 26):
        want = gs.segments_ref(neigh, lab, M, count, M, 3, c)
        got = sm.smooth_segments_ref(neigh, lab, M, count, M, 3, c, normals=np.tile(F([0.6, 0.0, 0.8]), (M, 1)), min_cos=F(0.99))
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert got["smooth_stats"][0] == got["smooth_stats"][1] > 0


def test_the_pool_by_hand():
    segment = np.array([0, 0, 1, 1, -1, 2, 2, 5], np.int32)        # 5 >= S: a member of nothing
    count = np.array([1, 3, 2, 2, 9, 1, 1, 1], np.int32)
    v = np.array([[0.5, 0.25], [0.5, 1.0], [1.0, 1.0], [NAN, 0.0], [3.0, 3.0], [0.0, 0.0], [300.0, 1.0], [1.0, 1.0]], F)
    one = 1 << 30
    r = sm.pool_ref(v, segment, 3, count, 8, 0)
    assert r["sums"][:3].tolist() == [[one, one + one // 4], [one, one], [0, 0]] and r["weights"].tolist() == [2, 1, 1, 0, 0, 0, 0, 0]
    assert r["mean"][:3].tolist() == [[0.5, 0.625], [1.0, 1.0], [0.0, 0.0]] and not r["sums"][3:].any()
    assert r["label"].tolist() == [1, 0, -1, -1, -1, -1, -1, -1]      # a tie to the lowest class; all sums 0: -1
    assert r["voxel_label"].tolist() == [1, 1, 0, 0, -1, -1, -1, -1] and r["stats"].tolist() == [4, 2, 2, 1]
    r = sm.pool_ref(v, segment, 3, count, 8, 1)
    assert r["weights"][:3].tolist() == [4, 2, 1] and r["sums"][0].tolist() == [2 * one, 3 * one + one // 4]
    assert r["mean"][0].tolist() == [0.5, 0.8125]
    r = sm.pool_ref(v[:3], segment, 3, count, 8, 0, with_mean=False)  # L = 3: voxel 3 and segment 2 do not contribute
    assert r["mean"] is None and r["weights"][:3].tolist() == [2, 1, 0] and r["stats"].tolist() == [3, 3, 2, 1]
    # int64: summed as they are, wrapping; a negative row; the mean of a sum beyond 2^53
    big = np.array([[(1 << 62) + 1, 1], [(1 << 62) + 1, -5], [-4, -3], [0, 0]], np.int64)
    r = sm.pool_ref(big, np.array([0, 0, 1, 1], np.int32), 2, count[:4], 4, 0)
    assert r["sums"][0].tolist() == [-(1 << 63) + 2, -4] and r["sums"][1].tolist() == [-4, -3]
    assert r["label"][:2].tolist() == [1, 1] and r["mean"][1].tolist() == [-2.0 / one, -1.5 / one]
    assert r["mean"][0, 0] == float(-(1 << 63) + 2) / (2.0 * one)


# ------------------------------------------------------------------------------------------------------ the C entries
SMOOTH = ["neigh", "voxel_labels", "L", "voxel_count", "grid_stats", "M", "num_class", "connectivity", "segment", "seg_root",
          "seg_size", "seg_rows", "seg_label", "seg_stats", "normals", "normal_flags", "curvature", "min_cos", "signed_normals",
          "max_curvature", "features", "F", "feature_stride", "max_difference", "smooth_stats", "workspace", "workspace_bytes",
          "stream"]
POOL = ["values", "L", "C", "value_stride", "segment", "seg_stats", "voxel_count", "grid_stats", "M", "weight", "sums", "weights",
        "mean", "seg_label", "voxel_label", "pool_stats", "stream"]


def test_the_new_symbols_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in (("conv3p_grid_segments_smooth", len(SMOOTH)), ("conv3p_grid_segment_pool_f32", len(POOL)),
                    ("conv3p_grid_segment_pool_i64", len(POOL))):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n
    assert len(SMOOTH) == 28 and len(POOL) == 17
    assert _lib.SYMBOLS["conv3p_grid_segment_pool_f32"] == _lib.SYMBOLS["conv3p_grid_segment_pool_i64"]
    assert _lib.load().conv3p_abi_version() == 5
    assert not [n for n in _lib.SYMBOLS if "smooth" in n or "pool" in n if n.endswith("_bytes")]     # no new size function
    assert grid.SegmentPool is __import__("pointwise_amd").SegmentPool


def _caller(f, names, ok):
    def call(**ch):
        a = list(ok)
        for key, val in ch.items():
            a[names.index(key)] = val
        return f(*a)
    return call


def test_the_smooth_entry_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below returns before a launch
    p = ctypes.addressof(words)
    need = lib.conv3p_grid_segments_workspace_bytes
    ok = [p, p, 4, p, p, 4, 3, 26, p, p, p, p, p, p, p, p, p, 0.5, 0, 0.1, p, 3, 3, 0.1, p, p, 1 << 40, None]
    call = _caller(lib.conv3p_grid_segments_smooth, SMOOTH, ok)
    bad = [{"M": -1}, {"L": -1}, {"L": 5}, {"num_class": 0}, {"num_class": 129}, {"connectivity": 0}, {"connectivity": 7},
           {"workspace": None}, {"workspace_bytes": need(4) - 1}, {"workspace_bytes": 0}]
    bad += [{n: None} for n in ("neigh", "voxel_count", "grid_stats", "segment", "seg_root", "seg_size", "seg_rows", "seg_label",
                                "seg_stats", "smooth_stats")]
    bad += [{"normals": None, "features": None, "F": 0}, {"F": -1}, {"F": 17}, {"F": 0}, {"features": None},
            {"feature_stride": 2}, {"signed_normals": 2}, {"signed_normals": -1}, {"min_cos": NAN}, {"max_curvature": NAN},
            {"max_difference": NAN}]
    for ch in bad:
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31, L=0) == _lib.ERR_UNSUPPORTED
    assert call(M=0, L=0) == _lib.OK and call(M=0, L=0, connectivity=5) == _lib.ERR_INVALID_ARGUMENT
    assert call(M=0, L=1) == _lib.ERR_INVALID_ARGUMENT


def test_the_pool_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(words)
    ok = [p, 4, 13, 13, p, p, p, p, 4, 0, p, p, p, p, p, p, None]
    for f, rows in ((lib.conv3p_grid_segment_pool_f32, True), (lib.conv3p_grid_segment_pool_i64, False)):
        call = _caller(f, POOL, ok)
        bad = [{"M": -1}, {"L": -1}, {"L": 5}, {"C": 0}, {"C": 129}, {"value_stride": 12}, {"weight": 2}, {"weight": -1}]
        bad += [{n: None} for n in ("values", "segment", "seg_stats", "voxel_count", "grid_stats", "sums", "weights", "seg_label",
                                    "pool_stats")]
        for ch in bad + ([] if rows else [{"weight": 1}]):
            assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
        assert call(M=1 << 31, L=0) == _lib.ERR_UNSUPPORTED
        if rows:
            assert call(M=1 << 31, L=0, weight=1) == _lib.ERR_UNSUPPORTED
        assert call(M=0, L=0) == _lib.OK and call(M=0, L=0, C=0) == _lib.ERR_INVALID_ARGUMENT
        assert call(M=0, L=1) == _lib.ERR_INVALID_ARGUMENT


def test_the_code_objects_have_no_spill_and_no_private_segment():
    names = ("smooth_local_kernel", "smooth_link_kernel", "pool_init_kernel", "pool_sum_kernel", "pool_finish_kernel",
             "pool_voxel_kernel")
    res = [r for r in build.kernel_resources() if any("conv3p" + str(len(n)) + n in r[0] for n in names)]
    assert len(res) == len(names) + 1                     # the sums for float32 and for int64
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 128, (name, vgprs, vgpr_spills, private)
    # the plain kernels are what they were: one code object each, the registers of profiles/grid_segments_time.txt
    plain = {r[0]: r[1] for r in build.kernel_resources() if "gseg_local_kernel" in r[0] or "gseg_link_kernel" in r[0]}
    assert sorted(plain.values()) == [16, 17], plain


# ------------------------------------------------------------------------------------------------- the Python checks
def cpu_object(M=4, rooms=False):
    return grid.GridRoomSubsample(10, 2, M, 6, False, "cpu") if rooms else grid.GridSubsample(10, M, 6, False, "cpu")


def cpu_normals(M=4):
    return grid.GridNormals(M, False, "cpu")


def cpu_segments(M=4, smooth=False):
    seg = grid.GridSegments(M, "cpu")
    seg._source = (cpu_object(M), None, 0, 1, 26)
    seg._smooth = smooth
    return seg


def test_the_checks_pass_up_to_the_device_check():
    nrm, bare, feat = cpu_normals(), torch.zeros((4, 3)), torch.zeros((4, 6))
    lab = torch.zeros(4, dtype=torch.int32)
    for kw in (dict(normals=nrm, max_angle=15), dict(normals=nrm, max_angle=0.0, signed=True, max_curvature=0.1),
               dict(normals=bare, max_angle=180), dict(features=feat, max_difference=0), dict(features=feat[:, 3:6], max_difference=0.5),
               dict(features=feat[:, 2:3], max_difference=math.inf), dict(normals=nrm, max_angle=30, features=feat[:, :4], max_difference=1),
               dict(voxel_labels=lab, num_class=3, connectivity=6, normals=nrm, max_angle=30)):
        for g in (cpu_object(), cpu_object(rooms=True)):
            with pytest.raises(Conv3pError, match="no CPU path"):          # a CPU tensor is refused, loudly, and last
                g.segments(**kw)
    seg = cpu_segments()
    for kw in (dict(values=torch.zeros((4, 13))), dict(values=torch.zeros((2, 1)), weight="rows"),
               dict(values=torch.zeros((4, 128), dtype=torch.int64), return_mean=False), dict(values=torch.zeros((4, 6))[:, 3:6]),
               dict(values=torch.zeros((0, 5)))):
        with pytest.raises(Conv3pError, match="no CPU path"):
            seg.pool(**kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(max_angle=15), "max_angle needs normals"),
    (dict(max_curvature=0.1), "max_curvature needs normals"),
    (dict(signed=True), "signed needs normals"),
    (dict(max_difference=0.1), "max_difference needs features"),
    (dict(normals=torch.zeros((4, 3)), max_angle=15, max_curvature=0.1), "bare tensor"),
    (dict(normals=grid.GridNormals(4, False, "cpu")), "max_angle, in degrees"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=181), "max_angle, in degrees"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=-1), "max_angle, in degrees"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=NAN), "max_angle, in degrees"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=True), "max_angle, in degrees"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=15, signed=1), "signed must be"),
    (dict(normals=grid.GridNormals(4, False, "cpu"), max_angle=15, max_curvature=NAN), "max_curvature must be"),
    (dict(normals=grid.GridNormals(5, False, "cpu"), max_angle=15), "another subsampling"),
    (dict(normals=torch.zeros((5, 3)), max_angle=15), "normals must be"),
    (dict(normals=torch.zeros((4, 3), dtype=torch.float64), max_angle=15), "normals must be"),
    (dict(normals=torch.zeros((4, 6))[:, :3], max_angle=15), "normals must be"),
    (dict(normals=[0, 0, 1], max_angle=15), "normals must be"),
    (dict(features=torch.zeros((4, 3))), "max_difference >= 0"),
    (dict(features=torch.zeros((4, 3)), max_difference=-0.5), "max_difference >= 0"),
    (dict(features=torch.zeros((4, 3)), max_difference=NAN), "max_difference >= 0"),
    (dict(features=torch.zeros((4, 17)), max_difference=1), "features must be"),
    (dict(features=torch.zeros((3, 3)), max_difference=1), "features must be"),
    (dict(features=torch.zeros((4, 3), dtype=torch.float64), max_difference=1), "features must be"),
    (dict(features=torch.zeros((4, 6))[:, ::2], max_difference=1), "contiguous rows"),
    (dict(features=torch.zeros((3, 4)).t(), max_difference=1), "contiguous rows"),
])
def test_segments_refuses_the_smooth_keywords_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_object().segments(**kw)


def test_the_smooth_keywords_are_keyword_only():
    with pytest.raises(TypeError):
        cpu_object().segments(None, None, 26, None, cpu_normals(), 15)


@pytest.mark.parametrize("kw,msg", [
    (dict(values=torch.zeros((5, 3))), "values must be"), (dict(values=torch.zeros((4, 129))), "values must be"),
    (dict(values=torch.zeros((4, 0))), "values must be"), (dict(values=torch.zeros(4)), "values must be"),
    (dict(values=torch.zeros((4, 3), dtype=torch.float64)), "values must be"), (dict(values=None), "values must be"),
    (dict(values=torch.zeros((4, 6))[:, ::2]), "contiguous rows"),
    (dict(values=torch.zeros((4, 3)), weight="points"), "weight must be"), (dict(values=torch.zeros((4, 3)), weight=1), "weight must be"),
    (dict(values=torch.zeros((4, 3), dtype=torch.int64), weight="rows"), "int64 values take"),
    (dict(values=torch.zeros((4, 3)), return_mean=1), "return_mean must be"),
    (dict(values=torch.zeros((4, 3)), out=grid.SegmentPool(4, 4, True, "cpu")), "out was made"),
    (dict(values=torch.zeros((4, 3)), out=grid.SegmentPool(4, 3, False, "cpu")), "out was made"),
])
def test_pool_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_segments().pool(**kw)


def test_absorb_refuses_a_smooth_result_and_pool_its_trim():
    seg = cpu_segments(smooth=True)
    with pytest.raises(Conv3pError, match="smooth segmentation"):
        seg.absorb(2)
    seg.smooth_stats = torch.zeros(8, dtype=torch.int64)
    seg.stats[0] = 2
    t = seg.trim()
    assert t._smooth and t.smooth_stats is seg.smooth_stats and t.root.shape == (2,)
    with pytest.raises(Conv3pError, match="not on its trim"):
        t.pool(torch.zeros((4, 3)))
    plain = cpu_segments().trim()
    assert plain.smooth_stats is None and not plain._smooth
    pool = grid.SegmentPool(4, 3, True, "cpu")
    pool._segments = seg
    tp = pool.trim()
    assert pool.num_segments() == 2 and tp.sums.shape == (2, 3) and tp.mean.shape == (2, 3) and tp.label.shape == (2,)
    assert tp.voxel_label is pool.voxel_label and tp.stats is pool.stats and tp.shape == (2, 3, True)
