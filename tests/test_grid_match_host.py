"""CPU tests (not gpu) of the segment matching (include/conv3p_match.h: c3p_grid_match_segments, rules M1-M10): the numpy
reference on hand-derived cases whose answers are stated here, not computed; the uniqueness and best-partner property of M8
on every case and on a seeded sweep; the new header against _lib.MATCH_SYMBOLS and the library's exports; the scratch
size; every status code of the C entry in its documented order, none of which launches; every Python argument check, in
order, on CPU tensors; the notes of the new kernels in the code object."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pointwise_amd
from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_match_cases as mc
from tests import grid_match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.int32
ONE = 1 << 30


def ref_of(c, weight="rows", iou=(1, 2), classes=True, max_pairs=None):
    use = classes and c["pred_class"] is not None
    return mr.match_ref(c["segment"], c["S"], c["inverse"], c["emitted"], mc.truth_of(c, weight), c["T"], weight,
                        c["pred_class"] if use else None, c["truth_class"] if use else None, c["num_class"] if use else 1, iou,
                        max_pairs)


# -------------------------------------------------------------------------------------- hand-derived cases, answers stated
def test_halves_an_iou_of_exactly_one_half_is_no_match():
    """An instance of 8 units split 4 / 4 by two segments: both IoUs are 4 / 8, not ABOVE 1 / 2."""
    c = mc.make([0] * 4 + [1] * 4, 2, np.arange(8), [0] * 8, 1)
    o = ref_of(c)
    assert o["pair_inter"][:2].tolist() == [4, 4] and o["stats"][0] == 2
    assert o["best_truth_union"].tolist()[:2] == [8, 8]
    assert o["pred_match"][:2].tolist() == [-1, -1] and o["truth_match"].tolist() == [-1]
    assert o["class_stats"].tolist() == [[0, 2, 1, 0, 1, 2]]                    # TP 0, FP 2, FN 1
    assert o["best_pred"].tolist() == [0]                                       # the lower segment on the tie
    assert o["stats"][8] == ONE // 2 and o["stats"][9] == 8 * (ONE // 2) and o["stats"][10] == 8


def test_five_three_split_the_larger_part_matches():
    """An instance of 8 units split 5 / 3: segment 0 has IoU 5 / 8 = 0.625, floor(0.625 * 2^30) = 671088640."""
    c = mc.make([0] * 5 + [1] * 3, 2, np.arange(8), [0] * 8, 1)
    o = ref_of(c)
    assert o["pred_match"][:2].tolist() == [0, -1] and o["truth_match"].tolist() == [0]
    assert o["pred_iou_q30"][0] == 671088640 and o["pred_iou_q30"][1] == 0
    assert o["class_stats"].tolist() == [[1, 1, 0, 671088640, 1, 2]]
    assert ref_of(c, iou=(3, 4))["pred_match"][:2].tolist() == [-1, -1]         # 5 / 8 is not above 3 / 4
    assert ref_of(c, iou=(5, 8))["pred_match"][:2].tolist() == [-1, -1]         # nor above itself
    assert ref_of(c, iou=(4999, 8000))["pred_match"][0] == 0


@pytest.mark.parametrize("k", [1, 5])
def test_perfect_every_planted_instance_is_its_segment(k):
    seg = np.repeat(np.arange(k), 6)
    c = mc.make(seg, k, np.arange(6 * k), seg, k)
    for weight in ("rows", "voxels"):
        o = ref_of(c, weight)
        assert o["class_stats"].tolist() == [[k, 0, 0, k * ONE, k, k]]
        assert o["stats"][8] == k * ONE and o["stats"][9] == 6 * k * ONE and (o["pred_iou_q30"] == ONE)[:k].all()
        s = mr.summary_ref(o)
        assert s["pq"] == [1.0] and s["mean_pq"] == s["mean_sq"] == s["mean_rq"] == s["mcov"] == s["mwcov"] == 1.0
        assert grid.match_summary(o["class_stats"].tolist(), o["stats"].tolist()) == s


def test_the_void_rule_a_segment_mostly_on_unannotated_ground_is_ignored():
    """Segment 0: 3 void + 3 valid units, unmatched (instance 0 has 20 units): an FP.  Segment 1: 4 void + 3 valid: void >
    size, ignored.  Instance 0 itself is an FN."""
    seg = [0] * 6 + [1] * 7 + [-1] * 14
    tru = [-1] * 3 + [0] * 3 + [-1] * 4 + [0] * 3 + [0] * 14
    o = ref_of(mc.make(seg, 2, np.arange(27), tru, 1))
    assert o["pred_size"][:2].tolist() == [3, 3] and o["pred_void"][:2].tolist() == [3, 4]
    assert o["truth_size"].tolist() == [20] and o["truth_missed"].tolist() == [14]
    assert o["class_stats"].tolist() == [[0, 1, 1, 0, 1, 2]]
    assert o["stats"][:8].tolist() == [2, 6, 2, 1, 7, 0, 14, 0]


def test_classes_a_mismatch_blocks_a_match_an_ignored_class_is_void_an_unknown_id_is_invalid():
    seg = [0] * 6 + [1] * 6 + [2] * 6
    tru = [0] * 6 + [1] * 6 + [2] * 4 + [7, -2]           # 7 and -2 are outside [-1, 3)
    base = dict(segment=seg, S=3, inverse=np.arange(18), truth_rows=tru, T=3)
    o = ref_of(mc.make(pred_class=[0, 1, 1] + [0] * 15, truth_class=[0, 0, 1], num_class=2, **base))
    assert o["pred_match"][:3].tolist() == [0, -1, 2]                           # segment 1 is class 1, instance 1 class 0
    assert o["best_truth"][:3].tolist() == [0, 1, 2]                            # M7 does not look at classes
    assert o["class_stats"].tolist() == [[1, 0, 1, ONE, 2, 1], [1, 1, 0, (4 << 30) // 4, 1, 2]]
    assert o["stats"][4] == 2 and o["stats"][5] == 2                            # two void units, both invalid ids
    o = ref_of(mc.make(pred_class=[0, 1, 1] + [0] * 15, truth_class=[0, 5, 1], num_class=2, **base))
    assert o["truth_size"].tolist() == [6, 0, 4] and o["pred_void"][:3].tolist() == [0, 6, 2]
    assert o["stats"][3] == 2 and o["stats"][4] == 8 and o["stats"][5] == 2     # instance 1 is an ignored category: void
    assert o["class_stats"].tolist() == [[1, 0, 0, ONE, 1, 1], [1, 0, 0, ONE, 1, 2]]      # segment 1: 6 void > 0, ignored
    o = ref_of(mc.make(pred_class=[0, 9, 1] + [0] * 15, truth_class=[0, 0, 1], num_class=2, **base))
    assert o["class_stats"][:, 5].tolist() == [1, 1] and o["class_stats"][:, 1].tolist() == [0, 0]   # class 9: counted nowhere


# --------------------------------------------------------------------------------------------------------- theorem M8
def all_cases():
    yield "ties", mc.ties()
    yield "long rows", mc.long_rows(40)
    yield "one pair", mc.one_pair(100)
    yield "all pairs", mc.all_pairs(100)
    for name in mc.EDGES:
        yield name, mc.edge(name)
    for n in mc.UNIT_COUNTS[:5]:
        yield "planted %d" % n, mc.planted(n, seed=n, classes=n != 64)


def test_a_match_is_unique_mutual_and_the_best_partner_of_both_sides():
    matches = 0
    for name, c in all_cases():
        for weight in ("rows", "voxels"):
            for iou in ((1, 2), (3, 4), (9, 10)):
                for classes in (True, False):
                    matches += mr.check_theorem(ref_of(c, weight, iou, classes))
    rng = np.random.default_rng(5)
    for seed in range(40):                               # few segments against few instances: large overlaps, many matches
        S, T = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        c = mc.planted(int(rng.integers(1, 400)), seed, S=S, T=T, classes=bool(seed & 1), shuffle=bool(seed & 2), scatter=bool(seed & 4))
        matches += mr.check_theorem(ref_of(c, iou=(int(rng.integers(50, 100)), 100)))
    assert matches > 100


def test_overflow_leaves_the_sizes_and_the_bound_exact():
    c = mc.all_pairs(10)
    full, cut = ref_of(c, max_pairs=10), ref_of(c, max_pairs=9)
    assert full["stats"][0] == 10 and cut["stats"][0] == -1 and cut["stats"][7] == 1 and cut["stats"][1] == 10
    for name in ("pred_size", "pred_void", "truth_size", "truth_missed"):
        assert np.array_equal(full[name], cut[name])
    assert (cut["pair_pred"] == -1).all() and (cut["t_pair"] == -1).all() and (cut["start"] == 0).all() and (cut["t_start"] == 0).all()
    assert (cut["best_pred"] == -1).all() and (cut["pred_match"] == -1).all() and (cut["class_stats"] == 0).all()
    assert cut["stats"][8] == cut["stats"][9] == 0 and cut["stats"][10] == full["stats"][10] == 10


# ------------------------------------------------------------------------------------------------- tables and exports
def declared(header, prefix):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
            for m in re.finditer(r"\b(%s\w+)\s*\(([^;{]*)\)\s*;" % prefix, text)}


def test_the_header_the_table_and_the_exports():
    names = {"c3p_grid_match_scratch_bytes": 4, "c3p_grid_match_segments": 39}
    assert declared("conv3p_match.h", "c3p_") == names and set(_lib.MATCH_SYMBOLS) == set(names)
    assert not declared("conv3p_match.h", "conv3p_")
    assert not any(name.startswith("conv3p_") for name in _lib.MATCH_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in names.items():
        assert hasattr(lib, name) and len(_lib.MATCH_SYMBOLS[name][1]) == n, name
    readelf = os.path.join(os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin"), "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    exported = {r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[6] != "UND"}
    assert {n for n in exported if n.startswith("c3p_")} == set(names)
    # the three old tables: still exactly the conv3p_ exports and their headers
    assert {n for n in exported if n.startswith("conv3p_")} == set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS) | set(_lib.KNN_SYMBOLS)
    assert set(declared("conv3p.h", "conv3p_")) == set(_lib.SYMBOLS)
    assert set(declared("conv3p_graph.h", "conv3p_")) == set(_lib.GRAPH_SYMBOLS) and len(_lib.GRAPH_SYMBOLS) == 2
    assert set(declared("conv3p_knn.h", "conv3p_")) == set(_lib.KNN_SYMBOLS) and len(_lib.KNN_SYMBOLS) == 5
    loaded = _lib.load()
    assert loaded.conv3p_abi_version() == _lib.ABI_VERSION == 5
    assert all(getattr(loaded, name).argtypes == _lib.MATCH_SYMBOLS[name][1] for name in names)
    assert loaded.c3p_grid_match_segments.restype is ctypes.c_int and loaded.c3p_grid_match_scratch_bytes.restype is ctypes.c_size_t
    for name in ("SegmentMatch", "match", "match_summary", "MATCH_SYMBOLS"):
        assert name not in pointwise_amd.__all__
    assert callable(pointwise_amd.grid.GridSegments.match) and pointwise_amd.grid.SegmentMatch is grid.SegmentMatch


def test_the_scratch_size_is_a_function_of_its_arguments():
    size = _lib.load().c3p_grid_match_scratch_bytes
    for P in (0, 1, 4095, 4096, 4097, 100000, (1 << 31) - 1):
        n = size(1000, 4000, 50, P)
        assert n == size(1000, 4000, 50, P) and n % 256 == 0
        slots = 2 * P + 64
        assert n >= 12 * slots + 32 * P                  # a key and a count per slot, four key buffers
        assert n <= 12 * slots + 32 * P + 1024 * ((P + 4095) // 4096 + 1) + 2 * 8192 + 12 * 256
        assert n == size(1, 0, 1, P) == size(1 << 24, 1 << 24, 1 << 24, P)      # M, N and T only bound it
    for a in ((0, 1, 1, 1), (-1, 1, 1, 1), ((1 << 24) + 1, 1, 1, 1), (1, -1, 1, 1), (1, (1 << 24) + 1, 1, 1), (1, 1, 0, 1),
              (1, 1, (1 << 24) + 1, 1), (1, 1, 1, -1), (1, 1, 1, 1 << 31)):
        assert size(*a) == 0, a


# ------------------------------------------------------------------------------------------- the C entry's refusals
ARGS = ["segment", "seg_stats", "inverse", "grid_stats", "truth", "M", "N", "T", "weight", "pred_class", "truth_class", "num_class",
        "iou_num", "iou_den", "max_pairs", "pred_size", "pred_void", "truth_size", "truth_missed", "pair_pred", "pair_truth",
        "pair_inter", "start", "t_start", "t_pair", "best_truth", "best_truth_inter", "best_truth_union", "best_pred",
        "best_pred_inter", "best_pred_union", "pred_match", "truth_match", "pred_iou_q30", "class_stats", "stats", "workspace",
        "workspace_bytes", "stream"]
POINTERS = [a for a in ARGS[:5] + ARGS[15:36]]


def test_the_c_entry_refuses_bad_arguments_without_a_launch_in_the_documented_order():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    need = lib.c3p_grid_match_scratch_bytes(8, 16, 4, 8)
    assert need > 0
    ok = [p] * 5 + [8, 16, 4, 1, p, p, 3, 1, 2, 8] + [p] * 21 + [p, need, None]
    assert len(ok) == len(ARGS) == len(_lib.MATCH_SYMBOLS["c3p_grid_match_segments"][1])

    def status(**ch):
        a = list(ok)
        for key, val in ch.items():
            a[ARGS.index(key)] = val
        return lib.c3p_grid_match_segments(*a)

    for ch in ({"M": -1}, {"N": -1}, {"T": 0}, {"T": (1 << 24) + 1}, {"weight": 2}, {"weight": -1}, {"num_class": 0},
               {"num_class": 129}, {"pred_class": None}, {"truth_class": None}, {"pred_class": None, "truth_class": None},
               {"iou_num": 0}, {"iou_num": 2}, {"iou_num": 3}, {"iou_den": 32769, "iou_num": 20000}, {"iou_num": 1, "iou_den": 3},
               {"max_pairs": -1}):
        assert status(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert status(pred_class=None, truth_class=None, num_class=1, workspace_bytes=need - 1) == _lib.ERR_INVALID_ARGUMENT
    # M == 0 comes before the pointers: nothing launched, nothing written
    assert status(M=0) == status(M=0, segment=None, stats=None, workspace=None) == _lib.OK
    for name in POINTERS:
        if name in ("inverse", "grid_stats"):
            continue
        expect = _lib.ERR_INVALID_ARGUMENT
        assert status(**{name: None}) == expect, name
    big = (1 << 24) + 1                                  # a call that passes the pointers is refused as UNSUPPORTED
    assert status(inverse=None) == _lib.ERR_INVALID_ARGUMENT                    # weight = 1 with N > 0 reads inverse
    assert status(weight=0, grid_stats=None) == _lib.ERR_INVALID_ARGUMENT       # weight = 0 reads grid_stats
    assert status(grid_stats=None, M=big) == status(weight=0, inverse=None, M=big) == _lib.ERR_UNSUPPORTED
    assert status(inverse=None, N=0, M=big) == _lib.ERR_UNSUPPORTED
    for ch in ({"M": (1 << 24) + 1}, {"N": (1 << 24) + 1}, {"max_pairs": 1 << 31}):
        assert status(**ch) == _lib.ERR_UNSUPPORTED, ch
    for ch in ({"workspace": None}, {"workspace_bytes": need - 1}, {"workspace_bytes": 0}):
        assert status(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    # the order: a scalar before M == 0, M == 0 before a NULL, a NULL before UNSUPPORTED, that before the workspace
    assert status(T=0, M=0) == _lib.ERR_INVALID_ARGUMENT
    assert status(M=0, stats=None) == _lib.OK
    assert status(stats=None, M=(1 << 24) + 1) == _lib.ERR_INVALID_ARGUMENT
    assert status(M=(1 << 24) + 1, workspace=None) == _lib.ERR_UNSUPPORTED
    # the pair arrays may be NULL with max_pairs == 0, and only then
    free = {"pair_pred": None, "pair_truth": None, "pair_inter": None, "t_pair": None}
    assert status(max_pairs=0, workspace_bytes=0, **free) == _lib.ERR_INVALID_ARGUMENT      # past the pointers: the workspace
    assert status(max_pairs=0, M=(1 << 24) + 1, **free) == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ the Python argument checks
def cpu_objects(N=10, M=4):
    g = grid.GridSubsample(N, M, 3, False, "cpu")
    seg = grid.GridSegments(M, "cpu")
    seg._source = (g, None, 0, None, 26)
    return g, seg


def test_the_checks_pass_up_to_the_device_check():
    g, seg = cpu_objects()
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    for kw in (dict(), dict(weight="rows"), dict(iou=(3, 4)), dict(iou=[9, 10]), dict(max_pairs=0), dict(max_pairs=99),
               dict(pred_class=i32(4), truth_class=i32(5), num_class=13), dict(out=grid.SegmentMatch(4, 5, 4, 1, "cpu")),
               dict(max_pairs=7, pred_class=i32(4), truth_class=i32(5), num_class=2, out=grid.SegmentMatch(4, 5, 7, 2, "cpu"))):
        with pytest.raises(Conv3pError, match="no CPU path"):
            seg.match(i32(10), 5, **kw)
    with pytest.raises(Conv3pError, match="no CPU path"):
        seg.match(i32(4), 5, weight="voxels")


def test_match_refuses_every_bad_argument_in_order():
    g, seg = cpu_objects()
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    cls = dict(pred_class=i32(4), truth_class=i32(5), num_class=3)
    bad = [
        ("weight", dict(weight="points"), "weight must be \"rows\" or \"voxels\""),
        ("weight", dict(weight=1), "weight must be \"rows\" or \"voxels\""),
        ("num_truth", dict(num_truth=0), "num_truth must be an integer from 1 to 2\\^24"),
        ("num_truth", dict(num_truth=(1 << 24) + 1), "num_truth must be an integer from 1 to 2\\^24"),
        ("num_truth", dict(num_truth=5.0), "num_truth must be an integer from 1 to 2\\^24"),
        ("num_truth", dict(num_truth=True), "num_truth must be an integer from 1 to 2\\^24"),
        ("truth", dict(truth=i32(9)), "truth must be a contiguous int32 \\(10,\\) tensor .* per raw row"),
        ("truth", dict(truth=i32(10).long()), "truth must be a contiguous int32"),
        ("truth", dict(truth=i32(20)[::2]), "truth must be a contiguous int32"),
        ("truth", dict(truth=i32(10), weight="voxels"), "truth must be a contiguous int32 \\(4,\\) tensor .* per voxel"),
        ("classes", dict(pred_class=i32(4)), "pred_class, truth_class and num_class go together"),
        ("classes", dict(num_class=3), "pred_class, truth_class and num_class go together"),
        ("classes", dict(pred_class=i32(4), truth_class=i32(5)), "pred_class, truth_class and num_class go together"),
        ("classes", dict(cls, num_class=0), "num_class must be an integer from 1 to 128"),
        ("classes", dict(cls, num_class=129), "num_class must be an integer from 1 to 128"),
        ("classes", dict(cls, pred_class=i32(5)), "pred_class must be a contiguous int32 \\(4,\\)"),
        ("classes", dict(cls, pred_class=i32(4).long()), "pred_class must be a contiguous int32"),
        ("classes", dict(cls, truth_class=i32(4)), "truth_class must be a contiguous int32 \\(5,\\)"),
        ("iou", dict(iou=0.5), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(1, 3)), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(2, 2)), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(0, 1)), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(20000, 32769)), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(1.0, 2)), "iou must be \\(num, den\\)"),
        ("iou", dict(iou=(1, 2, 3)), "iou must be \\(num, den\\)"),
        ("max_pairs", dict(max_pairs=-1), "max_pairs must be a non-negative integer below 2\\^31"),
        ("max_pairs", dict(max_pairs=1 << 31), "max_pairs must be a non-negative integer below 2\\^31"),
        ("max_pairs", dict(max_pairs=4.0), "max_pairs must be a non-negative integer below 2\\^31"),
        ("out", dict(out=grid.SegmentMatch(4, 5, 5, 1, "cpu")), "out was made for another shape"),
        ("out", dict(out=grid.SegmentMatch(4, 6, 4, 1, "cpu")), "out was made for another shape"),
        ("out", dict(cls, out=grid.SegmentMatch(4, 5, 4, 1, "cpu")), "out was made for another shape"),
        ("out", dict(out=i32(4)), "out was made for another shape"),
    ]
    order = ["weight", "num_truth", "truth", "classes", "iou", "max_pairs", "out"]
    worse = {"num_truth": dict(num_truth=-3), "truth": dict(truth=7), "classes": dict(num_class=77), "iou": dict(iou=None),
             "max_pairs": dict(max_pairs="many"), "out": dict(out=7)}
    for what, kw, msg in bad:
        args = dict(truth=i32(10), num_truth=5)
        for name in order[order.index(what) + 1:]:       # every later argument bad too: the earlier message wins
            if not set(worse[name]) & set(kw) and not (name == "classes" and what == "classes"):
                args.update(worse[name])
        args.update(kw)
        with pytest.raises(Conv3pError, match=msg):
            seg.match(args.pop("truth"), args.pop("num_truth"), **args)
    with pytest.raises(Conv3pError, match="match works on the object segments\\(\\), merge\\(\\) or agglomerate\\(\\) returned, not on its trim"):
        grid.GridSegments(4, "cpu").match(i32(10), 5)
    for what, msg in (("inverse", "inverse must be"), ("grid stats", "stats must be"), ("segment", "segment must be"),
                      ("seg stats", "stats must be")):
        g, seg = cpu_objects()
        if what == "inverse": g.inverse = g.inverse.long()
        elif what == "grid stats": g.stats = g.stats.long()
        elif what == "segment": seg.segment = seg.segment.long()
        elif what == "seg stats": seg.stats = torch.zeros(7, dtype=torch.int32)
        with pytest.raises(Conv3pError, match=msg):      # the last check before the device's
            seg.match(i32(10), 5)


def test_summary_is_plain_arithmetic_on_the_counters():
    cs = [[3, 1, 2, 3 * ONE - ONE // 2, 5, 4], [0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 2]]
    st = [9, 9, 6, 5, 0, 0, 0, 0, 4 * ONE, 30 * ONE, 40] + [0] * 5
    s = grid.match_summary(cs, st)
    assert s["tp"] == [3, 0, 0] and s["fp"] == [1, 0, 2] and s["fn"] == [2, 0, 0]
    assert s["sq"] == [2.5 / 3, None, None] and s["rq"] == [6 / 9, None, 0.0] and s["pq"] == [5.0 / 9, None, 0.0]
    assert s["precision"] == [0.75, None, 0.0] and s["recall"] == [0.6, None, None]
    assert s["mean_pq"] == (5.0 / 9 + 0.0) / 2 and s["mean_sq"] == 2.5 / 3 and s["mean_recall"] == 0.6
    assert s["mcov"] == 0.8 and s["mwcov"] == 0.75
    empty = grid.match_summary([[0] * 6], [0] * 16)
    assert empty["mean_pq"] is None and empty["mcov"] is None and empty["pq"] == [None]


# --------------------------------------------------------------------------------------------------- the code object
def test_the_new_kernels_use_no_private_memory():
    names = ("match_init_kernel", "match_walk_kernel", "match_rows_kernel", "match_transpose_kernel", "match_pred_kernel",
             "match_truth_kernel", "match_stats_kernel")
    res = build.kernel_resources()
    mine = [r for r in res if any("conv3p" + str(len(n)) + n in r[0] for n in names)]
    assert len(mine) == len(names), [r[0] for r in mine]
    for name, vgprs, vgpr_spills, _, private in mine:
        assert vgpr_spills == 0 and private == 0 and vgprs <= 256, (name, vgprs, vgpr_spills, private)


# ----------------------------------------------------------------------------------- the planted scene of the model step
def test_on_the_planted_scene_agglomeration_does_not_lower_pq():
    """tests/test_grid_match_model_step.py's second half on the references alone: four boxes, 5 % of the voxel labels
    redrawn (the seed is chosen here), segments by label, agglomerate(min_size=8).  The redrawn voxels are segments of a
    few voxels inside a box of 125: before, each is an FP of its class; after, it has joined the box around it."""
    from tests import grid_adjacency_ref as ga, grid_agglomerate_ref as gg, grid_segments_ref as gs
    neigh, cells = gs.lattice_table(mc.boxes_lattice(4))
    M = cells.shape[0]
    assert M == 500
    labels = mc.redrawn_labels(cells, mc.MODEL_STEP_SEED)
    truth = (cells[:, 0] // 15).astype(I32)
    tcls = (np.arange(4) % 3).astype(I32)
    assert 10 <= int((labels != tcls[truth]).sum()) <= 40
    seg = gs.segments_ref(neigh, labels, M, np.full(M, 8, I32), M, 3, 26)
    adj = ga.adjacency_ref(neigh, seg["segment"], int(seg["stats"][0]), M, 26, 2 * M)
    assert adj["stats"][0] >= 0
    agg = gg.agglomerate_ref(seg, adj, 8)
    pq = []
    for s in (seg, agg):
        o = mr.match_ref(s["segment"], s["stats"][0], np.repeat(np.arange(M, dtype=I32), 8), M, np.repeat(truth, 8), 4, "rows",
                         s["label"], tcls, 3)
        mr.check_theorem(o)
        pq.append(mr.summary_ref(o)["mean_pq"])
        assert o["class_stats"][:, 0].sum() == 4                                # every box is matched, before and after
    assert int(seg["stats"][0]) > int(agg["stats"][0]) == 4 and pq[0] < pq[1] == 1.0
