"""CPU tests (not gpu) of the k-nearest-voxel search (include/conv3p_knn.h: conv3p_grid_knn_f32, rules K1-K8, and its two
consumers): theorem K7 by brute force on every case of tests/grid_knn_cases.py over the whole parameter sweep; the scan
counts that follow from the geometry of a lattice of centres; the new header against _lib.KNN_SYMBOLS and the library's
exports; the scratch size; the C entries' refusals, none of which launches; every Python argument check, in order, on CPU
tensors; the notes of the new kernels in the code object."""
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
from tests import grid_knn_cases as kc
from tests import grid_knn_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# --------------------------------------------------------------------------------------------------------- theorem K7
@pytest.mark.parametrize("name", kc.NAMES)
def test_the_cube_of_scanned_gives_the_cube_of_rings_and_a_certified_set_is_the_rooms(name):
    c = kc.build(name)
    sub = kc.subsample_ref(c)
    nv, M = int(sub["stats"][0]), sub["data"].shape[0]
    certified = live = 0
    for voxel_queries in (True, False):
        q, qv = (sub["data"], None) if voxel_queries else (c["data"], sub["inverse"])
        for exclude_self in (False, True):
            for valid in (None, c["valid"](sub["voxel_cell"], nv, M)):
                s = kr.Search(q, qv, sub["data"], sub["voxel_cell"], nv, c["voxel"], exclude_self, valid, sub["voxel_room"],
                              sub["voxel_start"])
                for k in kc.KS:
                    for rings in kc.RINGS:
                        ref = kr.knn_ref(None, None, None, None, None, None, k, rings, search=s)
                        a, b = kr.check_theorem(ref, k, rings)
                        certified, live = certified + a, live + b
                        assert ref["stats"][:4].sum() == s.Q and ref["stats"][6:15].sum() == ref["stats"][0] + ref["stats"][1]
    assert live > 0 and (certified > 0 or name == "corner")          # the corner's three voxels never make k = 1 .. 16 certain


@pytest.mark.parametrize("what", ["displaced", "voxel / 3", "voxel * 3"])
def test_displaced_representatives_and_a_wrong_step_only_make_the_search_scan_further(what):
    """The stop test measures where the representatives lie: it stays conservative when they have left their cells by up
    to 1.5 voxels, and with a step that is not the lattice's."""
    c = kc.build("lattice")
    sub = kc.subsample_ref(c)
    nv = int(sub["stats"][0])
    vd = kc.displaced(sub["data"], c["voxel"], 7) if what == "displaced" else sub["data"]
    voxel = c["voxel"] * {"displaced": 1.0, "voxel / 3": 1 / 3, "voxel * 3": 3.0}[what]
    base = kr.knn_ref(c["data"], sub["inverse"], sub["data"], sub["voxel_cell"], nv, c["voxel"], 8, 8)
    s = kr.Search(c["data"], sub["inverse"], vd, sub["voxel_cell"], nv, voxel)
    for k in kc.KS:
        for rings in kc.RINGS:
            kr.check_theorem(kr.knn_ref(None, None, None, None, None, None, k, rings, search=s), k, rings)
    ref = kr.knn_ref(None, None, None, None, None, None, 8, 8, search=s)
    if what != "voxel / 3":                              # a step too small makes L_r small against the true spread: nothing stops
        assert ref["scanned"].sum() > base["scanned"].sum()
    else:
        assert ref["certified"].sum() == 0 and (ref["scanned"][s.live] == 8).all()


def test_scan_counts_on_a_lattice_of_centres_follow_from_the_geometry():
    """centres(6), mode center, voxel h = 0.25: every representative is its cell's centre and the rows are those centres
    and the origin, so S = h / 2 and L_r = (r + 1/2) h.  With k = 8 an interior row keeps itself, six face neighbours at h^2
    and one edge neighbour at 2 h^2 < 2.25 h^2 (1 - 2^-20): STOP(1).  A corner row's eighth is the cube's far corner at
    3 h^2: STOP(2), 3 h^2 < 6.25 h^2.  No row at a centre scans past ring 2.  The origin row, the one that makes S = h / 2,
    is the one exception: from the lattice's corner its eighth neighbour is the centre of cell (1, 1, 1) at 6.75 h^2, which
    is not below 6.25 h^2, so it stops at ring 3 (6.75 h^2 < 12.25 h^2)."""
    c = kc.build("centres")
    sub = kc.subsample_ref(c)
    nv = int(sub["stats"][0])
    assert nv == 216
    ref = kr.knn_ref(c["data"], sub["inverse"], sub["data"], sub["voxel_cell"], nv, c["voxel"], k=8, rings=8)
    assert ref["search"].S_room.tolist() == [0.125]
    cell = sub["voxel_cell"][sub["inverse"]]
    at_centre = np.arange(c["data"].shape[0]) > 0        # row 0 is the origin
    interior = at_centre & ((cell >= 1) & (cell <= 4)).all(axis=1)
    corner = at_centre & ((cell == 0) | (cell == 5)).all(axis=1)
    assert interior.sum() == 64 and corner.sum() == 8
    h2 = F(0.25) * F(0.25)
    assert (ref["d2"][interior, 7] == 2 * h2).all() and (ref["scanned"][interior] == 1).all()
    assert (ref["d2"][corner, 7] == 3 * h2).all() and (ref["scanned"][corner] == 2).all()
    assert ref["scanned"][at_centre].max() == 2
    assert ref["d2"][0, 7] == F(6.75) * h2 and ref["scanned"][0] == 3
    assert (ref["count"] == 8).all() and (ref["certified"] == 1).all()
    # exact ties: the six face neighbours of an interior row come in ascending voxel number
    assert (np.diff(ref["index"][interior, 1:7], axis=1) > 0).all() and (ref["d2"][interior, 1:7] == h2).all()


# ------------------------------------------------------------------------------------------------- tables and exports
def declared(header):
    """The functions a header declares: name -> the number of parameters."""
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
            for m in re.finditer(r"\b(conv3p_\w+)\s*\(([^;{]*)\)\s*;", text)}


KNN_NAMES = {"conv3p_grid_knn_scratch_bytes", "conv3p_grid_knn_f32", "conv3p_grid_interpolate_knn_f32",
             "conv3p_grid_interpolate_knn_i64", "conv3p_grid_normals_knn_f32"}


def test_the_header_the_table_and_the_exports():
    knn = declared("conv3p_knn.h")
    assert set(knn) == KNN_NAMES == set(_lib.KNN_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in knn.items():
        assert hasattr(lib, name) and len(_lib.KNN_SYMBOLS[name][1]) == n, name
    assert _lib.KNN_SYMBOLS["conv3p_grid_interpolate_knn_f32"] == _lib.KNN_SYMBOLS["conv3p_grid_interpolate_knn_i64"]
    assert not set(_lib.KNN_SYMBOLS) & set(_lib.SYMBOLS) and not set(_lib.KNN_SYMBOLS) & set(_lib.GRAPH_SYMBOLS)
    assert set(declared("conv3p.h")) == set(_lib.SYMBOLS) and set(declared("conv3p_graph.h")) == set(_lib.GRAPH_SYMBOLS)
    assert not any(name.endswith("_workspace_bytes") for name in knn)
    readelf = os.path.join(os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin"), "llvm-readelf")      # build.kernel_resources' tool
    out = subprocess.run([readelf, "--dyn-syms", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    exported = {r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[6] != "UND" and r[7].startswith("conv3p_")}
    assert exported == set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS) | set(_lib.KNN_SYMBOLS)
    loaded = _lib.load()
    assert loaded.conv3p_abi_version() == _lib.ABI_VERSION == 5
    assert all(getattr(loaded, name).argtypes == _lib.KNN_SYMBOLS[name][1] for name in knn)
    for name in ("GridKnn", "knn", "grid_knn", "KNN_SYMBOLS"):
        assert name not in pointwise_amd.__all__
    assert grid.GridKnn is pointwise_amd.grid.GridKnn and callable(pointwise_amd.grid.GridSubsample.knn)
    assert grid.GridRoomSubsample.knn is grid.GridSubsample.knn


def test_the_scratch_size_is_a_function_of_its_arguments():
    size = _lib.load().conv3p_grid_knn_scratch_bytes
    for Q in (0, 1, 63, 64, 1000, 1 << 20, (1 << 31) - 1):
        for rooms in (0, 1, 2, 1000, 65536):
            n = size(Q, rooms)
            assert n == size(Q, rooms) and n % 256 == 0
            assert n >= 256 + max(rooms, 1) * 13 * 8 + 4 * Q          # a counter, 12 extremes and an S per room, an int32 per query
            assert n <= 4 * 256 + max(rooms, 1) * 13 * 8 + 4 * Q
    assert size(10, 0) == size(10, 1) < size(10, 40) < size(1000, 40)
    for Q, rooms in ((-1, 0), (1 << 31, 0), (0, -1), (0, 65537), (-5, -5)):
        assert size(Q, rooms) == 0


# ------------------------------------------------------------------------------------------- the C entries' refusals
KNN_ARGS = ["query", "Q", "query_stride", "query_voxel", "voxel_data", "voxel_K", "neigh", "cell", "room", "start", "num_rooms",
            "grid_stats", "M", "valid", "voxel", "k", "rings", "exclude_self", "index", "d2", "count", "ring", "scanned",
            "certified", "stats", "scratch", "scratch_bytes", "stream"]


def test_the_c_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    ok = [p, 4, 6, p, p, 6, p, p, None, None, 0, p, 8, None, 0.1, 8, 2, 0, p, p, p, p, p, p, p, p, 1 << 20, None]
    assert len(ok) == len(KNN_ARGS) == len(_lib.KNN_SYMBOLS["conv3p_grid_knn_f32"][1])

    def status(**ch):
        a = list(ok)
        for key, val in ch.items():
            a[KNN_ARGS.index(key)] = val
        return lib.conv3p_grid_knn_f32(*a)

    need = lib.conv3p_grid_knn_scratch_bytes(4, 0)
    for ch in ({"Q": -1}, {"M": -1}, {"query_stride": 2}, {"voxel_K": 2}, {"k": 0}, {"k": 17}, {"rings": 0}, {"rings": 9},
               {"exclude_self": 2}, {"exclude_self": -1}, {"num_rooms": -1}, {"voxel": 0.0}, {"voxel": -0.1},
               {"voxel": float("nan")}, {"voxel": float("inf")}, {"room": p}, {"start": p}, {"stats": None}, {"query": None},
               {"index": None}, {"d2": None}, {"count": None}, {"ring": None}, {"scanned": None}, {"certified": None},
               {"voxel_data": None}, {"neigh": None}, {"cell": None}, {"grid_stats": None},
               {"query_voxel": None, "Q": 9, "scratch_bytes": 1 << 20}, {"scratch": None}, {"scratch_bytes": need - 1}):
        assert status(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    for ch in ({"Q": 1 << 31}, {"M": 1 << 31}, {"room": p, "start": p, "num_rooms": 65537}):
        assert status(**ch) == _lib.ERR_UNSUPPORTED, ch
    # the order: a range before the rooms, the rooms before a NULL, a NULL before UNSUPPORTED, that before the scratch
    assert status(k=0, room=p) == status(room=p, stats=None) == status(stats=None, M=1 << 31) == _lib.ERR_INVALID_ARGUMENT
    assert status(M=1 << 31, scratch=None) == _lib.ERR_UNSUPPORTED
    for fn in (lib.conv3p_grid_interpolate_knn_f32, lib.conv3p_grid_interpolate_knn_i64):
        good = [p, p, p, 4, 8, 3, p, 8, 13, p, None, p, None]
        assert len(good) == len(_lib.KNN_SYMBOLS["conv3p_grid_interpolate_knn_f32"][1])
        for at, val in ((3, -1), (7, -1), (4, 0), (4, 17), (5, 0), (5, 9), (8, 0), (8, 129), (11, None), (0, None), (1, None),
                        (2, None), (9, None), (6, None)):
            a = list(good)
            a[at] = val
            assert fn(*a) == _lib.ERR_INVALID_ARGUMENT, (at, val)
        for at in (3, 7):
            a = list(good)
            a[at] = 1 << 31
            assert fn(*a) == _lib.ERR_UNSUPPORTED, at
    good = [p, 6, p, p, 8, p, None, None, 0, 8, 6, p, p, p, p, None, p, None]
    assert len(good) == len(_lib.KNN_SYMBOLS["conv3p_grid_normals_knn_f32"][1])
    for at, val in ((9, -1), (1, 2), (4, 0), (4, 17), (10, 2), (10, 17), (0, None), (2, None), (3, None), (5, None), (11, None),
                    (12, None), (13, None), (14, None), (16, None)):
        a = list(good)
        a[at] = val
        assert lib.conv3p_grid_normals_knn_f32(*a) == _lib.ERR_INVALID_ARGUMENT, (at, val)
    a = list(good)
    a[7], a[8] = p, 0                                    # a viewpoint with V < 1
    assert lib.conv3p_grid_normals_knn_f32(*a) == _lib.ERR_INVALID_ARGUMENT
    a[8] = 2                                             # one per room without voxel_room
    assert lib.conv3p_grid_normals_knn_f32(*a) == _lib.ERR_INVALID_ARGUMENT
    a = list(good)
    a[9] = 0                                             # M == 0: nothing launched, nothing written
    assert lib.conv3p_grid_normals_knn_f32(*a) == _lib.OK
    a[9] = 1 << 31
    assert lib.conv3p_grid_normals_knn_f32(*a) == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ the Python argument checks
def cpu_object(N=10, M=4, K=6, rooms=False):
    g = grid.GridRoomSubsample(N, 2, M, K, False, "cpu") if rooms else grid.GridSubsample(N, M, K, False, "cpu")
    return g, torch.zeros((N, K))


def test_the_checks_pass_up_to_the_device_check():
    for rooms in (False, True):
        g, data = cpu_object(rooms=rooms)
        valid = torch.zeros(4, dtype=torch.int32)
        for step in (np.float32(0.1), np.float64(0.1), 1):       # a step computed in numpy is a number too
            with pytest.raises(Conv3pError, match="no CPU path"):
                g.knn(step)
        for kw in (dict(), dict(k=1, rings=1), dict(k=16, rings=8, exclude_self=True), dict(points=data), dict(valid_labels=valid),
                   dict(points=data, query_voxel=torch.zeros(10, dtype=torch.int32)), dict(out=grid.GridKnn(4, 8, "cpu")),
                   dict(points=data[:7], query_voxel=torch.zeros(7, dtype=torch.int32), k=3, out=grid.GridKnn(7, 3, "cpu"))):
            with pytest.raises(Conv3pError, match="no CPU path"):
                g.knn(0.1, **kw)
    t = grid.GridKnn(4, 8, "cpu")
    t.grid, t.voxel_queries = cpu_object()[0], True
    lab = torch.zeros(4, dtype=torch.int32)
    for kw in (dict(), dict(k=1), dict(k=8, return_scores=True), dict(out=lab), dict(return_scores=True, out=(lab, torch.zeros((4, 13))))):
        with pytest.raises(Conv3pError, match="no CPU path"):
            t.interpolate(torch.zeros((4, 13)), **kw)
    for kw in (dict(), dict(min_neighbors=3), dict(min_neighbors=16, return_moments=True), dict(viewpoint=(0.0, 1.0, 2.0)),
               dict(out=grid.GridNormals(4, False, "cpu"))):
        with pytest.raises(Conv3pError, match="no CPU path"):
            t.normals(**kw)


def _ordered(calls):
    """calls: (what, a function that must raise, the message).  Each is given ONE bad argument behind good ones, and the
    list is in the order of the checks: a call with this bad argument and every later one raises this message."""
    for what, fn, msg in calls:
        with pytest.raises(Conv3pError, match=msg):
            fn()


def test_knn_refuses_every_bad_argument_in_order():
    g, data = cpu_object()
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    bad = [
        ("voxel", dict(voxel=0.0), "voxel must be finite and positive"),
        ("voxel", dict(voxel=float("nan")), "voxel must be finite and positive"),
        ("voxel", dict(voxel=True), "voxel must be finite and positive"),
        ("voxel", dict(voxel="0.1"), "voxel must be finite and positive"),
        ("query_voxel", dict(query_voxel=i32(4)), "query_voxel needs points"),
        ("points", dict(points=torch.zeros((10, 2))), "points must be a float32"),
        ("points", dict(points=torch.zeros((10, 6), dtype=torch.float64)), "points must be a float32"),
        ("points", dict(points=torch.zeros((10, 12))[:, ::2]), "points must be contiguous"),
        ("query_voxel", dict(points=data, query_voxel=i32(9)), "query_voxel must be a contiguous int32"),
        ("query_voxel", dict(points=data, query_voxel=i32(10).long()), "query_voxel must be a contiguous int32"),
        ("query_voxel", dict(points=data[:7]), "query_voxel must be a contiguous int32"),      # the default, inverse, has 10 rows
        ("k", dict(k=0), "k must be an integer in \\[1, 16\\]"),
        ("k", dict(k=17), "k must be an integer in \\[1, 16\\]"),
        ("k", dict(k=8.0), "k must be an integer in \\[1, 16\\]"),
        ("k", dict(k=True), "k must be an integer in \\[1, 16\\]"),
        ("rings", dict(rings=0), "rings must be an integer in \\[1, 8\\]"),
        ("rings", dict(rings=9), "rings must be an integer in \\[1, 8\\]"),
        ("rings", dict(rings=None), "rings must be an integer in \\[1, 8\\]"),
        ("exclude_self", dict(exclude_self=1), "exclude_self must be a bool"),
        ("valid_labels", dict(valid_labels=i32(5)), "valid_labels must be a contiguous int32"),
        ("valid_labels", dict(valid_labels=torch.zeros(4)), "valid_labels must be a contiguous int32"),
        ("out", dict(out=grid.GridKnn(4, 7, "cpu")), "out was made for another shape"),
        ("out", dict(out=grid.GridKnn(5, 8, "cpu")), "out was made for another shape"),
        ("out", dict(out=i32(4)), "out was made for another shape"),
    ]
    order = ["voxel", "points", "query_voxel", "k", "rings", "exclude_self", "valid_labels", "out", "table"]
    worse = {"voxel": dict(voxel=-1.0), "points": dict(points=torch.zeros(3)), "k": dict(k=99), "rings": dict(rings=99),
             "exclude_self": dict(exclude_self="no"), "valid_labels": dict(valid_labels=3), "out": dict(out=7)}
    for what, kw, msg in bad:
        later = {}
        for name in order[order.index(what) + 1:]:       # every later argument bad too: the earlier message wins
            if name in worse and not set(worse[name]) & set(kw) and not (name == "points" and "query_voxel" in kw):
                later.update(worse[name])
        args = dict(voxel=0.1)
        args.update(later)
        args.update(kw)
        with pytest.raises(Conv3pError, match=msg):
            g.knn(args.pop("voxel"), **args)
    for what, msg in (("cell dtype", "voxel_cell must be"), ("cell shape", "voxel_cell must be"), ("stats dtype", "stats must be"),
                      ("room dtype", "voxel_room must be"), ("start dtype", "voxel_start must be")):
        g, data = cpu_object(rooms=what.startswith(("room", "start")))
        if what == "cell dtype": g.voxel_cell = g.voxel_cell.long()
        elif what == "cell shape": g.voxel_cell = torch.zeros((3, 3), dtype=torch.int32)
        elif what == "stats dtype": g.stats = g.stats.long()
        elif what == "room dtype": g.voxel_room = g.voxel_room.long()
        elif what == "start dtype": g.voxel_start = g.voxel_start.long()
        with pytest.raises(Conv3pError, match=msg):      # the last check before the device's
            g.knn(0.1)


def test_the_consumers_refuse_every_bad_argument_in_order():
    g, _ = cpu_object()
    t = grid.GridKnn(4, 8, "cpu")
    t.grid, t.voxel_queries = g, True
    scores, lab = torch.zeros((4, 13)), torch.zeros(4, dtype=torch.int32)
    _ordered([
        ("k", lambda: t.interpolate(torch.zeros(3), k=0), "k must be an integer in \\[1, 8\\], the table's width"),
        ("k", lambda: t.interpolate(scores, k=9), "k must be an integer in \\[1, 8\\]"),
        ("k", lambda: t.interpolate(scores, k=2.0), "k must be an integer in \\[1, 8\\]"),
        ("scores", lambda: t.interpolate(torch.zeros(3), out=(lab,), return_scores=True), "voxel_scores must be"),
        ("scores", lambda: t.interpolate(scores.double()), "voxel_scores must be"),
        ("scores", lambda: t.interpolate(torch.zeros((4, 26))[:, ::2]), "voxel_scores must be"),
        ("classes", lambda: t.interpolate(torch.zeros((4, 129)), out=(lab,), return_scores=True), "at most 128 classes"),
        ("classes", lambda: t.interpolate(torch.zeros((4, 0))), "at most 128 classes"),
        ("out", lambda: t.interpolate(scores, return_scores=True, out=lab), "out must be \\(labels, scores\\)"),
        ("out", lambda: t.interpolate(scores, return_scores=True, out=(lab, scores, lab)), "out must be \\(labels, scores\\)"),
        ("out labels", lambda: t.interpolate(scores, out=lab.long()), "out labels must be"),
        ("out labels", lambda: t.interpolate(scores, out=torch.zeros(5, dtype=torch.int32)), "out labels must be"),
        ("out scores", lambda: t.interpolate(scores, return_scores=True, out=(lab, torch.zeros((4, 12)))), "out scores must be"),
    ])
    rows = grid.GridKnn(10, 8, "cpu")
    rows.grid, rows.voxel_queries = g, False
    other = grid.GridKnn(5, 8, "cpu")
    other.grid, other.voxel_queries = g, True
    _ordered([
        ("table", lambda: grid.GridKnn(4, 8, "cpu").normals(min_neighbors=0), "normals need the table of voxel queries"),
        ("table", lambda: rows.normals(min_neighbors=0), "normals need the table of voxel queries"),
        ("table", lambda: other.normals(min_neighbors=0), "the table was made for another subsampling"),
        ("min_neighbors", lambda: t.normals(min_neighbors=2, return_moments=1), "min_neighbors must be an integer in \\[3, 16\\]"),
        ("min_neighbors", lambda: t.normals(min_neighbors=17), "min_neighbors must be an integer in \\[3, 16\\]"),
        ("return_moments", lambda: t.normals(return_moments=1, viewpoint=(1, 2)), "return_moments must be a bool"),
        ("viewpoint", lambda: t.normals(viewpoint=(1, 2), out=3), "viewpoint must be"),
        ("viewpoint", lambda: t.normals(viewpoint=(1, 2, float("inf"))), "viewpoint must be"),
        ("viewpoint", lambda: t.normals(viewpoint=torch.zeros((2, 3))), "a viewpoint per room needs a GridRoomSubsample"),
        ("out", lambda: t.normals(out=grid.GridNormals(4, True, "cpu")), "out was made for another shape"),
        ("out", lambda: t.normals(out=3), "out was made for another shape"),
    ])


# --------------------------------------------------------------------------------------------------- the code object
def test_the_new_kernels_keep_their_lists_in_registers():
    names = ("grid_knn_spread_kernel", "grid_knn_bound_kernel", "grid_knn_near_kernel", "grid_knn_ring_kernel",
             "grid_knn_normals_kernel")
    res = build.kernel_resources()
    mine = [r for r in res if any("conv3p" + str(len(n)) + n in r[0] for n in names)]
    assert len(mine) == len(names), [r[0] for r in mine]
    mine += [r for r in res if "grid_knn_interpolate_kernelI" in r[0]]
    assert len(mine) == len(names) + 2                   # float32 scores and the int64 sums
    for name, vgprs, vgpr_spills, _, private in mine:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
