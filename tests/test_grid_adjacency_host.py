"""CPU tests (not gpu) of the segment adjacency and the merge (include/conv3p.h: conv3p_grid_segment_adjacency, rules E1-E7;
conv3p_grid_merge_segments, rules U1-U5): tests/grid_adjacency_ref.py against cases written out by hand, against a
throw-away loop implementation and against closed forms; its invariants on random fields; the overflow rule; the merge
against the segmentation it must reproduce; every Python argument check of GridSegments.adjacency / merge (each raises
before any device work: the objects here live on the CPU); the C entries' statuses in their order; the new symbols in
_lib's table and the notes of the new kernels' code objects."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_adjacency_ref as ga
from tests import grid_segments_ref as gs

EDGE_KEYS = ("start", "src", "dst", "contacts", "voxels", "offset", "twin", "border", "stats")


def segments(neigh, labels, num_class, connectivity):
    M = neigh.shape[0]
    return gs.segments_ref(neigh, labels, M, np.ones(M, np.int32), M, num_class, connectivity)


def adjacency(neigh, seg, connectivity, max_edges=None, ne=None):
    M = neigh.shape[0]
    return ga.adjacency_ref(neigh, seg["segment"], seg["stats"][0], M if ne is None else ne, connectivity,
                            2 * M if max_edges is None else max_edges)


def against_loops(neigh, seg, connectivity, ne=None):
    """The vectorised reference equals the loops, edge by edge -> it."""
    M = neigh.shape[0]
    r = adjacency(neigh, seg, connectivity, max_edges=26 * M, ne=ne)
    edges, border = ga.adjacency_loops(neigh, seg["segment"], int(seg["stats"][0]), M if ne is None else ne, connectivity)
    E = int(r["stats"][0])
    assert E == len(edges) and r["border"].tolist() == border
    for e, (a, b) in enumerate(sorted(edges)):
        c, vox, off = edges[(a, b)]
        assert (r["src"][e], r["dst"][e], r["contacts"][e], r["voxels"][e]) == (a, b, c, len(vox)) and r["offset"][e].tolist() == off
        assert (r["src"][r["twin"][e]], r["dst"][r["twin"][e]]) == (b, a)
    assert r["stats"][1] == sum(len(v[1]) for v in edges.values()) and r["stats"][3] == sum(v[0] for v in edges.values())
    return r


def checkerboard():
    neigh, cells = gs.lattice_table(np.ones((17, 16, 8), bool))
    return neigh, (cells.sum(axis=1) % 2).astype(np.int32)


def slabs(n=64, h=1):
    """Two slabs n x n x h, the label the slab -> (neigh, labels)."""
    neigh, cells = gs.lattice_table(np.ones((n, n, 2 * h), bool))
    return neigh, (cells[:, 2] >= h).astype(np.int32)


def random_field(seed=5, shape=(24, 24, 24), classes=13):
    neigh, cells = gs.lattice_table(np.ones(shape, bool))
    return neigh, np.random.default_rng(seed).integers(0, classes, cells.shape[0]).astype(np.int32)


# ------------------------------------------------------------------------------------- the reference against hand cases
def test_two_voxels():
    neigh, _ = gs.lattice_table(np.ones((2, 1, 1), bool))
    seg = segments(neigh, np.array([0, 1], np.int32), 2, 6)
    r = against_loops(neigh, seg, 6)
    assert r["src"][:2].tolist() == [0, 1] and r["dst"][:2].tolist() == [1, 0] and r["contacts"][:2].tolist() == [1, 1]
    assert r["voxels"][:2].tolist() == [1, 1] and r["offset"][:2].tolist() == [[1, 0, 0], [-1, 0, 0]]
    assert r["twin"][:2].tolist() == [1, 0] and r["border"].tolist() == [[1, 0, 5, 1], [1, 0, 5, 1]]
    assert r["start"].tolist() == [0, 1, 2] and r["stats"].tolist() == [2, 2, 2, 2, 1, 1, 0, 0]
    assert r["src"][2:].tolist() == [-1] * 50 and r["twin"][2:].tolist() == [-1] * 50 and not r["offset"][2:].any()


def test_the_line_with_unlabelled_voxels():
    neigh, _ = gs.lattice_table(np.ones((6, 1, 1), bool))
    seg = segments(neigh, np.array([1, 1, 0, 1, 5, -1], np.int32), 2, 6)
    assert seg["segment"].tolist() == [0, 0, 1, 2, -1, -1]
    r = against_loops(neigh, seg, 6)
    assert r["stats"][0] == 4 and r["src"][:4].tolist() == [0, 1, 1, 2] and r["dst"][:4].tolist() == [1, 0, 2, 1]
    assert r["border"][:3].tolist() == [[1, 0, 9, 2], [2, 0, 4, 1], [1, 1, 4, 1]]
    assert r["start"].tolist() == [0, 1, 3, 4, 4, 4, 4]
    r = against_loops(neigh, seg, 26)
    assert r["border"][:3, 2].tolist() == [49, 24, 24] and r["stats"][0] == 4
    # a cut at ne = 3: voxel 3 is past the emitted ones and a member of nothing, so segment 2 has no member and no edge
    r = against_loops(neigh, seg, 6, ne=3)
    assert r["stats"].tolist() == [2, 2, 3, 2, 1, 1, 0, 0] and r["border"][:3].tolist() == [[1, 0, 9, 2], [1, 0, 5, 1], [0, 0, 0, 0]]


def test_same_label_segments_touch_at_a_corner():
    occ = np.zeros((2, 2, 2), bool)
    occ[0, 0, 0] = occ[1, 1, 1] = True
    neigh, _ = gs.lattice_table(occ)
    seg = segments(neigh, np.zeros(2, np.int32), 1, 6)
    assert seg["stats"][0] == 2
    assert adjacency(neigh, seg, 6)["stats"][0] == 0 and adjacency(neigh, seg, 18)["stats"][0] == 0
    r = against_loops(neigh, seg, 26)
    assert r["stats"][0] == 2 and r["offset"][:2].tolist() == [[1, 1, 1], [-1, -1, -1]]


# -------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("connectivity,edges", [(6, 11984), (18, 33972), (26, 47412)])
def test_the_checkerboard_segmented_at_six(connectivity, edges):
    neigh, lab = checkerboard()
    seg = segments(neigh, lab, 2, 6)
    assert seg["stats"][0] == 2176
    r = adjacency(neigh, seg, connectivity, max_edges=edges)
    assert r["stats"].tolist() == [edges, edges, 2176, edges, connectivity, 1, 0, 0]
    assert (r["contacts"] == 1).all() and (r["voxels"] == 1).all()


@pytest.mark.parametrize("connectivity,contacts", [(6, 4096), (18, 20224), (26, 36100)])
def test_two_slabs(connectivity, contacts):
    neigh, lab = slabs(64, 1)
    seg = segments(neigh, lab, 2, 26)
    r = adjacency(neigh, seg, connectivity)
    assert r["stats"].tolist() == [2, 8192, 2, 2 * contacts, 1, contacts, 0, 0]
    assert r["contacts"][:2].tolist() == [contacts, contacts] and r["voxels"][:2].tolist() == [4096, 4096]
    assert r["offset"][:2].tolist() == [[0, 0, contacts], [0, 0, -contacts]]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_invariants_on_a_random_field(connectivity):
    neigh, lab = random_field()
    seg = segments(neigh, lab, 13, 26)
    S = int(seg["stats"][0])
    r = adjacency(neigh, seg, connectivity, max_edges=26 * neigh.shape[0])
    E = int(r["stats"][0])
    if connectivity == 26:
        assert (S, E) == (4117, 102438)
    assert E % 2 == 0 and E <= r["stats"][1]
    src, dst, twin = r["src"][:E], r["dst"][:E], r["twin"][:E]
    assert np.array_equal(twin[twin], np.arange(E)) and np.array_equal(src[twin], dst) and np.array_equal(dst[twin], src)
    assert np.array_equal(r["contacts"][:E][twin], r["contacts"][:E]) and np.array_equal(r["offset"][:E][twin], -r["offset"][:E])
    key = src.astype(np.int64) * S + dst
    assert (np.diff(key) > 0).all()                                           # ascending (src, dst): dst ascends in a row
    assert np.array_equal(r["start"][:S + 1], np.searchsorted(src, np.arange(S + 1))) and (r["start"][S:] == E).all()
    assert np.array_equal(r["border"][:S, 0], np.bincount(src, weights=r["contacts"][:E], minlength=S).astype(np.int64))
    assert r["voxels"][:E].sum() == r["stats"][1] and r["contacts"][:E].sum() == r["stats"][3]
    assert not r["border"][S:].any() and (r["border"][:S, 3] <= seg["size"][:S]).all()


def test_overflow():
    neigh, lab = random_field(seed=3, shape=(6, 5, 4), classes=4)
    seg = segments(neigh, lab, 4, 6)
    full = adjacency(neigh, seg, 26, max_edges=26 * neigh.shape[0])
    E = int(full["stats"][0])
    fits = adjacency(neigh, seg, 26, max_edges=E)
    for k in EDGE_KEYS:
        assert np.array_equal(fits[k], full[k][:E] if full[k].shape[0] == 26 * neigh.shape[0] else full[k]), k
    for cap in (E - 1, 0):
        r = adjacency(neigh, seg, 26, max_edges=cap)
        assert r["stats"].tolist() == [-1, full["stats"][1], full["stats"][2], full["stats"][3], 0, 0, 1, 0]
        assert not r["start"].any() and (r["src"] == -1).all() and (r["twin"] == -1).all() and not r["contacts"].any()
        assert np.array_equal(r["border"], full["border"]) and r["src"].shape == (cap,) and r["offset"].shape == (cap, 3)
    assert E <= full["stats"][1] <= 26 * neigh.shape[0]


# --------------------------------------------------------------------------------------------------------------- merge
SEG_KEYS = ("segment", "root", "size", "rows", "label", "stats")


def test_nothing_selected_is_the_identity():
    neigh, lab = random_field(seed=5, shape=(7, 6, 5), classes=3)
    seg = segments(neigh, lab, 3, 18)
    adj = adjacency(neigh, seg, 18)
    S = int(seg["stats"][0])
    for m in (ga.merge_ref(seg, adj["src"], adj["dst"], np.zeros_like(adj["src"])), ga.merge_ref(seg, [], []),
              ga.merge_ref(seg, [-1, S, 3, 0], [0, 0, 3, M_OUT])):                 # filler, out of range, a == b
        for k in SEG_KEYS:
            assert np.array_equal(m[k], seg[k]), k
        assert np.array_equal(m["seg_map"][:S], np.arange(S)) and (m["seg_map"][S:] == -1).all()
        assert m["merge_stats"].tolist() == [S, S, 0, 0]


M_OUT = 1 << 20


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_every_edge_merged_gives_the_geometric_components(connectivity):
    rng = np.random.default_rng(connectivity)
    neigh, cells = gs.lattice_table(rng.random((10, 9, 8)) < 0.45)
    M = neigh.shape[0]
    lab = rng.integers(-1, 4, M).astype(np.int32)                              # -1: unlabelled
    count = rng.integers(1, 9, M).astype(np.int32)
    seg = gs.segments_ref(neigh, lab, M, count, M, 4, connectivity)
    adj = adjacency(neigh, seg, connectivity, max_edges=26 * M)
    m = ga.merge_ref(seg, adj["src"], adj["dst"])
    want = gs.segments_ref(neigh, np.where(lab >= 0, 0, -1).astype(np.int32), M, count, M, 1, connectivity)
    for k in ("segment", "root", "size", "rows"):
        assert np.array_equal(m[k], want[k]), k
    assert m["stats"][0] == want["stats"][0] < seg["stats"][0] and np.array_equal(m["stats"][1:6], want["stats"][1:6])
    # one direction of every edge is enough
    half = ga.merge_ref(seg, adj["src"], adj["dst"], adj["src"] < adj["dst"])
    for k in SEG_KEYS + ("seg_map",):
        assert np.array_equal(half[k], m[k]), k
    assert half["merge_stats"][2] * 2 == m["merge_stats"][2] == adj["stats"][0]


def test_the_label_is_the_largest_members_and_a_tie_goes_to_the_lowest_number():
    neigh, _ = gs.lattice_table(np.ones((7, 1, 1), bool))
    seg = segments(neigh, np.array([2, 0, 0, 1, 1, 1, 3], np.int32), 4, 6)
    assert seg["size"][:4].tolist() == [1, 2, 3, 1]
    m = ga.merge_ref(seg, [0, 1], [1, 2])
    assert m["segment"].tolist() == [0, 0, 0, 0, 0, 0, 1] and m["label"][:2].tolist() == [1, 3] and m["size"][:2].tolist() == [6, 1]
    assert m["root"][:2].tolist() == [0, 6] and m["seg_map"][:4].tolist() == [0, 0, 0, 1] and m["merge_stats"].tolist() == [2, 4, 2, 1]
    m = ga.merge_ref(seg, [3], [0])                                            # sizes 1 and 1: segment 0's label
    assert m["label"][:3].tolist() == [2, 0, 1] and m["seg_map"][:4].tolist() == [0, 1, 2, 0] and m["stats"][0] == 3
    assert m["root"][:3].tolist() == [0, 1, 3]


def test_an_alternating_line_becomes_one_group():
    neigh, _ = gs.lattice_table(np.ones((4096, 1, 1), bool))
    seg = segments(neigh, (np.arange(4096) % 2).astype(np.int32), 2, 6)
    assert seg["stats"][0] == 4096
    adj = adjacency(neigh, seg, 6, max_edges=8190)
    assert adj["stats"].tolist() == [8190, 8190, 4096, 8190, 2, 1, 0, 0]
    m = ga.merge_ref(seg, adj["src"], adj["dst"])
    assert m["stats"].tolist() == [1, 4096, 0, 0, 4096, 4096, 0, 0] and not m["segment"].any() and m["label"][0] == 0
    assert m["merge_stats"].tolist() == [1, 4096, 8190, 1]


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_segments(M=4, merged=False):
    seg = grid.GridSegments(M, "cpu")
    seg._source = (grid.GridSubsample(10, M, 6, False, "cpu"), None, 0, 1, 26)
    seg._merged = merged
    return seg


def pairs(P=3, dtype=torch.int32):
    return torch.zeros(P, dtype=dtype)


def test_the_checks_pass_up_to_the_device_check():
    for kw in ({}, {"connectivity": 6}, {"connectivity": 18}, {"max_edges": 0}, {"max_edges": 2 ** 31 - 1},
               {"out": grid.SegmentAdjacency(4, 8, "cpu")}, {"max_edges": 5, "out": grid.SegmentAdjacency(4, 5, "cpu")}):
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_segments().adjacency(**kw)
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_segments(merged=True).adjacency(**kw)
    for a in ((pairs(), pairs()), (pairs(0), pairs(0)), (pairs(), pairs(), pairs()), (pairs(), pairs(), pairs(dtype=torch.bool)),
              (pairs(), pairs(), None, grid.GridSegments(4, "cpu"))):
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_segments().merge(*a)
    adj = grid.SegmentAdjacency(4, 8, "cpu")
    adj._segments = cpu_segments()
    with pytest.raises(Conv3pError, match="no CPU path"):
        adj.merge()
    with pytest.raises(Conv3pError, match="no CPU path"):
        adj.merge(torch.ones(8, dtype=torch.bool))


@pytest.mark.parametrize("kw,msg", [
    (dict(connectivity=7), "connectivity must be"), (dict(connectivity=26.0), "connectivity must be"),
    (dict(connectivity=True), "connectivity must be"), (dict(connectivity="6"), "connectivity must be"),
    (dict(max_edges=-1), "max_edges must be"), (dict(max_edges=2 ** 31), "max_edges must be"),
    (dict(max_edges=8.0), "max_edges must be"), (dict(max_edges=True), "max_edges must be"),
    (dict(out=torch.zeros(4, dtype=torch.int32)), "out was made"), (dict(out=grid.SegmentAdjacency(5, 8, "cpu")), "out was made"),
    (dict(out=grid.SegmentAdjacency(4, 9, "cpu")), "out was made"),
    (dict(max_edges=9, out=grid.SegmentAdjacency(4, 8, "cpu")), "out was made"),
])
def test_adjacency_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_segments().adjacency(**kw)


@pytest.mark.parametrize("args,msg", [
    ((pairs(dtype=torch.int64), pairs()), "pair_a must be"), ((np.zeros(3, np.int32), pairs()), "pair_a must be"),
    ((torch.zeros((3, 1), dtype=torch.int32), pairs()), "pair_a must be"), ((pairs(6)[::2], pairs()), "pair_a must be"),
    ((pairs(), pairs(4)), "pair_b must be"), ((pairs(), pairs(dtype=torch.int64)), "pair_b must be"),
    ((pairs(), pairs(6)[::2]), "pair_b must be"), ((pairs(), None), "pair_b must be"),
    ((pairs(), pairs(), pairs(4)), "select must be"), ((pairs(), pairs(), pairs(dtype=torch.int64)), "select must be"),
    ((pairs(), pairs(), [1, 0, 1]), "select must be"), ((pairs(), pairs(), pairs(6)[::2]), "select must be"),
    ((pairs(), pairs(), None, grid.GridSegments(5, "cpu")), "out was made"),
    ((pairs(), pairs(), None, torch.zeros(4, dtype=torch.int32)), "out was made"),
])
def test_merge_refuses_before_any_device_work(args, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_segments().merge(*args)


def test_the_objects_they_work_on():
    seg = cpu_segments()
    with pytest.raises(Conv3pError, match="out was made"):
        seg.merge(pairs(), pairs(), None, seg)                                  # not into itself
    seg.stats[0] = 2
    t = seg.trim()
    for call in (lambda: t.adjacency(), lambda: t.merge(pairs(), pairs()), lambda: grid.GridSegments(4, "cpu").adjacency()):
        with pytest.raises(Conv3pError, match="not on its trim"):
            call()
    with pytest.raises(Conv3pError, match="absorb works on what segments\\(\\) returned"):
        cpu_segments(merged=True).absorb(2)
    with pytest.raises(Conv3pError, match="no CPU path"):
        cpu_segments().absorb(2)                                               # as before
    merged = cpu_segments(merged=True)                   # trim() carries what merge() added, and only then
    merged.seg_map, merged.merge_stats = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    merged.stats[0] = 3
    cut = merged.trim()
    assert cut.seg_map is merged.seg_map and cut.merge_stats is merged.merge_stats and cut._merged and cut.label.shape == (3,)
    assert "seg_map" not in vars(t) and t.seg_map is None and not t._merged
    with pytest.raises(Conv3pError, match="adjacency\\(\\) returned"):
        grid.SegmentAdjacency(4, 8, "cpu").merge()
    adj = grid.SegmentAdjacency(4, 8, "cpu")
    adj.stats[:] = torch.tensor([6, 7, 3, 9, 2, 2, 0, 0])
    assert (adj.num_edges(), adj.edges_bound(), adj.overflowed()) == (6, 7, False)
    t = adj.trim()
    assert t.src.shape == (6,) and t.offset.shape == (6, 3) and t.shape == (4, 6) and t.start is adj.start and t.stats is adj.stats
    assert t.src.data_ptr() == adj.src.data_ptr() and t.border is adj.border
    adj.stats[:] = torch.tensor([-1, 7, 3, 9, 0, 0, 1, 0])
    assert (adj.num_edges(), adj.overflowed()) == (-1, True) and adj.trim().src.shape == (0,)
    assert grid.SegmentAdjacency is __import__("pointwise_amd").SegmentAdjacency


# -------------------------------------------------------------------------------------------------------- the C entries
ADJ_NAMES = ["neigh", "segment", "seg_stats", "grid_stats", "M", "connectivity", "max_edges", "adj_start", "edge_src", "edge_dst",
             "edge_contacts", "edge_voxels", "edge_offset", "edge_twin", "seg_border", "adj_stats", "workspace", "workspace_bytes",
             "stream"]
MERGE_NAMES = ["segment", "seg_root", "seg_size", "seg_rows", "seg_label", "seg_stats", "pair_a", "pair_b", "select", "P", "M",
               "seg_map", "segment_out", "root_out", "size_out", "rows_out", "label_out", "stats_out", "merge_stats", "workspace",
               "workspace_bytes", "stream"]
EDGE_ARRAYS = ("edge_src", "edge_dst", "edge_contacts", "edge_voxels", "edge_offset", "edge_twin")


def test_the_new_symbols_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in (("conv3p_grid_adjacency_scratch_bytes", 2), ("conv3p_grid_segment_adjacency", len(ADJ_NAMES)),
                    ("conv3p_grid_merge_scratch_bytes", 1), ("conv3p_grid_merge_segments", len(MERGE_NAMES))):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n
    assert len(ADJ_NAMES) == 19 and len(MERGE_NAMES) == 22
    sig = _lib.SYMBOLS["conv3p_grid_segment_adjacency"][1]
    assert sig[ADJ_NAMES.index("M")] is ctypes.c_int64 and sig[ADJ_NAMES.index("max_edges")] is ctypes.c_int64
    sig = _lib.SYMBOLS["conv3p_grid_merge_segments"][1]
    assert sig[MERGE_NAMES.index("M")] is ctypes.c_int64 and sig[MERGE_NAMES.index("P")] is ctypes.c_int64
    assert _lib.load().conv3p_abi_version() == 5


def test_the_workspaces_are_functions_of_their_arguments_alone():
    lib = _lib.load()
    adj, mrg = lib.conv3p_grid_adjacency_scratch_bytes, lib.conv3p_grid_merge_scratch_bytes
    for bad in ((0, 8), (-1, 8), (1 << 31, 8), (4, -1), (4, 1 << 31)):
        assert adj(*bad) == 0
    assert mrg(0) == 0 and mrg(-1) == 0 and mrg(1 << 31) == 0
    for M in (1, 2048, 2049, 1 << 20, (1 << 22) + 5):
        assert 4 * 5 * M <= mrg(M) <= 4 * 5 * M + 8 * M // 2048 + 4096 and mrg(M) % 256 == 0
        for E in (0, 1, 4096, 4097, 2 * M, 26 * M):
            b = adj(M, E)
            # 18 words a row of max_edges -- a table of 2 E + 64 slots of 7 words, two 64-bit sort buffers -- a histogram
            # of 256 words per 4096 edges and a few KiB: nothing per voxel, no record per contact
            assert b == adj(1, E) and b % 256 == 0
            assert 72 * E <= b <= 72 * E + 1024 * (E // 4096 + 1) + 16384, (M, E, b)
    assert adj(1 << 22, 2 << 22) < (1 << 22) * 26 * 8                          # far below a record per contact


def test_the_c_entries_refuse_bad_arguments_in_their_order():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    big = 1 << 40
    adj_ok = [p, p, p, p, 4, 26, 8, p, p, p, p, p, p, p, p, p, p, big, None]
    merge_ok = [p, p, p, p, p, p, p, p, p, 3, 4, p, p, p, p, p, p, p, p, p, big, None]

    def caller(f, names, ok_args):
        def call(**ch):
            a = list(ok_args)
            for key, val in ch.items():
                a[names.index(key)] = val
            return f(*a)
        return call

    call = caller(lib.conv3p_grid_segment_adjacency, ADJ_NAMES, adj_ok)
    need = lib.conv3p_grid_adjacency_scratch_bytes(4, 8)
    bad = [{"M": -1}, {"connectivity": 0}, {"connectivity": 7}, {"connectivity": 27}, {"max_edges": -1}, {"workspace": None},
           {"workspace_bytes": need - 1}, {"workspace_bytes": 0}]
    bad += [{n: None} for n in ADJ_NAMES if n not in ("M", "connectivity", "max_edges", "workspace", "workspace_bytes", "stream")]
    for ch in bad:
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31) == _lib.ERR_UNSUPPORTED and call(max_edges=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(M=1 << 31, neigh=None) == _lib.ERR_INVALID_ARGUMENT            # the pointers come before the limits
    assert call(M=1 << 31, workspace=None) == _lib.ERR_UNSUPPORTED             # and the limits before the workspace
    assert call(M=0) == _lib.OK and call(M=0, connectivity=5) == _lib.ERR_INVALID_ARGUMENT
    assert call(M=0, max_edges=-1) == _lib.ERR_INVALID_ARGUMENT
    nulls = [None if a == p else a for a in adj_ok]
    nulls[ADJ_NAMES.index("M")] = nulls[ADJ_NAMES.index("workspace_bytes")] = 0
    assert lib.conv3p_grid_segment_adjacency(*nulls) == _lib.OK
    # the edge arrays may be NULL with max_edges == 0 alone: the next refusal is the workspace's
    no_edges = {n: None for n in EDGE_ARRAYS}
    assert call(max_edges=0, workspace=None, **no_edges) == _lib.ERR_INVALID_ARGUMENT
    assert call(max_edges=0, M=1 << 31, **no_edges) == _lib.ERR_UNSUPPORTED
    assert call(max_edges=1, M=1 << 31, **no_edges) == _lib.ERR_INVALID_ARGUMENT

    call = caller(lib.conv3p_grid_merge_segments, MERGE_NAMES, merge_ok)
    need = lib.conv3p_grid_merge_scratch_bytes(4)
    bad = [{"M": -1}, {"P": -1}, {"workspace": None}, {"workspace_bytes": need - 1}, {"workspace_bytes": 0}]
    bad += [{n: None} for n in MERGE_NAMES if n not in ("select", "P", "M", "workspace", "workspace_bytes", "stream")]
    for ch in bad:
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31) == _lib.ERR_UNSUPPORTED and call(P=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(M=1 << 31, seg_map=None) == _lib.ERR_INVALID_ARGUMENT and call(M=1 << 31, workspace=None) == _lib.ERR_UNSUPPORTED
    assert call(M=0) == _lib.OK and call(M=0, P=-1) == _lib.ERR_INVALID_ARGUMENT
    nulls = [None if a == p else a for a in merge_ok]
    nulls[MERGE_NAMES.index("M")] = nulls[MERGE_NAMES.index("workspace_bytes")] = 0
    assert lib.conv3p_grid_merge_segments(*nulls) == _lib.OK
    # the pairs may be NULL with P == 0 alone, select always: the next refusal is the limit's
    assert call(P=0, pair_a=None, pair_b=None, select=None, M=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(select=None, M=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(P=1, pair_a=None, M=1 << 31) == _lib.ERR_INVALID_ARGUMENT


def test_the_code_objects_have_no_spill_and_no_private_segment():
    names = ("adj_init_kernel", "adj_walk_kernel", "adj_compact_kernel", "adj_sort_hist_kernel", "adj_sort_scan_kernel",
             "adj_sort_scatter_kernel", "adj_finish_kernel", "adj_stats_kernel", "merge_init_kernel", "merge_union_kernel",
             "merge_number_kernel", "merge_assign_kernel", "merge_finish_kernel")
    res = [r for r in build.kernel_resources() if any("conv3p" + str(len(n)) + n in r[0] for n in names)]
    assert len(res) == len(names)
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
