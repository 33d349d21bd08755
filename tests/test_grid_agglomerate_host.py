"""CPU tests (not gpu) of the agglomeration (include/conv3p_graph.h: conv3p_grid_agglomerate_segments, rules H1-H10):
tests/grid_agglomerate_ref.py against cases written out by hand; its two restatements against each other on random
fields; the identities of H6, H7, H8 and H10; the unusable input of H1; every Python argument check of
SegmentAdjacency.agglomerate (each raises before any device work: the objects here live on the CPU); the C entry's statuses
in their order; the scratch size; the new header against _lib.GRAPH_SYMBOLS and the library's exports; the notes of the new
kernels' code objects; and pointwise_amd.__all__, which the feature leaves alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pointwise_amd
from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_adjacency_ref as ga
from tests import grid_agglomerate_ref as ar
from tests import grid_segments_ref as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def field(occ_or_shape, labels, num_class, made_at, connectivity, max_edges=None, count=None):
    """-> (neigh, seg, adj) of the references on a lattice; labels an array or a function of the cells."""
    occ = np.ones(occ_or_shape, bool) if isinstance(occ_or_shape, tuple) else occ_or_shape
    neigh, cells = gs.lattice_table(occ)
    M = neigh.shape[0]
    lab = labels(cells) if callable(labels) else np.asarray(labels, np.int32)
    seg = gs.segments_ref(neigh, lab, M, np.ones(M, np.int32) if count is None else count, M, num_class, made_at)
    adj = ga.adjacency_ref(neigh, seg["segment"], seg["stats"][0], M, connectivity, 26 * M if max_edges is None else max_edges)
    return neigh, seg, adj


def both(neigh, seg, adj, connectivity, **kw):
    """The two restatements agree on every output word -> it."""
    a = ar.agglomerate_ref(seg, adj, **kw)
    b = ar.agglomerate_slow(neigh, seg, neigh.shape[0], connectivity, adj["src"].shape[0], **kw)
    for k in ar.ALL_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    return a


def log_rows(r):
    P = int(r["agg_stats"][3])
    assert (r["log_a"][P:] == -1).all() and (r["log_b"][P:] == -1).all() and (r["log_round"][P:] == -1).all()
    assert not r["log_contacts"][P:].any()
    return [tuple(int(r[k][i]) for k in ar.LOG_KEYS) for i in range(P)]


# ------------------------------------------------------------------------------------- the reference against hand cases
def test_two_voxels():
    neigh, seg, adj = field((2, 1, 1), [0, 1], 2, 6, 6)
    r = both(neigh, seg, adj, 6, min_size=2)
    assert log_rows(r) == [(0, 1, 0, 1)]                                       # a mutual pair, logged by the lower root
    assert r["agg_stats"].tolist() == [1, 2, 1, 1, 0, 0, 0, 0] and r["merge_stats"].tolist() == [1, 2, 1, 1]
    assert r["segment"].tolist() == [0, 0] and r["size"].tolist() == [2, 0] and r["voxel_label"].tolist() == [0, 0]
    assert r["start"].tolist() == [0, 0, 0] and (r["src"] == -1).all()
    r = both(neigh, seg, adj, 6, min_size=1)                                    # nothing is small
    assert log_rows(r) == [] and r["agg_stats"].tolist() == [2, 2, 0, 0, 0, 0, 0, 2] and r["voxel_label"].tolist() == [0, 1]


def test_a_small_piece_prefers_the_large_neighbour_over_a_small_one_with_more_contacts():
    # x ->   y = 0:  L L X T      L: 4 voxels, X: 1, T: 3.  X touches L once and T twice; T touches L once and X twice
    #        y = 1:  L L T T
    lab = {(0, 0): 0, (0, 1): 0, (1, 0): 0, (1, 1): 0, (2, 0): 1, (2, 1): 2, (3, 0): 2, (3, 1): 2}
    neigh, seg, adj = field((4, 2, 1), lambda cells: np.array([lab[(x, y)] for x, y, _ in cells], np.int32), 3, 6, 6)
    assert seg["size"][:3].tolist() == [4, 1, 3] and adj["contacts"][:6].tolist() == [1, 1, 1, 2, 1, 2]
    r = both(neigh, seg, adj, 6, min_size=4)
    assert log_rows(r) == [(1, 0, 0, 1), (2, 0, 0, 1)]                         # both into L, although they touch each other more
    assert r["agg_stats"].tolist() == [1, 3, 1, 2, 0, 0, 0, 0] and r["label"][0] == 0
    r = both(neigh, seg, adj, 6, min_size=2)                                    # T is not small now: X goes by the contacts
    assert log_rows(r) == [(1, 2, 0, 2)] and r["size"][:2].tolist() == [4, 4] and r["contacts"][:2].tolist() == [2, 2]
    r = both(neigh, seg, adj, 6, min_size=5)                                    # everything small: X and T are mutual
    assert log_rows(r) == [(0, 1, 0, 1), (1, 2, 0, 2)]                          # L -> X by the lowest number on a tie of 1 : 1


def test_a_mutual_pair_is_logged_once():
    neigh, seg, adj = field((3, 1, 1), [0, 1, 2], 3, 6, 6)
    r = both(neigh, seg, adj, 6, min_size=2)
    # 0 -> 1, 1 -> 0 (a tie of 0 and 2, the lowest number), 2 -> 1
    assert log_rows(r) == [(0, 1, 0, 1), (2, 1, 0, 1)] and r["agg_stats"].tolist() == [1, 3, 1, 2, 0, 0, 0, 0]
    assert r["seg_map"].tolist() == [0, 0, 0] and r["label"][0] == 0 and r["merge_stats"].tolist() == [1, 3, 2, 1]


def test_min_contacts_needs_two_rounds():
    # y = 0:  X A A     X touches A and B by one contact each, A and B touch by two
    # y = 1:  B B B
    lab = {(0, 0): 0, (1, 0): 2, (2, 0): 2, (0, 1): 1, (1, 1): 1, (2, 1): 1}
    neigh, seg, adj = field((3, 2, 1), lambda cells: np.array([lab[(x, y)] for x, y, _ in cells], np.int32), 3, 6, 6)
    assert seg["size"][:3].tolist() == [1, 3, 2]
    r = both(neigh, seg, adj, 6, min_size=100, min_contacts=2)
    assert log_rows(r) == [(1, 2, 0, 2), (0, 1, 1, 2)]                         # A-B first, then X against contacts 1 + 1
    assert r["agg_stats"].tolist() == [1, 3, 2, 2, 1, 0, 0, 0]                 # one small group is left, with no neighbour
    one = both(neigh, seg, adj, 6, min_size=100, min_contacts=2, max_rounds=1)
    assert log_rows(one) == [(1, 2, 0, 2)] and one["agg_stats"].tolist() == [2, 3, 1, 1, 2, 2, 0, 2]
    assert one["contacts"][:2].tolist() == [2, 2] and one["offset"][:2].tolist() == [[1, 1, 0], [-1, -1, 0]]
    assert log_rows(both(neigh, seg, adj, 6, min_size=100, min_contacts=3)) == []


def test_same_label():
    occ = np.zeros((2, 2, 2), bool)
    occ[0, 0, 0] = occ[1, 0, 0] = occ[1, 1, 1] = True    # 0 and 2 share a label and touch at a corner; 1 touches both
    neigh, seg, adj = field(occ, [0, 1, 0], 2, 6, 26)
    assert seg["stats"][0] == 3 and adj["stats"][0] == 6
    r = both(neigh, seg, adj, 26, min_size=2, same_label=1)
    assert log_rows(r) == [(0, 2, 0, 1)] and r["agg_stats"].tolist() == [2, 3, 1, 1, 1, 0, 0, 2] and r["label"][:2].tolist() == [0, 1]
    assert both(neigh, seg, adj, 26, min_size=2)["agg_stats"][0] == 1
    # on a plain segmentation with the connectivity it was made with, neighbours never share a label
    for c in (6, 26):
        neigh, seg, adj = field((8, 8, 8), ar.random_classes, 13, c, c)
        r = both(neigh, seg, adj, c, min_size=8, same_label=1)
        assert r["agg_stats"][2:4].tolist() == [0, 0] and r["agg_stats"][5] == 0 and r["agg_stats"][0] == seg["stats"][0]


def test_rows_against_voxels():
    count = np.array([1, 1, 9, 1, 1, 1], np.int32)
    neigh, seg, adj = field((6, 1, 1), [0, 0, 1, 2, 2, 2], 3, 6, 6, count=count)
    assert seg["size"][:3].tolist() == [2, 1, 3] and seg["rows"][:3].tolist() == [2, 9, 3]
    v = both(neigh, seg, adj, 6, min_size=3)
    assert log_rows(v) == [(0, 1, 0, 1), (1, 2, 0, 1)]                         # 0 and 1 are small in voxels: 1 goes to the large 2
    r = both(neigh, seg, adj, 6, min_size=3, weight=1)
    assert log_rows(r) == [(0, 1, 0, 1)] and r["rows"][:2].tolist() == [11, 3] and r["size"][:2].tolist() == [3, 3]
    assert r["label"][0] == 0                            # H2: the label goes by seg_size whatever the weight


# ------------------------------------------------------------------------------------------------ the two restatements
CASES = [((12, 12, 12), "classes", 6, c, dict(min_size=ms, min_contacts=mc)) for c in (6, 18, 26) for ms, mc in ((2, 1), (8, 1), (16, 3))]
CASES += [((12, 12, 12), "classes", 6, 26, dict(min_size=8, same_label=1)), ((12, 12, 12), "classes", 26, 26, dict(min_size=5, weight=1)),
          ((24, 24, 6), "slabs", 26, 26, dict(min_size=8)), ((24, 24, 6), "slabs", 18, 6, dict(min_size=16, min_contacts=3)),
          ((24, 24, 6), "slabs", 6, 26, dict(min_size=4, max_rounds=1))]


@pytest.mark.parametrize("shape,kind,made_at,connectivity,kw", CASES)
def test_the_two_references_agree_and_the_identities_hold(shape, kind, made_at, connectivity, kw):
    labels = ar.random_classes if kind == "classes" else ar.redrawn_slabs
    M = int(np.prod(shape))
    count = np.random.default_rng(2).integers(1, 5, M).astype(np.int32)
    neigh, seg, adj = field(shape, labels, 13, made_at, connectivity, count=count)
    r = both(neigh, seg, adj, connectivity, **kw)
    S, G, P = int(seg["stats"][0]), int(r["stats"][0]), int(r["agg_stats"][3])
    assert P == S - G                                                          # H6: a spanning forest
    rows = log_rows(r)
    assert rows == sorted(rows, key=lambda x: (x[2], x[0])) and len({(x[2], x[0]) for x in rows}) == P
    m = ga.merge_ref(seg, r["log_a"], r["log_b"])                              # H7
    for k in ar.SEG_KEYS:
        assert np.array_equal(m[k], r[k]), k
    assert r["merge_stats"].tolist()[:3] == [G, S, P]
    g = ga.adjacency_ref(neigh, r["segment"], G, M, connectivity, adj["src"].shape[0])      # H8
    for k in ar.GRAPH_KEYS:
        assert np.array_equal(g[k], r[k]), k
    assert r["agg_stats"][7] == g["stats"][0]
    for k in range(1, int(r["agg_stats"][2]) + 1):                              # H10: a cut of the log
        cut = ar.agglomerate_ref(seg, adj, **{**kw, "max_rounds": k})
        want = ga.merge_ref(seg, r["log_a"], r["log_b"], r["log_round"] < k)
        for key in ("seg_map", "segment", "root", "size", "rows", "label", "stats"):
            assert np.array_equal(cut[key], want[key]), (k, key)
        n = int((r["log_round"][:P] < k).sum())
        assert all(np.array_equal(cut[key][:n], r[key][:n]) for key in ar.LOG_KEYS) and cut["agg_stats"][3] == n


def test_nothing_small_is_the_identity():
    neigh, seg, adj = field((9, 8, 7), ar.random_classes, 13, 6, 18)
    r = both(neigh, seg, adj, 18, min_size=1)
    S = int(seg["stats"][0])
    for k in ("segment", "root", "size", "rows", "label", "stats"):
        assert np.array_equal(r[k], seg[k]), k
    assert np.array_equal(r["seg_map"][:S], np.arange(S)) and r["merge_stats"].tolist() == [S, S, 0, 0]
    for k in ar.GRAPH_KEYS:
        assert np.array_equal(r[k], adj[k]), k
    assert r["agg_stats"].tolist() == [S, S, 0, 0, 0, 0, 0, adj["stats"][0]]


def test_an_overflowed_adjacency_is_unusable():
    neigh, seg, full = field((6, 5, 4), lambda cells: ar.random_classes(cells, 3, 4), 4, 6, 26)
    E, S, M = int(full["stats"][0]), int(seg["stats"][0]), neigh.shape[0]
    for cap in (E - 1, 0):
        adj = ga.adjacency_ref(neigh, seg["segment"], S, M, 26, cap)
        assert adj["stats"][0] == -1
        r = ar.agglomerate_ref(seg, adj, min_size=8)
        for k in ("segment", "root", "size", "rows", "label", "stats"):
            assert np.array_equal(r[k], seg[k]), k
        small = int((seg["size"][:S] < 8).sum())
        assert r["agg_stats"].tolist() == [S, S, 0, 0, small, 0, 1, 0] and log_rows(r) == []
        assert not r["start"].any() and (r["src"] == -1).all() and (r["twin"] == -1).all() and r["src"].shape == (cap,)
    adj = dict(full, stats=full["stats"].copy())
    adj["stats"][0] = 26 * M + 1                                               # E past max_edges: unusable too
    assert ar.agglomerate_ref(seg, adj, min_size=8)["agg_stats"][6] == 1


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_adjacency(M=4, E=8, merged=False):
    seg = grid.GridSegments(M, "cpu")
    seg._source = (grid.GridSubsample(10, M, 6, False, "cpu"), None, 0, 1, 26)
    seg._merged = merged
    adj = grid.SegmentAdjacency(M, E, "cpu")
    adj._segments, adj.connectivity = seg, 26
    return adj


def test_the_checks_pass_up_to_the_device_check():
    for kw in ({}, {"weight": "rows"}, {"same_label": True}, {"min_contacts": 3}, {"max_rounds": 1}, {"max_rounds": 32},
               {"min_size": 2 ** 31 - 1}, {"out": grid.SegmentAgglomeration(4, 8, "cpu")}):
        kw = {"min_size": 8, **kw}
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_adjacency().agglomerate(**kw)
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_adjacency(merged=True).agglomerate(**kw)
    adj = cpu_adjacency()
    adj.stats[:] = torch.tensor([6, 7, 3, 9, 2, 2, 0, 0])
    t = adj.trim()
    assert t.shape == (4, 6)
    with pytest.raises(Conv3pError, match="no CPU path"):
        t.agglomerate(8)                                                        # its trim() too
    with pytest.raises(Conv3pError, match="no CPU path"):
        t.agglomerate(8, out=grid.SegmentAgglomeration(4, 6, "cpu"))


@pytest.mark.parametrize("kw,msg", [
    (dict(min_size=0), "min_size must be"), (dict(min_size=2 ** 31), "min_size must be"), (dict(min_size=8.0), "min_size must be"),
    (dict(min_size=True), "min_size must be"), (dict(weight="points"), "weight must be"), (dict(weight=0), "weight must be"),
    (dict(same_label=1), "same_label must be"), (dict(same_label=None), "same_label must be"),
    (dict(min_contacts=0), "min_contacts must be"), (dict(min_contacts=1.0), "min_contacts must be"),
    (dict(min_contacts=True), "min_contacts must be"), (dict(max_rounds=0), "max_rounds must be"),
    (dict(max_rounds=33), "max_rounds must be"), (dict(max_rounds=8.0), "max_rounds must be"),
    (dict(out=torch.zeros(4, dtype=torch.int32)), "out was made"), (dict(out=grid.SegmentAgglomeration(5, 8, "cpu")), "out was made"),
    (dict(out=grid.SegmentAgglomeration(4, 9, "cpu")), "out was made"), (dict(out=grid.SegmentAdjacency(4, 8, "cpu")), "out was made"),
])
def test_agglomerate_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_adjacency().agglomerate(**{"min_size": 8, **kw})


def test_the_objects_it_works_on():
    with pytest.raises(Conv3pError, match="adjacency\\(\\) returned"):
        grid.SegmentAdjacency(4, 8, "cpu").agglomerate(8)
    adj = cpu_adjacency()
    adj._segments = adj._segments.trim()                 # a trimmed segmentation has no source
    with pytest.raises(Conv3pError, match="adjacency\\(\\) returned"):
        adj.agglomerate(8)
    adj = cpu_adjacency()
    adj.src = adj.src[:7]
    with pytest.raises(Conv3pError, match="src must be"):
        adj.agglomerate(8)
    adj = cpu_adjacency()
    adj.stats = adj.stats.to(torch.int32)
    with pytest.raises(Conv3pError, match="stats must be"):
        adj.agglomerate(8)
    adj = cpu_adjacency()
    out = grid.SegmentAgglomeration(4, 8, "cpu")
    out.segments = adj._segments                         # not into the segmentation it reads
    with pytest.raises(Conv3pError, match="out was made"):
        adj.agglomerate(8, out=out)
    # the result object: a merged GridSegments, the host reads, trim()
    res = grid.SegmentAgglomeration(4, 8, "cpu")
    assert res.segments._merged and res.segments.seg_map.shape == (4,) and res.segments.merge_stats.shape == (4,)
    assert res.log_a.shape == res.voxel_label.shape == (4,) and res.start.shape == (5,) and res.offset.shape == (8, 3)
    res.stats[:] = torch.tensor([2, 4, 3, 2, 1, 0, 0, 6])
    assert (res.num_groups(), res.num_rounds(), res.converged()) == (2, 3, True)
    t = res.trim()
    assert t.log_a.shape == (2,) and t.src.shape == (6,) and t.offset.shape == (6, 3) and t.shape == (4, 6)
    assert t.segments is res.segments and t.stats is res.stats and t.start is res.start and t.log_b.data_ptr() == res.log_b.data_ptr()
    res.stats[5] = 1
    assert not res.converged()
    res.stats[5:7] = torch.tensor([0, 1])
    assert not res.converged()


# --------------------------------------------------------------------------------------------------------- the C entry
NAMES = ["segment", "seg_root", "seg_size", "seg_rows", "seg_label", "seg_stats", "adj_start", "edge_src", "edge_dst",
         "edge_contacts", "edge_offset", "adj_stats", "M", "max_edges", "min_size", "weight", "same_label", "min_contacts",
         "max_rounds", "log_a", "log_b", "log_round", "log_contacts", "seg_map", "segment_out", "root_out", "size_out",
         "rows_out", "label_out", "stats_out", "merge_stats", "voxel_label", "start_out", "src_out", "dst_out", "contacts_out",
         "offset_out", "twin_out", "agg_stats", "workspace", "workspace_bytes", "stream"]
EDGE_ARRAYS = ("edge_src", "edge_dst", "edge_contacts", "edge_offset", "src_out", "dst_out", "contacts_out", "offset_out", "twin_out")
INTEGERS = ("M", "max_edges", "min_size", "weight", "same_label", "min_contacts", "max_rounds", "workspace_bytes", "stream")


def declared(header):
    """The functions a header declares: name -> the number of parameters."""
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
            for m in re.finditer(r"\b(conv3p_\w+)\s*\(([^;{]*)\)\s*;", text)}


def test_the_header_the_table_and_the_exports():
    graph = declared("conv3p_graph.h")
    assert set(graph) == {"conv3p_grid_agglomerate_scratch_bytes", "conv3p_grid_agglomerate_segments"} == set(_lib.GRAPH_SYMBOLS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in graph.items():
        assert hasattr(lib, name) and len(_lib.GRAPH_SYMBOLS[name][1]) == n, name
    assert graph["conv3p_grid_agglomerate_segments"] == len(NAMES) == 42
    sig = _lib.GRAPH_SYMBOLS["conv3p_grid_agglomerate_segments"][1]
    assert sig[NAMES.index("M")] is ctypes.c_int64 and sig[NAMES.index("max_edges")] is ctypes.c_int64
    assert sig[NAMES.index("workspace_bytes")] is ctypes.c_size_t
    assert all(sig[NAMES.index(n)] is ctypes.c_int for n in INTEGERS[2:7])
    assert set(declared("conv3p.h")) == set(_lib.SYMBOLS) and not set(_lib.SYMBOLS) & set(graph)       # SYMBOLS is conv3p.h's still
    loaded = _lib.load()
    assert loaded.conv3p_grid_agglomerate_segments.argtypes == sig and loaded.conv3p_abi_version() == 5


def test_pointwise_amd_all_is_unchanged():
    assert "SegmentAgglomeration" not in pointwise_amd.__all__ and not any("gglomerat" in n for n in pointwise_amd.__all__)
    assert grid.SegmentAgglomeration.__module__ == "pointwise_amd.grid" and hasattr(grid.SegmentAdjacency, "agglomerate")


def test_the_scratch_is_a_function_of_its_arguments_alone():
    lib = _lib.load()
    agg, adj, mrg = lib.conv3p_grid_agglomerate_scratch_bytes, lib.conv3p_grid_adjacency_scratch_bytes, lib.conv3p_grid_merge_scratch_bytes
    for bad in ((0, 8), (-1, 8), (1 << 31, 8), (4, -1), (4, 1 << 31)):
        assert agg(*bad) == 0
    for M in (1, 2048, 2049, 1 << 20, (1 << 22) + 5):
        for E in (0, 1, 4096, 4097, 2 * M, 26 * M):
            b = agg(M, E)
            # the adjacency's and the merge's as they stand, a word per edge row, 6 M words of group state, a word per
            # 2048 segments and the header; every array rounded up to 256 bytes
            own = 4 * E + 24 * M + 4 * (M // 2048 + 1)
            assert b % 256 == 0 and b == agg(M, E) and adj(M, E) + mrg(M) + own <= b <= adj(M, E) + mrg(M) + own + 8 * 256, (M, E, b)


def test_the_c_entry_refuses_bad_arguments_in_its_order():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    ok = [0 if n in INTEGERS else p for n in NAMES]
    for n, v in (("M", 4), ("max_edges", 8), ("min_size", 8), ("weight", 0), ("same_label", 0), ("min_contacts", 1), ("max_rounds", 8),
                 ("workspace_bytes", 1 << 40), ("stream", None)):
        ok[NAMES.index(n)] = v

    def call(**ch):
        a = list(ok)
        for key, val in ch.items():
            a[NAMES.index(key)] = val
        return lib.conv3p_grid_agglomerate_segments(*a)

    need = lib.conv3p_grid_agglomerate_scratch_bytes(4, 8)
    bad = [{"M": -1}, {"max_edges": -1}, {"min_size": 0}, {"min_size": -3}, {"weight": 2}, {"weight": -1}, {"same_label": 2},
           {"same_label": -1}, {"min_contacts": 0}, {"max_rounds": 0}, {"max_rounds": 33}, {"workspace": None},
           {"workspace_bytes": need - 1}, {"workspace_bytes": 0}]
    bad += [{n: None} for n in NAMES if n not in INTEGERS and n != "workspace"]
    for ch in bad:
        assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
    assert call(M=1 << 31) == _lib.ERR_UNSUPPORTED and call(max_edges=1 << 31) == _lib.ERR_UNSUPPORTED
    assert call(M=1 << 31, seg_map=None) == _lib.ERR_INVALID_ARGUMENT          # the pointers come before the limits
    assert call(M=1 << 31, workspace=None) == _lib.ERR_UNSUPPORTED             # and the limits before the workspace
    assert call(M=0) == _lib.OK                                                 # nothing launched ...
    for ch in ({"min_size": 0}, {"max_rounds": 33}, {"weight": 2}, {"max_edges": -1}):
        assert call(M=0, **ch) == _lib.ERR_INVALID_ARGUMENT, ch                 # ... but the integers come first
    nulls = [None if a == p else a for a in ok]
    nulls[NAMES.index("M")] = nulls[NAMES.index("workspace_bytes")] = 0
    assert lib.conv3p_grid_agglomerate_segments(*nulls) == _lib.OK
    # the edge arrays, in and out, may be NULL with max_edges == 0 alone: the next refusal is the limit's or the workspace's
    no_edges = {n: None for n in EDGE_ARRAYS}
    assert call(max_edges=0, workspace=None, **no_edges) == _lib.ERR_INVALID_ARGUMENT
    assert call(max_edges=0, M=1 << 31, **no_edges) == _lib.ERR_UNSUPPORTED
    assert call(max_edges=1, M=1 << 31, **no_edges) == _lib.ERR_INVALID_ARGUMENT
    for n in EDGE_ARRAYS:
        assert call(max_edges=1, M=1 << 31, **{n: None}) == _lib.ERR_INVALID_ARGUMENT, n


def test_the_code_objects_have_no_spill_and_no_private_segment():
    names = ("agg_init_kernel", "agg_contract_kernel", "agg_choose_kernel", "agg_count_kernel", "agg_scan_kernel", "agg_log_kernel",
             "agg_flatten_kernel", "agg_census_kernel", "agg_finish_kernel")
    res = [r for r in build.kernel_resources() if any("conv3p" + str(len(n)) + n in r[0] for n in names)]
    assert len(res) == len(names)
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
