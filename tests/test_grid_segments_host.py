"""CPU tests (not gpu) of the connected segments and the clean-up of small ones: tests/grid_segments_ref.py against cases
written out by hand and against scipy.ndimage.label, the absorb by hand and on a noisy field of four quadrants, every
Python argument check of GridSubsample.segments / clean_labels / GridSegments.absorb (each raises before any device work:
the objects here live on the CPU), the C entries' statuses, the new symbols in _lib's table and the notes of the new
kernels' code objects."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, build, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_segments_ref as gs


def table(cells):
    """Occupied cells, in any order -> (neigh, the cells in voxel order) on the lattice that just holds them."""
    cells = np.asarray(cells)
    occ = np.zeros(tuple(cells.max(axis=0) + 1), dtype=bool)
    occ[tuple(cells.T)] = True
    return gs.lattice_table(occ)


def run(neigh, labels, num_class, connectivity, count=None, ne=None, L=None):
    M = neigh.shape[0]
    return gs.segments_ref(neigh, labels, M if L is None else L, np.ones(M, np.int32) if count is None else count,
                           M if ne is None else ne, num_class, connectivity)


def quadrant_field(seed=11):
    """A 16 x 16 x 8 lattice of four quadrant classes, 5 % of the voxels redrawn -> (neigh, clean, noisy)."""
    neigh, cells = gs.lattice_table(np.ones((16, 16, 8), bool))
    clean = ((cells[:, 0] >= 8) * 2 + (cells[:, 1] >= 8)).astype(np.int32)
    rng = np.random.default_rng(seed)
    noisy = clean.copy()
    hit = rng.choice(clean.size, clean.size // 20, replace=False)
    noisy[hit] = rng.integers(0, 4, hit.size)
    return neigh, clean, noisy


# ------------------------------------------------------------------------------------- the reference against hand cases
def test_an_l_of_three_voxels_and_two_diagonal_pairs():
    neigh, cells = table([(0, 0, 0), (1, 0, 0), (1, 1, 0)])
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0]]
    for c in (6, 18, 26):
        r = run(neigh, None, None, c, count=np.array([2, 3, 5], np.int32))
        assert r["segment"].tolist() == [0, 0, 0] and r["root"].tolist() == [0, -1, -1]
        assert r["size"].tolist() == [3, 0, 0] and r["rows"].tolist() == [10, 0, 0] and r["label"].tolist() == [0, -1, -1]
        assert r["stats"].tolist() == [1, 3, 0, 0, 3, 10, 0, 0]
    edge, _ = table([(0, 0, 0), (1, 1, 0)])              # share an edge: joined at 18 and 26
    corner, _ = table([(0, 0, 0), (1, 1, 1)])            # share a corner: joined at 26 alone
    assert [int(run(edge, None, None, c)["stats"][0]) for c in (6, 18, 26)] == [2, 1, 1]
    assert [int(run(corner, None, None, c)["stats"][0]) for c in (6, 18, 26)] == [2, 2, 1]
    assert run(corner, None, None, 18)["segment"].tolist() == [0, 1] and run(corner, None, None, 18)["root"].tolist() == [0, 1]
    assert [len(gs.taps(c)) for c in (6, 18, 26)] == [6, 18, 26] and 13 not in gs.taps(26)


def test_labels_split_what_the_cells_join_and_unlabelled_voxels_are_in_no_segment():
    neigh, _ = gs.lattice_table(np.ones((6, 1, 1), bool))
    lab = np.array([1, 1, 0, 1, 5, -1], np.int32)        # 5 >= num_class, -1: unlabelled
    r = run(neigh, lab, 2, 6)
    assert r["segment"].tolist() == [0, 0, 1, 2, -1, -1] and r["root"].tolist() == [0, 2, 3, -1, -1, -1]
    assert r["label"].tolist() == [1, 0, 1, -1, -1, -1] and r["size"].tolist() == [2, 1, 1, 0, 0, 0]
    assert r["stats"].tolist() == [3, 4, 2, 0, 2, 2, 0, 0]
    # L = 3 label words, ne = 5 emitted voxels of 6 rows
    r = run(neigh, lab, 2, 6, ne=5, L=3)
    assert r["segment"].tolist() == [0, 0, 1, -1, -1, -1] and r["stats"].tolist() == [2, 3, 2, 1, 2, 2, 0, 0]
    # a cut: the voxel past ne joins nothing, even where the table names it
    r = run(neigh, None, None, 6, ne=2)
    assert r["segment"].tolist() == [0, 0, -1, -1, -1, -1] and r["stats"].tolist() == [1, 2, 0, 4, 2, 2, 0, 0]


def test_the_checkerboard():
    neigh, cells = gs.lattice_table(np.ones((4, 4, 4), bool))
    lab = (cells.sum(axis=1) % 2).astype(np.int32)
    r6, r18, r26 = (run(neigh, lab, 2, c) for c in (6, 18, 26))
    assert r6["stats"][0] == 64 and np.array_equal(r6["segment"], np.arange(64)) and (r6["size"] == 1).all()
    for r in (r18, r26):                                 # face diagonals keep the colour: one segment per colour
        assert r["stats"][0] == 2 and np.array_equal(r["segment"], lab) and r["size"][:2].tolist() == [32, 32]
        assert r["root"][:2].tolist() == [0, 1] and r["label"][:2].tolist() == [0, 1]


@pytest.mark.parametrize("connectivity,rank", [(6, 1), (18, 2), (26, 3)])
def test_one_class_has_the_numbering_of_scipy(connectivity, rank):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(connectivity)
    for fill in (0.25, 0.5):
        occ = rng.random((14, 13, 12)) < fill
        neigh, cells = gs.lattice_table(occ)
        r = run(neigh, None, None, connectivity)
        want, n = ndimage.label(occ, structure=ndimage.generate_binary_structure(3, rank))
        assert r["stats"][0] == n and np.array_equal(r["segment"], want[tuple(cells.T)] - 1)
        assert np.array_equal(r["size"][:n], np.bincount(want[occ] - 1))


@pytest.mark.parametrize("connectivity,rank", [(6, 1), (18, 2), (26, 3)])
def test_three_classes_have_the_partition_of_scipy(connectivity, rank):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(100 + connectivity)
    shape = (14, 13, 12)
    neigh, cells = gs.lattice_table(np.ones(shape, bool))
    lab = rng.integers(0, 3, cells.shape[0]).astype(np.int32)
    r = run(neigh, lab, 3, connectivity)
    dense = lab.reshape(shape)
    pieces, total = np.zeros(shape, np.int64), 0
    for c in range(3):
        want, n = ndimage.label(dense == c, structure=ndimage.generate_binary_structure(3, rank))
        pieces[dense == c] = want[dense == c] + total
        total += n
    assert r["stats"][0] == total
    pairs = np.unique(np.stack([r["segment"], pieces.ravel()]), axis=1)       # a bijection between the two numberings
    assert pairs.shape[1] == total and np.unique(pairs[0]).size == total and np.unique(pairs[1]).size == total
    assert np.array_equal(r["label"][r["segment"]], lab)


# ------------------------------------------------------------------------------------------------------ absorb, by hand
def absorb(neigh, lab, num_class, connectivity, min_size, drop=False, ne=None, L=None):
    M = neigh.shape[0]
    seg = run(neigh, lab, num_class, connectivity, ne=ne, L=L)
    return seg, gs.absorb_ref(neigh, lab, M if L is None else L, seg, M if ne is None else ne, num_class, connectivity,
                              min_size, drop)


def test_a_tie_goes_to_the_lowest_class():
    neigh, _ = gs.lattice_table(np.ones((7, 1, 1), bool))
    lab = np.array([2, 2, 2, 3, 1, 1, 1], np.int32)
    _, a = absorb(neigh, lab, 4, 6, 2)
    assert a["labels"].tolist() == [2, 2, 2, 1, 1, 1, 1] and a["stats"].tolist() == [1, 1, 0, 1]
    assert a["seg_label"].tolist() == [2, 1, 1, -1, -1, -1, -1]
    # two votes beat one: an L of class 0 on two sides, one voxel of class 1 on the third (26: faces and diagonals vote)
    neigh, cells = gs.lattice_table(np.ones((3, 3, 1), bool))
    lab = np.array([0, 0, 0, 0, 2, 1, 0, 1, 1], np.int32)
    _, a = absorb(neigh, lab, 3, 26, 2)
    assert a["labels"].tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 1]


def test_a_small_neighbour_does_not_vote_and_orphans_are_kept_or_dropped():
    neigh, _ = gs.lattice_table(np.ones((6, 1, 1), bool))
    lab = np.array([0, 0, 0, 2, 1, 1], np.int32)
    seg, a = absorb(neigh, lab, 3, 6, 3)
    assert seg["size"][:3].tolist() == [3, 1, 2]
    # {3} hears class 0 alone: its right neighbour is small.  {4, 5} hears nobody: an orphan, kept
    assert a["labels"].tolist() == [0, 0, 0, 0, 1, 1] and a["stats"].tolist() == [2, 1, 1, 1]
    _, a = absorb(neigh, lab, 3, 6, 3, drop=True)
    assert a["labels"].tolist() == [0, 0, 0, 0, -1, -1] and a["stats"].tolist() == [2, 1, 1, 3]
    assert a["seg_label"].tolist() == [0, 0, -1, -1, -1, -1]
    # the geometric segmentation: every small segment is an orphan, drop_orphans removes the floating cluster
    neigh, _ = table([(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 0, 0)])
    _, a = absorb(neigh, None, None, 26, 2, drop=True)
    assert a["labels"].tolist() == [0, 0, 0, -1] and a["stats"].tolist() == [1, 0, 1, 1]
    _, a = absorb(neigh, None, None, 26, 2)
    assert a["labels"].tolist() == [0, 0, 0, 0] and a["stats"].tolist() == [1, 0, 1, 0]


def test_min_size_one_is_the_identity_and_unlabelled_words_are_kept():
    neigh, _ = gs.lattice_table(np.ones((4, 3, 2), bool))
    lab = np.random.default_rng(2).integers(-1, 5, 24).astype(np.int32)      # -1 and 4 are unlabelled at num_class 4
    for drop in (False, True):
        _, a = absorb(neigh, lab, 4, 18, 1, drop=drop)
        assert np.array_equal(a["labels"], lab) and a["stats"].tolist() == [0, 0, 0, 0]
    _, a = absorb(neigh, lab, 4, 18, 1, ne=20, L=10)
    assert np.array_equal(a["labels"][:10], lab[:10]) and (a["labels"][10:] == -1).all()


def test_noise_on_four_quadrants_is_absorbed():
    neigh, clean, noisy = quadrant_field()
    seg, a = absorb(neigh, noisy, 4, 6, 4)
    after = run(neigh, a["labels"], 4, 6)
    wrong_before, wrong_after = int((noisy != clean).sum()), int((a["labels"] != clean).sum())
    print("segments %d -> %d, wrong voxels %d -> %d" % (seg["stats"][0], after["stats"][0], wrong_before, wrong_after))
    assert seg["stats"][0] > 4 and after["stats"][0] == QUADRANTS[1] and seg["stats"][0] == QUADRANTS[0]
    assert (wrong_before, wrong_after) == QUADRANTS[2:] and wrong_after < wrong_before
    big = np.nonzero(seg["size"] >= 4)[0]
    assert np.array_equal(a["seg_label"][big], seg["label"][big])
    assert sorted(seg["label"][np.argsort(seg["size"])[-4:]].tolist()) == [0, 1, 2, 3]
    assert a["stats"][0] == a["stats"][1] + a["stats"][2]


QUADRANTS = (75, 4, 78, 4)        # of quadrant_field(seed=11): segments before, after; voxels off the clean field before, after


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_object(M=4, rooms=False):
    return grid.GridRoomSubsample(10, 2, M, 6, False, "cpu") if rooms else grid.GridSubsample(10, M, 6, False, "cpu")


def cpu_segments(M=4):
    seg = grid.GridSegments(M, "cpu")
    seg._source = (cpu_object(M), None, 0, 1, 26)
    return seg


def test_the_checks_pass_up_to_the_device_check():
    lab = torch.zeros(4, dtype=torch.int32)
    for kw in ({}, {"connectivity": 6}, {"connectivity": 18}, {"voxel_labels": lab, "num_class": 1},
               {"voxel_labels": lab[:2], "num_class": 128}, {"voxel_labels": lab[:0], "num_class": 3},
               {"num_class": 5}, {"out": grid.GridSegments(4, "cpu")}):
        for g in (cpu_object(), cpu_object(rooms=True)):
            with pytest.raises(Conv3pError, match="no CPU path"):
                g.segments(**kw)
    with pytest.raises(Conv3pError, match="no CPU path"):
        cpu_object().clean_labels(lab, 3, 4)
    for kw in ({"min_size": 1}, {"min_size": 9, "drop_orphans": True}, {"min_size": 2, "out": torch.zeros(4, dtype=torch.int32)}):
        with pytest.raises(Conv3pError, match="no CPU path"):
            cpu_segments().absorb(**kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int64), num_class=3), "voxel_labels must be"),
    (dict(voxel_labels=torch.zeros((4, 1), dtype=torch.int32), num_class=3), "voxel_labels must be"),
    (dict(voxel_labels=torch.zeros(8, dtype=torch.int32)[::2], num_class=3), "voxel_labels must be"),
    (dict(voxel_labels=np.zeros(4, np.int32), num_class=3), "voxel_labels must be"),
    (dict(voxel_labels=torch.zeros(5, dtype=torch.int32), num_class=3), "more rows than"),
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int32)), "num_class must be"),
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int32), num_class=0), "num_class must be"),
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int32), num_class=129), "num_class must be"),
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int32), num_class=3.0), "num_class must be"),
    (dict(voxel_labels=torch.zeros(4, dtype=torch.int32), num_class=True), "num_class must be"),
    (dict(num_class=0), "num_class must be"),
    (dict(connectivity=7), "connectivity must be"), (dict(connectivity=26.0), "connectivity must be"),
    (dict(connectivity="26"), "connectivity must be"), (dict(connectivity=True), "connectivity must be"),
    (dict(out=torch.zeros(4, dtype=torch.int32)), "out was made"), (dict(out=grid.GridSegments(5, "cpu")), "out was made"),
])
def test_segments_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_object().segments(**kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(min_size=0), "min_size must be"), (dict(min_size=-3), "min_size must be"), (dict(min_size=2.0), "min_size must be"),
    (dict(min_size=True), "min_size must be"), (dict(min_size=2 ** 31), "min_size must be"),
    (dict(min_size=2, drop_orphans=1), "drop_orphans must be"),
    (dict(min_size=2, out=torch.zeros(4, dtype=torch.int64)), "out must be"),
    (dict(min_size=2, out=torch.zeros(5, dtype=torch.int32)), "out must be"),
    (dict(min_size=2, out=torch.zeros(8, dtype=torch.int32)[::2]), "out must be"),
])
def test_absorb_refuses_before_any_device_work(kw, msg):
    with pytest.raises(Conv3pError, match=msg):
        cpu_segments().absorb(**kw)
    lab = torch.zeros(4, dtype=torch.int32)
    if "out" not in kw:
        with pytest.raises(Conv3pError, match=msg):
            cpu_object().clean_labels(lab, 3, kw["min_size"], drop_orphans=kw.get("drop_orphans", False))


def test_absorb_needs_the_object_segments_returned():
    seg = cpu_segments()
    seg.stats[0] = 2
    t = seg.trim()
    assert t.root.shape == (2,) and t.size.shape == (2,) and t.rows.shape == (2,) and t.label.shape == (2,)
    assert t.segment.data_ptr() == seg.segment.data_ptr() and t.stats is seg.stats and t.absorbed_label is None
    assert seg.num_segments() == 2
    with pytest.raises(Conv3pError, match="not on its trim"):
        t.absorb(2)
    with pytest.raises(Conv3pError, match="not on its trim"):
        grid.GridSegments(4, "cpu").absorb(2)


# -------------------------------------------------------------------------------------------------------- the C entries
def test_the_new_symbols_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in (("conv3p_grid_segments_workspace_bytes", 1), ("conv3p_grid_segments", 17),
                    ("conv3p_grid_absorb_workspace_bytes", 1), ("conv3p_grid_absorb_segments", 19)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n
    assert _lib.load().conv3p_abi_version() == 5
    assert grid.GridSegments is __import__("pointwise_amd").GridSegments


def test_the_workspaces_depend_on_the_voxels_alone():
    lib = _lib.load()
    for f, words in ((lib.conv3p_grid_segments_workspace_bytes, 2), (lib.conv3p_grid_absorb_workspace_bytes, 4)):
        assert f(0) == 0 and f(-1) == 0 and f(1 << 31) == 0
        for M in (1, 2048, 2049, 1 << 20):
            assert 4 * words * M <= f(M) <= 4 * words * M + 8 * M // 2048 + 4096        # O(M) words, no class factor


def test_the_c_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    big = 1 << 40
    seg_names = ["neigh", "voxel_labels", "L", "voxel_count", "grid_stats", "M", "num_class", "connectivity", "segment",
                 "seg_root", "seg_size", "seg_rows", "seg_label", "seg_stats", "workspace", "workspace_bytes", "stream"]
    seg_ok = [p, p, 4, p, p, 4, 3, 26, p, p, p, p, p, p, p, big, None]
    abs_names = ["neigh", "voxel_labels", "L", "segment", "seg_size", "seg_label", "seg_stats", "grid_stats", "M", "num_class",
                 "connectivity", "min_size", "drop_orphans", "labels_out", "seg_label_out", "absorb_stats", "workspace",
                 "workspace_bytes", "stream"]
    abs_ok = [p, p, 4, p, p, p, p, p, 4, 3, 26, 2, 0, p, p, p, p, big, None]
    for f, names, ok_args, need in ((lib.conv3p_grid_segments, seg_names, seg_ok, lib.conv3p_grid_segments_workspace_bytes),
                                    (lib.conv3p_grid_absorb_segments, abs_names, abs_ok, lib.conv3p_grid_absorb_workspace_bytes)):
        def call(**ch):
            a = list(ok_args)
            for key, val in ch.items():
                a[names.index(key)] = val
            return f(*a)

        bad = [{"M": -1}, {"L": -1}, {"L": 5}, {"num_class": 0}, {"num_class": 129}, {"connectivity": 0}, {"connectivity": 7},
               {"connectivity": 27}, {"workspace": None}, {"workspace_bytes": need(4) - 1}, {"workspace_bytes": 0}]
        bad += [{n: None} for n in names if n not in ("voxel_labels", "L", "M", "num_class", "connectivity", "min_size",
                                                      "drop_orphans", "workspace_bytes", "stream", "workspace")]
        if f is lib.conv3p_grid_absorb_segments:
            bad += [{"min_size": 0}, {"min_size": -2}, {"drop_orphans": 2}, {"drop_orphans": -1}]
        for ch in bad:
            assert call(**ch) == _lib.ERR_INVALID_ARGUMENT, ch
        assert call(M=1 << 31, L=0) == _lib.ERR_UNSUPPORTED
        # no voxels: nothing to do, whatever the pointers; the argument checks still come first
        assert call(M=0, L=0) == _lib.OK
        nulls = [None if a == p else a for a in ok_args]
        nulls[names.index("M")] = nulls[names.index("L")] = nulls[names.index("workspace_bytes")] = 0
        assert f(*nulls) == _lib.OK
        assert call(M=0, L=0, connectivity=5) == _lib.ERR_INVALID_ARGUMENT
        assert call(M=0, L=1) == _lib.ERR_INVALID_ARGUMENT           # L > M
        # without labels L is not read
        assert call(voxel_labels=None, L=-7, M=0) == _lib.OK


def test_the_code_objects_have_no_spill_and_no_private_segment():
    names = ("gseg_local_kernel", "gseg_link_kernel", "gseg_flatten_kernel", "gseg_scan_kernel", "gseg_number_kernel",
             "gseg_assign_kernel", "gseg_max_kernel", "absorb_count_kernel", "absorb_plan_kernel", "absorb_scatter_kernel",
             "absorb_vote_kernel", "absorb_labels_kernel")
    res = [r for r in build.kernel_resources() if any(n in r[0] for n in names)]
    assert len(res) == len(names)
    for name, vgprs, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0 and 0 < vgprs <= 256, (name, vgprs, vgpr_spills, private)
