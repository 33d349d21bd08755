"""CPU tests (not gpu) of the interpolated projection: tests/grid_interp_ref.py against a brute-force neighbour lookup and
against project_ref where the two must agree, every Python argument check of GridSubsample.neighbors / interpolate (each
raises before any device work: the objects here live on the CPU), and the new symbols in _lib's table."""
import numpy as np
import pytest
import torch

from pointwise_amd import _lib, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument as Conv3pError
from tests import grid_interp_ref as gi
from tests import grid_ref as gr

F = np.float32


def lattice(seed, n, fill, rooms=None):
    """Random occupied cells of an n[0] x n[1] x n[2] lattice in ascending order (per room) -> voxel_cell, room, start."""
    rng = np.random.default_rng(seed)
    cells, room, start = [], [], [0]
    for r in range(rooms or 1):
        total = n[0] * n[1] * n[2]
        c = np.sort(rng.permutation(total)[:max(1, int(fill * total))])
        cells.append(np.stack([c // (n[1] * n[2]), (c // n[2]) % n[1], c % n[2]], axis=1))
        room += [r] * c.size
        start.append(start[-1] + c.size)
    cell = np.concatenate(cells).astype(np.int32)
    return cell, (np.asarray(room, np.int32) if rooms else None), (np.asarray(start, np.int32) if rooms else None)


@pytest.mark.parametrize("seed,n,fill", [(1, (5, 5, 5), 1.0), (2, (7, 4, 9), 0.5), (3, (12, 11, 1), 0.3), (4, (1, 1, 40), 0.6),
                                         (5, (30, 30, 30), 0.02)])
def test_the_neighbour_table_against_a_dictionary_lookup(seed, n, fill):
    cell, _, _ = lattice(seed, n, fill)
    V = cell.shape[0]
    filler = np.full((5, 3), -1, np.int32)
    for ne, table in ((V, cell), (V, np.concatenate([cell, filler])), (V // 2, cell)):
        got = gi.neighbors_ref(table, ne)
        assert np.array_equal(got, gi.neighbors_brute(table, ne))
        assert np.array_equal(got[:ne, 13], np.arange(ne)) and (got[ne:] == -1).all()
        assert got.max() < max(ne, 1)                    # a cut voxel is in nobody's row
    if fill == 1.0:
        full = gi.neighbors_ref(cell, V)
        per = (full >= 0).sum(axis=1)
        assert per.max() == 27 and per.min() == 8 and (per == 8).sum() == 8 and (per == 27).sum() == 27


def test_rooms_share_no_neighbour():
    cell, room, start = lattice(6, (6, 5, 4), 0.6, rooms=3)      # the rooms' lattices coincide in space
    V = cell.shape[0]
    got = gi.neighbors_ref(cell, V, room, start)
    assert np.array_equal(got, gi.neighbors_brute(cell, V, room))
    assert np.array_equal(got[:, 13], np.arange(V))
    hit = got >= 0
    assert np.array_equal(room[got[hit]], np.broadcast_to(room[:, None], got.shape)[hit])
    for r in range(3):                                   # a room's slice is the single table, shifted
        a, b = start[r], start[r + 1]
        one = gi.neighbors_ref(cell[a:b], b - a)
        assert np.array_equal(got[a:b], np.where(one >= 0, one + a, -1))


def test_one_neighbour_where_every_row_is_its_own_voxel_is_the_projection_of_the_argmax():
    rng = np.random.default_rng(11)
    N = 600
    cells = np.concatenate([[0], 1 + rng.permutation(10 * 10 * 10 - 1)[:N - 1]])
    ijk = np.stack([cells // 100, (cells // 10) % 10, cells % 10], axis=1)
    xyz = (ijk + 0.25 + 0.5 * rng.random((N, 3))) * 0.1
    xyz[0] = 0.0
    data = np.concatenate([xyz, rng.random((N, 2))], axis=1).astype(F)
    data[7, 1] = np.nan
    for mode in ("mean", "center"):
        g = gr.grid_subsample_ref(data, None, voxel=0.1, mode=mode)
        V = int(g["stats"][0])
        assert V == N - 1
        scores = rng.standard_normal((V, 13)).astype(F)
        neigh = gi.neighbors_ref(g["voxel_cell"], V)
        lab, out, stats = gi.interpolate_ref(data, g["inverse"], g["data"], neigh, scores, k=1)
        # the row is its voxel's representative: d2 = 0, the weight 1e10, and (1e10 s) / 1e10 keeps the order of the classes
        assert np.array_equal(lab, gr.project_ref(scores.argmax(axis=1).astype(np.int32), g["inverse"]))
        assert stats.tolist() == [N - 1, 1, 0] and lab[7] == -1 and not out[7].any()


def test_the_reference_on_a_case_written_out_by_hand():
    # two voxels 0.5 apart on x, a row a quarter of the way: d2 = 1/64 and 9/64, weights 64 and 64/9
    data = np.array([[0.125, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    voxel_data = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], F)
    neigh = np.full((2, 27), -1, np.int32)
    neigh[0, 13], neigh[0, 22], neigh[1, 13], neigh[1, 4] = 0, 1, 1, 0
    inverse = np.array([0, 0, 1, -1], np.int32)
    scores = np.array([[1.0, 0.0], [0.0, 1.0]], F)
    lab, out, stats, chosen, ties = gi.interpolate_ref(data, inverse, voxel_data, neigh, scores, k=3, detail=True)
    w0, w1 = F(1.0) / F(1.0 / 64.0), F(1.0) / F(9.0 / 64.0)
    assert out[0, 0] == F(w0 / F(w0 + w1)) and out[0, 1] == F(w1 / F(w0 + w1)) and lab.tolist() == [0, 0, 1, -1]
    assert chosen[0].tolist() == [0, 1] + [-1] * 6 and chosen[2].tolist() == [1, 0] + [-1] * 6 and not ties.any()
    assert stats.tolist() == [3, 1, 0] and not out[3].any()
    big = F(1.0) / F(1e-10)                              # row 1 coincides with voxel 0: the floor, not a division by zero
    assert F(big + F(4.0)) == big and out[1, 0] == F(1.0)                  # W = 1e10 + 4 rounds to 1e10 ...
    assert out[1, 1] == F(F(4.0) / big) and out[1, 1] != scores[0, 1]      # ... and voxel 1 still reaches class 1
    # an invalid voxel is no candidate; with both invalid nothing is left
    lab, out, stats = gi.interpolate_ref(data, inverse, voxel_data, neigh, scores, k=3, valid_labels=np.array([-1, 1], np.int32))
    assert lab.tolist() == [1, 1, 1, -1] and stats.tolist() == [3, 1, 0]
    lab, out, stats = gi.interpolate_ref(data, inverse, voxel_data, neigh, scores, k=3, valid_labels=np.array([-1, -1], np.int32))
    assert lab.tolist() == [-1] * 4 and stats.tolist() == [0, 1, 3] and not out.any()
    # the int64 sums: float32(s) rounds to nearest even before the exact scaling
    s64 = np.array([[(1 << 40) + (1 << 16), 1 << 30], [(1 << 24) + 1, (1 << 24) + 3]], np.int64)
    lab, out, _ = gi.interpolate_ref(data[1:2], inverse[1:2], voxel_data, neigh, s64, k=1)
    assert out[0, 0] == F(1024.0) and out[0, 1] == F(1.0)
    lab, out, _ = gi.interpolate_ref(data[2:3], inverse[2:3], voxel_data, neigh, s64, k=1)
    assert out[0, 0] == F(2.0 ** -6) and out[0, 1] == F((2.0 ** 24 + 4) * 2.0 ** -30) and lab[0] == 1


# ------------------------------------------------------------------------------------------------- the argument checks
def cpu_object(N=10, M=4, K=6, rooms=False):
    g = grid.GridRoomSubsample(N, 2, M, K, False, "cpu") if rooms else grid.GridSubsample(N, M, K, False, "cpu")
    return g, torch.zeros((N, K)), torch.zeros((M, 13))


def test_the_checks_pass_up_to_the_device_check():
    g, data, scores = cpu_object()
    with pytest.raises(Conv3pError, match="no CPU path"):
        g.interpolate(data, scores)
    with pytest.raises(Conv3pError, match="no CPU path"):
        g.interpolate(data, scores, k=8, valid_labels=torch.zeros(4, dtype=torch.int32), return_scores=True,
                      out=(torch.zeros(10, dtype=torch.int32), torch.zeros((10, 13))))
    with pytest.raises(Conv3pError, match="no CPU path"):
        g.neighbors()
    with pytest.raises(Conv3pError, match="no CPU path"):
        cpu_object(rooms=True)[0].neighbors()


@pytest.mark.parametrize("what,msg", [
    ("data dtype", "data must be a float32"), ("data shape", "data must be a float32"), ("data K", "data must be a float32"),
    ("data strided", "data must be contiguous"), ("data rows", "inverse has 10"),
    ("k 0", "k must be"), ("k 9", "k must be"), ("k float", "k must be"), ("k bool", "k must be"),
    ("scores dtype", "voxel_scores must be"), ("scores shape", "voxel_scores must be"), ("scores strided", "voxel_scores must be"),
    ("scores list", "voxel_scores must be"), ("C 129", "at most 128 classes"), ("C 0", "at most 128 classes"),
    ("M large", "more rows than the subsampling"),
    ("valid dtype", "valid_labels must be"), ("valid shape", "valid_labels must be"), ("valid strided", "valid_labels must be"),
    ("out pair", "out must be"), ("out dtype", "out labels must be"), ("out shape", "out labels must be"),
    ("out strided", "out labels must be"), ("out scores shape", "out scores must be"), ("out scores dtype", "out scores must be"),
])
def test_interpolate_refuses_before_any_device_work(what, msg):
    g, data, scores = cpu_object()
    kw = {}
    if what == "data dtype": data = data.double()
    elif what == "data shape": data = data[0]
    elif what == "data K": data = data[:, :2].contiguous()
    elif what == "data strided": data = torch.zeros((10, 12))[:, ::2]
    elif what == "data rows": data = torch.zeros((11, 6))
    elif what == "k 0": kw["k"] = 0
    elif what == "k 9": kw["k"] = 9
    elif what == "k float": kw["k"] = 3.0
    elif what == "k bool": kw["k"] = True
    elif what == "scores dtype": scores = scores.double()
    elif what == "scores shape": scores = scores[0]
    elif what == "scores strided": scores = torch.zeros((4, 26))[:, ::2]
    elif what == "scores list": scores = [[0.0] * 13] * 4
    elif what == "C 129": scores = torch.zeros((4, 129))
    elif what == "C 0": scores = torch.zeros((4, 0))
    elif what == "M large": scores = torch.zeros((5, 13))
    elif what == "valid dtype": kw["valid_labels"] = torch.zeros(4, dtype=torch.int64)
    elif what == "valid shape": kw["valid_labels"] = torch.zeros(5, dtype=torch.int32)
    elif what == "valid strided": kw["valid_labels"] = torch.zeros(8, dtype=torch.int32)[::2]
    elif what == "out pair": kw.update(return_scores=True, out=torch.zeros(10, dtype=torch.int32))
    elif what == "out dtype": kw["out"] = torch.zeros(10, dtype=torch.int64)
    elif what == "out shape": kw["out"] = torch.zeros(9, dtype=torch.int32)
    elif what == "out strided": kw["out"] = torch.zeros(20, dtype=torch.int32)[::2]
    elif what == "out scores shape": kw.update(return_scores=True, out=(torch.zeros(10, dtype=torch.int32), torch.zeros((10, 12))))
    elif what == "out scores dtype":
        kw.update(return_scores=True, out=(torch.zeros(10, dtype=torch.int32), torch.zeros((10, 13), dtype=torch.float64)))
    with pytest.raises(Conv3pError, match=msg):
        g.interpolate(data, scores, **kw)


@pytest.mark.parametrize("what", ["cell dtype", "cell shape", "cell strided", "stats dtype", "room dtype", "room shape", "start dtype"])
def test_neighbors_refuses_before_any_device_work(what):
    g = cpu_object(rooms=what.startswith(("room", "start")))[0]
    if what == "cell dtype": g.voxel_cell = g.voxel_cell.long()
    elif what == "cell shape": g.voxel_cell = torch.zeros((4, 2), dtype=torch.int32)
    elif what == "cell strided": g.voxel_cell = torch.zeros((4, 6), dtype=torch.int32)[:, ::2]
    elif what == "stats dtype": g.stats = g.stats.long()
    elif what == "room dtype": g.voxel_room = g.voxel_room.long()
    elif what == "room shape": g.voxel_room = torch.zeros(3, dtype=torch.int32)
    elif what == "start dtype": g.voxel_start = g.voxel_start.long()
    with pytest.raises(Conv3pError, match="must be a contiguous int32 tensor"):
        g.neighbors()


def test_the_new_symbols_are_declared_and_exported():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("conv3p_grid_neighbors", "conv3p_grid_interpolate_f32", "conv3p_grid_interpolate_i64"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.SYMBOLS["conv3p_grid_interpolate_f32"] == _lib.SYMBOLS["conv3p_grid_interpolate_i64"]
    assert len(_lib.SYMBOLS["conv3p_grid_interpolate_f32"][1]) == 16 and len(_lib.SYMBOLS["conv3p_grid_neighbors"][1]) == 8


def test_the_c_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    import ctypes
    words = (ctypes.c_int64 * 8)()                       # never read: every call below is refused before a launch
    p = ctypes.addressof(words)
    f = lib.conv3p_grid_interpolate_f32
    ok_args = [p, 4, 6, p, p, 6, p, p, 2, 13, None, 3, p, None, p, None]

    def call(**ch):
        names = ["data", "N", "K", "inverse", "voxel_data", "voxel_K", "neigh", "scores", "M", "C", "valid", "k", "labels",
                 "out_scores", "stats", "stream"]
        a = list(ok_args)
        for key, val in ch.items():
            a[names.index(key)] = val
        return a

    for fn in (f, lib.conv3p_grid_interpolate_i64):
        for ch in ({"N": -1}, {"M": -1}, {"K": 2}, {"voxel_K": 2}, {"C": 0}, {"C": 129}, {"k": 0}, {"k": 9}, {"stats": None},
                   {"data": None}, {"inverse": None}, {"labels": None}, {"voxel_data": None}, {"neigh": None}, {"scores": None}):
            assert fn(*call(**ch)) == _lib.ERR_INVALID_ARGUMENT, ch
        assert fn(*call(N=1 << 31)) == _lib.ERR_UNSUPPORTED and fn(*call(M=1 << 31)) == _lib.ERR_UNSUPPORTED
    g = lib.conv3p_grid_neighbors
    assert g(p, None, None, p, -1, 0, p, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(p, None, None, p, 4, -1, p, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(p, p, None, p, 4, 1, p, None) == _lib.ERR_INVALID_ARGUMENT and g(p, None, p, p, 4, 1, p, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(None, None, None, p, 4, 0, p, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(p, None, None, None, 4, 0, p, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(p, None, None, p, 4, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert g(p, p, p, p, 4, 65537, p, None) == _lib.ERR_UNSUPPORTED
    assert g(None, None, None, None, 0, 0, None, None) == _lib.OK          # no voxels: nothing to do
