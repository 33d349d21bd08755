"""CPU tests (not gpu) of the many-clouds voxel-grid subsampling (include/conv3p.h: conv3p_grid_subsample_rooms_f32): the
two symbols and their argument types, the workspace bound and every status through the library (none of them launches),
the argument checks of grid.grid_subsample_rooms (all before device work), and the stitched numpy reference on a case
written out by hand and on its three error bits."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument
from tests import grid_ref as gr
from tests import grid_rooms_ref as grr

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
PTR = ctypes.c_void_p(4096)
F = np.float32


def test_symbols_are_declared_with_argtypes():
    lib = _lib.load()
    for name, nargs in (("conv3p_grid_subsample_rooms_workspace_bytes", 3), ("conv3p_grid_subsample_rooms_f32", 24)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert lib.conv3p_abi_version() == _lib.ABI_VERSION == 5                 # additions do not move it
    assert _lib.GRID_ROOMS_MAX_ROOMS == 65536


def test_workspace_bytes_through_the_library():
    lib = _lib.load()
    f, single = lib.conv3p_grid_subsample_rooms_workspace_bytes, lib.conv3p_grid_subsample_workspace_bytes
    rows = (1, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 70000, 1 << 20, 1 << 24)
    rooms = (1, 2, 7, 64, 1000, 3000, 65536)
    for mv in (1, 1000, 1 << 24, 2 ** 31 - 1):
        for R in rooms:
            sizes = [f(N, R, mv) for N in rows]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
            assert all(s >= single(N, mv) for s, N in zip(sizes, rows))      # the single call's words are all there
        for N in rows:
            sizes = [f(N, R, mv) for R in rooms]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert f(1000, 3, 1) <= f(1000, 3, 1 << 30)
    # refused, or nothing to do
    assert f(0, 3, 10) == 0 and f(-1, 3, 10) == 0 and f((1 << 24) + 1, 3, 10) == 0
    assert f(1000, 0, 10) == 0 and f(1000, -1, 10) == 0 and f(1000, 65537, 10) == 0
    assert f(1000, 3, 0) == 0 and f(1000, 3, -1) == 0


def test_status_codes_and_their_order():
    lib = _lib.load()
    f, nbytes = lib.conv3p_grid_subsample_rooms_f32, lib.conv3p_grid_subsample_rooms_workspace_bytes
    big = 1 << 40

    def call(N=100, R=3, K=6, lb=1, voxel=0.1, mode=0, ncls=13, mv=10, data=PTR, labels=PTR, start=PTR, lab_out=PTR, out=PTR,
             row=PTR, cnt=PTR, cell=PTR, room=PTR, vstart=PTR, inverse=PTR, rstats=PTR, stats=PTR, ws=PTR, ws_bytes=big):
        return f(data, labels, start, N, R, K, lb, voxel, mode, ncls, mv, out, lab_out, row, cnt, cell, room, vstart, inverse,
                 rstats, stats, ws, ws_bytes, None)
    assert call(N=-1) == INV and call(R=-1) == INV and call(K=2) == INV and call(mv=-1) == INV
    assert call(mode=2) == INV and call(mode=-1) == INV
    assert call(voxel=float("inf")) == INV and call(voxel=float("nan")) == INV and call(voxel=0.0) == INV and call(voxel=-1.0) == INV
    assert call(labels=None) == INV and call(lab_out=None) == INV and call(lb=2) == INV and call(lb=0) == INV
    assert call(ncls=0) == INV and call(ncls=-5) == INV
    assert call(ncls=0, mode=1, ws=None) == WS and call(ncls=0, labels=None, lab_out=None, ws=None) == WS   # not read there
    nothing = dict(data=None, start=None, out=None, row=None, cnt=None, cell=None, room=None, vstart=None, inverse=None,
                   rstats=None, stats=None, labels=None, lab_out=None, ws=None, ws_bytes=0)
    assert call(N=-1, mv=0) == INV and call(K=2, N=0) == INV and call(R=-1, N=0) == INV and call(mode=3, R=0) == INV
    assert call(N=0, **nothing) == OK and call(R=0, **nothing) == OK and call(mv=0, **nothing) == OK
    assert call(R=0, N=(1 << 24) + 1, K=70000, ncls=500, **nothing) == OK    # ... which comes before the limits
    for name in ("data", "start", "out", "row", "cnt", "cell", "room", "vstart", "inverse", "rstats", "stats"):
        assert call(**{name: None}) == INV, name
    assert call(data=None, N=(1 << 24) + 1) == INV and call(start=None, R=65537) == INV     # a NULL pointer before the limits
    assert call(N=(1 << 24) + 1) == UNS and call(R=65537) == UNS and call(K=65537) == UNS and call(ncls=129) == UNS
    assert call(N=1 << 24, R=65536, ws=None) == WS                           # the limits themselves are served
    assert call(ncls=129, mode=1, ws=None) == WS and call(ncls=128, ws=None) == WS
    assert call(N=(1 << 24) + 1, ws=None) == UNS and call(R=65537, ws=None) == UNS          # the limits before the workspace
    need = nbytes(100, 3, 10)
    assert need > 0 and call(ws=None) == WS and call(ws_bytes=need - 1) == WS and call(ws=ctypes.c_void_p(4097)) == WS
    assert call(mode=1, ws_bytes=need - 1) == WS and call(labels=None, lab_out=None, ws=None) == WS


START = torch.tensor([0, 4, 10], dtype=torch.int32)


@pytest.mark.parametrize("kw,msg", [
    (dict(data=torch.zeros((10, 6), dtype=torch.float64)), "float32"),
    (dict(data=torch.zeros((10, 2), dtype=torch.float32)), "float32"),
    (dict(data=torch.zeros((6, 10), dtype=torch.float32).t()), "contiguous"),
    (dict(labels=torch.zeros(10, dtype=torch.int16), num_class=4), "labels"),
    (dict(labels=torch.zeros(9, dtype=torch.int32), num_class=4), "labels"),
    (dict(voxel=0.0), "voxel"),
    (dict(voxel=float("nan")), "voxel"),
    (dict(voxel="0.1"), "voxel"),
    (dict(mode="median"), "mode"),
    (dict(labels=torch.zeros(10, dtype=torch.uint8)), "num_class"),
    (dict(labels=torch.zeros(10, dtype=torch.uint8), num_class=129), "num_class"),
    (dict(num_class=2.5), "num_class"),
    (dict(max_voxels=-1), "max_voxels"),
    (dict(max_voxels=2 ** 31), "max_voxels"),
    (dict(room_start=[0, 4, 10]), "room_start"),
    (dict(room_start=np.array([0, 4, 10], np.int32)), "room_start"),
    (dict(room_start=torch.tensor([0, 4, 10], dtype=torch.int64)), "room_start"),
    (dict(room_start=torch.zeros((2, 2), dtype=torch.int32)), "room_start"),
    (dict(room_start=torch.zeros((0,), dtype=torch.int32)), "room_start"),
    (dict(room_start=torch.zeros((8,), dtype=torch.int32)[::2]), "room_start"),
    (dict(room_start=torch.zeros((65538,), dtype=torch.int32)), "65536 rooms"),
    (dict(out=object()), "another shape"),
    (dict(out=grid.GridSubsample(10, 10, 6, False, torch.device("cpu"))), "another shape"),
])
def test_argument_checks_raise_before_device_work(kw, msg):
    a = dict(data=torch.zeros((10, 6), dtype=torch.float32), room_start=START)
    a.update(kw)
    with pytest.raises(Conv3pInvalidArgument, match=msg):
        grid.grid_subsample_rooms(**a)


def test_the_checks_of_grid_subsample_come_first_and_the_no_cpu_path_check_last():
    data = torch.zeros((10, 6), dtype=torch.float32)
    with pytest.raises(Conv3pInvalidArgument, match="voxel"):                # before room_start's
        grid.grid_subsample_rooms(data, [0, 10], voxel=-1.0)
    with pytest.raises(Conv3pInvalidArgument, match="max_voxels"):
        grid.grid_subsample_rooms(data, [0, 10], max_voxels=-2)
    out = grid.GridRoomSubsample(10, 2, 8, 6, False, torch.device("cpu"))
    assert out.voxel_room.shape == (8,) and out.voxel_start.shape == (3,) and out.room_stats.shape == (2, 8)
    for kw in (dict(max_voxels=9), dict(max_voxels=8, data=torch.zeros((11, 6))), dict(max_voxels=8, data=torch.zeros((10, 7))),
               dict(max_voxels=8, labels=torch.zeros(10, dtype=torch.uint8), num_class=3),
               dict(max_voxels=8, room_start=torch.tensor([0, 4, 6, 10], dtype=torch.int32))):
        a = dict(data=data, room_start=START, out=out)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument, match="another shape"):
            grid.grid_subsample_rooms(**a)
    with pytest.raises(Conv3pInvalidArgument, match="room_start"):           # before out's shape
        grid.grid_subsample_rooms(data, [0, 4, 10], max_voxels=9, out=out)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):          # every check passed: only the device is wrong
        grid.grid_subsample_rooms(data, START, max_voxels=8, out=out)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):
        grid.grid_subsample_rooms(data, START, torch.zeros(10, dtype=torch.int64), mode="center")
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):          # project is GridSubsample's
        out.project(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(Conv3pInvalidArgument, match="room number"):
        out.room(2)


def test_reference_on_the_hand_cloud_as_two_rooms():
    d, l = gr.hand_cloud()
    data, labels = np.concatenate([d, d]), np.concatenate([l, l])
    one = gr.grid_subsample_ref(d, l, voxel=0.5, mode="mean", num_class=4, max_voxels=5)
    r = grr.grid_subsample_rooms_ref(data, [0, 12, 24], labels, voxel=0.5, mode="mean", num_class=4, max_voxels=12)
    assert r["stats"].tolist() == [10, 10, 2, 2, 0, 4, 4, 0]
    assert r["room_stats"].tolist() == [[5, 5, 3, 2, 3, 2, 4, 0]] * 2 and r["voxel_start"].tolist() == [0, 5, 10]
    inv = [0, 0, 3, -1, 0, 1, 3, 0, 2, -1, 1, 4]
    assert r["inverse"].tolist() == inv + [v + 5 if v >= 0 else -1 for v in inv]         # room 1 behind room 0's five voxels
    assert r["voxel_room"].tolist() == [0] * 5 + [1] * 5 + [-1, -1]
    assert r["voxel_row"].tolist() == [0, 5, 8, 2, 11, 12, 17, 20, 14, 23, -1, -1]       # global rows
    assert r["voxel_cell"][:5].tolist() == r["voxel_cell"][5:10].tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 2], [2, 0, 0], [2, 0, 2]]
    assert r["voxel_count"].tolist() == [4, 2, 1, 2, 1] * 2 + [0, 0] and r["labels"].tolist() == [1, 0, 0, -1, 3] * 2 + [-1, -1]
    for a in (0, 5):                                                         # twice the voxels, bit for bit
        assert np.array_equal(r["data"][a:a + 5].view(np.uint32), one["data"].view(np.uint32))
    assert not r["data"][10:].any()
    # the cut inside room 1: max_voxels_1 = 7 - 5 = 2; and before it: words 1-7 of room 1 are still written
    cut = grr.grid_subsample_rooms_ref(data, [0, 12, 24], labels, voxel=0.5, mode="center", max_voxels=7)
    assert cut["stats"].tolist() == [7, 10, 2, 2, 0, 4, 4, 0] and cut["voxel_start"].tolist() == [0, 5, 7]
    assert cut["room_stats"].tolist() == [[5, 5, 3, 2, 3, 2, 4, 0], [2, 5, 3, 2, 3, 2, 4, 0]]
    assert cut["inverse"].tolist() == inv + [5, 5, -1, -1, 5, 6, -1, 5, -1, -1, 6, -1]
    assert cut["voxel_row"].tolist() == [1, 10, 8, 6, 11, 13, 22]
    cut = grr.grid_subsample_rooms_ref(data, [0, 12, 24], labels, voxel=0.5, mode="mean", num_class=4, max_voxels=3)
    assert cut["stats"].tolist() == [3, 10, 2, 1, 0, 4, 4, 0] and cut["voxel_start"].tolist() == [0, 3, 3]
    assert cut["room_stats"].tolist() == [[3, 5, 3, 2, 3, 2, 4, 0], [0, 5, 3, 2, 3, 2, 4, 0]]
    assert (cut["inverse"][12:] == -1).all() and cut["inverse"][:12].tolist() == [0, 0, -1, -1, 0, 1, -1, 0, 2, -1, 1, -1]
    # rows outside the rooms, and an empty room between them
    r = grr.grid_subsample_rooms_ref(data, [1, 12, 12, 23], labels, voxel=0.5, mode="mean", num_class=4)
    assert r["inverse"][0] == -1 and r["inverse"][23] == -1 and r["room_stats"][1].tolist() == [0] * 8
    assert r["stats"][[2, 3, 5]].tolist() == [3, 2, 4] and r["voxel_start"][1] == r["voxel_start"][2]
    # nothing to do
    for kw in (dict(room_start=[5]), dict(room_start=[0, 12, 24], max_voxels=0)):
        e = grr.grid_subsample_rooms_ref(data, labels=labels, voxel=0.5, num_class=4, **kw)
        assert not e["stats"].any() and (e["inverse"] == -1).all() and not e["voxel_start"].any() and not e["room_stats"].any()


def test_reference_reports_the_three_error_bits():
    ok = np.array([[0.5, 0.5, 0.5], [3.5, 1.5, 0.5]], F)
    far = np.array([[0.5, 0.5, 0.5], [1048576.5, 0.5, 0.5]], F)             # n_x = 2^20 + 1
    data = np.concatenate([ok, far, ok + F(7.0)])
    r = grr.grid_subsample_rooms_ref(data, [0, 2, 4, 6], None, voxel=1.0)
    assert r["stats"].tolist() == [4, 4, 3, 2, 1, 0, 1, 1]                  # bit 0: the room in the middle emits nothing
    assert r["room_stats"].tolist() == [[2, 2, 4, 2, 1, 0, 1, 0], [0, 0, (1 << 20) + 1, 1, 1, 0, 0, 1], [2, 2, 4, 2, 1, 0, 1, 0]]
    assert r["inverse"].tolist() == [0, 1, -1, -1, 2, 3] and r["voxel_start"].tolist() == [0, 2, 2, 4]
    assert r["voxel_room"].tolist() == [0, 0, 2, 2, -1, -1]
    for start in ([0, 4, 2, 6], [-1, 2, 6], [0, 2, 7]):                     # bit 1: a decrease, a negative first, a last above N
        r = grr.grid_subsample_rooms_ref(data, start, None, voxel=1.0)
        assert r["stats"].tolist() == [0, 0, len(start) - 1, 0, 0, 0, 0, 2] and (r["inverse"] == -1).all()
        assert not r["voxel_start"].any() and not r["room_stats"].any() and (r["voxel_room"] == -1).all()
    a = np.array([[0.5, 0.5, 0.5], [1048575.5, 1023.5, 1022.5]], F)         # 2^20 x 1024 x 1023 cells
    b = np.array([[0.5, 0.5, 0.5], [1023.5, 1023.5, 1023.5]], F)            # 2^30 cells: 2^40 in all
    c = np.array([[5.0, 5.0, np.nan], [5.0, 5.0, 5.0]], F)                  # one cell more
    r = grr.grid_subsample_rooms_ref(np.concatenate([a, b]), [0, 2, 4], None, voxel=1.0)
    assert r["stats"].tolist() == [4, 4, 2, 2, 0, 0, 1, 0]
    r = grr.grid_subsample_rooms_ref(np.concatenate([a, b, c]), [0, 2, 4, 6], None, voxel=1.0)
    assert r["stats"].tolist() == [0, 0, 3, 0, 0, 1, 0, 4] and (r["inverse"] == -1).all() and not r["voxel_start"].any()
    assert r["room_stats"].tolist() == [[0, 0, 1 << 20, 1024, 1023, 0, 0, 0], [0, 0, 1024, 1024, 1024, 0, 0, 0],
                                        [0, 0, 1, 1, 1, 1, 0, 0]]
