"""CPU tests (not gpu) of the many-rooms tiling (include/conv3p.h: conv3p_scene_blocks_rooms_f32): the numpy reference
against its naive restatement, the argument checks of scene.scene_blocks_rooms (all before device work), the workspace
bound through the library, and the default max_blocks against what the fixtures need."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, scene
from pointwise_amd.conv3p_op import Conv3pInvalidArgument
from tests import scene_ref as base
from tests import scene_rooms_ref as rr

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
PTR = ctypes.c_void_p(4096)


def small_rooms():
    """Four small rooms for the naive loops: a room, an empty one, one on cell edges, one with non-finite rows."""
    a = base.room(400, 21, (2.6, 1.7, 3.0))
    c = base.room(300, 22, (2.0, 2.0, 3.0), quantum=0.25) + np.float32(0)     # no -0.0: the _naive twins take Python's min, whose zero has no one sign
    d = base.room(200, 23, (1.5, 2.4, 3.0))
    d[3, 0], d[50, 1], d[199, 2] = np.inf, np.nan, -np.inf
    return rr.concat([a, a[:0], c, d])


@pytest.mark.parametrize("cover", [False, True])
@pytest.mark.parametrize("stride,min_points,max_blocks", [(1.0, 20, 64), (0.5, 1, 400), (1.0, 20, 7), (0.5, 1, 30), (1.0, 1, 0)])
def test_reference_equals_the_naive_restatement(cover, stride, min_points, max_blocks):
    data, rs, labels = small_rooms()
    a = rr.call_args(num_point=16, stride=stride, min_points=min_points, max_blocks=max_blocks)
    want = rr.rooms_blocks_ref(data, labels, rs, cover=cover, **a)
    rr.assert_equal(rr.rooms_blocks_naive(data, labels, rs, cover=cover, **a), want)
    assert int(want["stats"][2]) == 4 and want["room_stats"][1].tolist() == [0] * 8
    assert int(want["room_stats"][3][4]) == 3 and int(want["stats"][4]) == 3
    assert want["room_blocks"][-1] == want["stats"][0] == (want["block_room"] >= 0).sum()
    assert np.array_equal(np.diff(want["room_blocks"]), want["room_stats"][:, 0])
    nb = int(want["stats"][0])
    assert (want["index"][:nb] >= 0).all() and (want["index"][nb:] == -1).all()
    room_of_row = np.searchsorted(rs, want["index"][:nb], side="right") - 1
    assert np.array_equal(room_of_row, np.broadcast_to(want["block_room"][:nb, None], room_of_row.shape))


def test_reference_on_a_malformed_room_start_and_on_one_room():
    data, rs, labels = small_rooms()
    for bad in ([0, 500, 400, 900], [-1, 400, 900], [0, 400, 901]):
        r = rr.rooms_blocks_ref(data, labels, bad, max_blocks=5, **rr.call_args())
        assert r["stats"].tolist() == [0, 0, len(bad) - 1, 0, 0, 0, 0, 2] and not r["room_blocks"].any() and (r["index"] == -1).all()
    one = data[:400]
    for cover, fn in ((False, base.scene_blocks_ref), (True, __import__("tests.scene_cover_ref", fromlist=["x"]).cover_blocks_ref)):
        a = rr.call_args(num_point=16, min_points=20, max_blocks=40)
        got = rr.rooms_blocks_ref(one, labels[:400], [0, 400], cover=cover, **a)
        want = fn(one, labels[:400], **a)
        for k in ("data", "labels", "index", "block_cell", "block_count"):
            assert np.array_equal(got[k], want[k]), k
        assert got["room_stats"][0].tolist() == want["stats"].tolist()


def _dev_free_args():
    data = torch.zeros((10, 6), dtype=torch.float32)
    return data, [0, 4, 10]


@pytest.mark.parametrize("kw,msg", [
    (dict(room_start=[0, 6, 4, 10]), "ascend"),
    (dict(room_start=[0, 4, 11]), "ascend"),
    (dict(room_start=[-1, 4, 10]), "ascend"),
    (dict(room_start=np.array([0.0, 4.0, 10.0])), "integers"),
    (dict(room_start=torch.tensor([0.0, 4.0, 10.0])), "integers"),
    (dict(room_start=np.zeros((2, 2), np.int32)), "R \\+ 1"),
    (dict(room_start=[]), "room_start"),
    (dict(data=torch.zeros((10, 6), dtype=torch.float64)), "float32"),
    (dict(data=torch.zeros((10, 2), dtype=torch.float32)), "float32"),
    (dict(labels=torch.zeros(10, dtype=torch.int16)), "labels"),
    (dict(labels=torch.zeros(9, dtype=torch.int32)), "labels"),
    (dict(num_point=0), "num_point"),
    (dict(num_point=65537), "num_point"),
    (dict(block=float("nan")), "block"),
    (dict(stride=0.0), "stride"),
    (dict(block=1.0, stride=0.4), "2 stride"),
    (dict(min_points=2 ** 31), "min_points"),
    (dict(cover=1), "cover"),
    (dict(max_blocks=-1), "max_blocks"),
    (dict(seed=-1), "seed"),
    (dict(step=2 ** 64), "seed"),
    (dict(out=object()), "another shape"),
])
def test_argument_checks_raise_before_device_work(kw, msg):
    data, rs = _dev_free_args()
    a = dict(data=data, room_start=rs)
    a.update(kw)
    with pytest.raises(Conv3pInvalidArgument, match=msg):
        scene.scene_blocks_rooms(**a)


def test_out_of_another_shape_and_the_no_cpu_path_check_come_last():
    data, rs = _dev_free_args()
    out = scene.SceneRoomBlocks(8, 64, 6, False, torch.device("cpu"), 0, 2)
    for kw in (dict(max_blocks=9), dict(max_blocks=8, num_point=32), dict(max_blocks=8, room_start=[0, 10]),
               dict(max_blocks=8, labels=torch.zeros(10, dtype=torch.uint8))):
        a = dict(data=data, room_start=rs, num_point=64, out=out)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument, match="another shape"):
            scene.scene_blocks_rooms(**a)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):          # every check passed: only the device is wrong
        scene.scene_blocks_rooms(data, rs, num_point=64, max_blocks=8, out=out)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):
        scene.scene_blocks_rooms(data, torch.tensor([0, 4, 10], dtype=torch.int64))


def test_workspace_bytes_through_the_library():
    lib = _lib.load()
    assert "conv3p_scene_blocks_rooms_f32" in _lib.SYMBOLS and _lib.SCENE_ROOMS_MAX_CELLS == 1 << 20
    f = lib.conv3p_scene_blocks_rooms_workspace_bytes
    for cover in (0, 1):
        for stride in (1.0, 0.5):
            sizes = [f(N, 3, 64, 100, 1.0, stride, cover) for N in (1, 1000, 1024, 1025, 70000, 1 << 20, 1 << 26)]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
            m = 2 if stride == 1.0 else 3
            assert sizes[-2] >= (1 << 20) * m * m * 16                       # the two pair buffers
        assert f(1000, 1, 64, 100, 1.0, 0.5, cover) <= f(1000, 65536, 64, 100, 1.0, 0.5, cover)
        assert f(1000, 3, 64, 100, 1.0, 0.5, cover) <= f(1000, 3, 64, 100000, 1.0, 0.5, cover)
        # refused, or nothing to do
        assert f(0, 3, 64, 100, 1.0, 1.0, cover) == 0 and f(-1, 3, 64, 100, 1.0, 1.0, cover) == 0
        assert f((1 << 26) + 1, 3, 64, 100, 1.0, 1.0, cover) == 0
        assert f(1000, 0, 64, 100, 1.0, 1.0, cover) == 0 and f(1000, -1, 64, 100, 1.0, 1.0, cover) == 0
        assert f(1000, 65537, 64, 100, 1.0, 1.0, cover) == 0
        assert f(1000, 3, 0, 100, 1.0, 1.0, cover) == 0 and f(1000, 3, 65537, 100, 1.0, 1.0, cover) == 0
        assert f(1000, 3, 64, 0, 1.0, 1.0, cover) == 0 and f(1000, 3, 64, -1, 1.0, 1.0, cover) == 0
        assert f(1000, 3, 64, 100, 1.0, 0.4, cover) == 0 and f(1000, 3, 64, 100, 0.5, 1.0, cover) == 0
        assert f(1000, 3, 64, 100, float("nan"), 1.0, cover) == 0 and f(1000, 3, 64, 100, 1.0, 0.0, cover) == 0
    assert f(1000, 3, 64, 100, 1.0, 1.0, 2) == 0 and f(1000, 3, 64, 100, 1.0, 1.0, -1) == 0


def test_status_codes_and_their_order():
    lib = _lib.load()
    f, nbytes = lib.conv3p_scene_blocks_rooms_f32, lib.conv3p_scene_blocks_rooms_workspace_bytes
    big = 1 << 40

    def call(N=100, R=2, K=6, lb=1, block=1.0, stride=1.0, P=64, mb=10, cover=0, data=PTR, labels=PTR, rs=PTR, lab_out=PTR,
             out=PTR, ws=PTR, ws_bytes=big):
        return f(data, labels, rs, N, R, K, lb, block, stride, P, 100, mb, cover, 0, 0, out, lab_out, out, out, out, out, out,
                 out, out, ws, ws_bytes, None)
    assert call(N=-1) == INV and call(R=-1) == INV and call(K=2) == INV and call(P=0) == INV and call(mb=-1) == INV
    assert call(cover=2) == INV and call(block=float("inf")) == INV and call(stride=0.0) == INV
    assert call(labels=None) == INV and call(lab_out=None) == INV and call(lb=2) == INV
    assert call(R=-1, N=0) == INV                                            # invalid arguments before "nothing to do"
    assert call(R=0, data=None, rs=None, out=None, labels=None, lab_out=None) == OK
    assert call(N=0, data=None, rs=None, out=None, labels=None, lab_out=None) == OK
    assert call(mb=0, data=None, rs=None, out=None, labels=None, lab_out=None) == OK
    assert call(data=None) == INV and call(rs=None) == INV and call(out=None) == INV
    assert call(N=(1 << 26) + 1) == UNS and call(R=65537) == UNS and call(P=65537) == UNS and call(K=65537) == UNS
    assert call(stride=0.4) == UNS and call(block=0.5) == UNS
    need = nbytes(100, 2, 64, 10, 1.0, 1.0, 0)
    assert need > 0 and call(ws=None) == WS and call(ws_bytes=need - 1) == WS and call(ws=ctypes.c_void_p(4097)) == WS


def test_default_max_blocks_covers_what_the_fixtures_need():
    data, rs, _ = rr.three_rooms()
    rows = np.diff(rs).tolist()
    for cover in (False, True):
        for stride in (1.0, 0.5):
            for min_points in (100, 1):
                a, mb, want = rr.three_rooms_ref(stride, min_points, cover)
                need = rr.blocks_needed(want, cover)
                assert need == mb == int(want["stats"][0])
                P = a["num_point"] if cover else None
                summed = scene.default_max_blocks_rooms(rows, 1.0, stride, min_points, P)
                assert summed == sum(scene.default_max_blocks(n, 1.0, stride, min_points, P) for n in rows) >= need
                assert scene._rooms_bound(data.shape[0], len(rows), 1.0, stride, min_points, P) >= summed
