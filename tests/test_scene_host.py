"""CPU tests (not gpu) of the scene tiling and voting (include/conv3p.h: conv3p_scene_blocks_f32, conv3p_scene_vote,
conv3p_scene_vote_labels and their _bytes functions): the symbols and constants, the status codes and their order -- all
decided before any HIP call, so bogus (never dereferenced) pointers are fine -- the workspace sizes, the Python checks
that come before device work, and the numpy restatement itself (tests/scene_ref.py): its two forms agree, every emitted
index is a member of its cell, and the fixtures of tests/test_scene.py have the shape that file relies on."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pointwise_amd
from pointwise_amd import _lib, scene
from pointwise_amd.conv3p_op import Conv3pInvalidArgument
from tests import scene_ref as ref

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
P = ctypes.c_void_p(4096)
NAMES = ("conv3p_scene_blocks_workspace_bytes", "conv3p_scene_blocks_f32", "conv3p_scene_vote",
         "conv3p_scene_vote_labels_workspace_bytes", "conv3p_scene_vote_labels")


def test_symbols_constants_and_abi_version():
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    assert _lib.SCENE_MAX_CELLS == 65536 and _lib.SCENE_MAX_ROWS == 1 << 24 and _lib.SCENE_MAX_NUM_POINT == 65536
    assert lib.conv3p_abi_version() == 5 and _lib.ABI_VERSION == 5
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"             # the launches are outside the bracket
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conv3p.h")).read()
    assert "#define CONV3P_SCENE_MAX_CELLS 65536" in header
    for n in NAMES:
        assert n + "(" in header
    for n in ("scene_blocks", "SceneBlocks", "SceneVotes", "default_max_blocks"):
        assert n in pointwise_amd.__all__ and getattr(pointwise_amd, n) is getattr(scene, n)


def _blocks(**kw):
    a = dict(data=P, labels=P, N=1000, K=6, lb=1, block=1.0, stride=1.0, P=256, minp=100, maxb=8, seed=1, step=2, out=P,
             lout=P, iout=P, cell=P, cnt=P, stats=P, ws=P, wsb=1 << 40)
    a.update(kw)
    return _lib.load().conv3p_scene_blocks_f32(*[a[k] for k in (
        "data", "labels", "N", "K", "lb", "block", "stride", "P", "minp", "maxb", "seed", "step", "out", "lout", "iout",
        "cell", "cnt", "stats", "ws", "wsb")], None)


def test_blocks_status_codes_and_their_order():
    f = _lib.load().conv3p_scene_blocks_workspace_bytes
    for kw in (dict(N=-1), dict(K=2), dict(P=0), dict(P=-3), dict(maxb=-1), dict(block=0.0), dict(block=-1.0),
               dict(stride=0.0), dict(stride=-0.5), dict(block=float("nan")), dict(block=float("inf")),
               dict(stride=float("nan")), dict(stride=float("inf")), dict(lb=2), dict(lb=0), dict(lb=16),
               dict(labels=None), dict(lout=None)):
        assert _blocks(**kw) == INV, kw
        assert _blocks(N=0, **{k: v for k, v in kw.items() if k != "N"}) == (OK if "N" in kw else INV), kw   # before N == 0
    assert _blocks(labels=None, lout=None, lb=77, ws=None) == WS             # no labels: label_bytes is not looked at
    nothing = dict(data=None, labels=None, out=None, lout=None, iout=None, cell=None, cnt=None, stats=None, ws=None, wsb=0)
    assert _blocks(N=0, **nothing) == OK and _blocks(maxb=0, **nothing) == OK
    assert _blocks(N=0, P=1 << 20, **nothing) == OK                          # OK for nothing to do comes before UNSUPPORTED
    for name in ("data", "out", "iout", "cell", "cnt", "stats"):
        assert _blocks(**{name: None}) == INV, name
        assert _blocks(N=(1 << 24) + 1, **{name: None}) == INV               # INVALID before UNSUPPORTED
    for kw in (dict(N=(1 << 24) + 1), dict(P=65537), dict(block=0.5, stride=1.0), dict(block=2.5, stride=1.0),
               dict(K=65537)):
        assert _blocks(**kw) == UNS, kw
        assert _blocks(ws=None, wsb=0, **kw) == UNS, kw                      # UNSUPPORTED before WORKSPACE
    for kw in (dict(), dict(N=1 << 24, P=65536), dict(block=1.0, stride=0.5), dict(block=2.0, stride=1.0), dict(N=1, P=1)):
        a = dict(N=1000, P=256, maxb=8, block=1.0, stride=1.0)
        a.update(kw)
        need = f(a["N"], a["P"], a["maxb"], a["block"], a["stride"])
        assert need > 0
        assert _blocks(wsb=need - 1, **kw) == WS and _blocks(ws=None, **kw) == WS
        assert _blocks(ws=ctypes.c_void_p(4096 + 8), **kw) == WS             # misaligned


def test_vote_status_codes_and_their_order():
    lib = _lib.load()
    v, l, nbytes = lib.conv3p_scene_vote, lib.conv3p_scene_vote_labels, lib.conv3p_scene_vote_labels_workspace_bytes
    assert v(P, P, 10, -1, 13, P, None) == INV and v(P, P, 10, 5, 0, P, None) == INV
    assert v(None, None, 0, -1, 13, None, None) == INV                       # before rows == 0
    assert v(None, None, 0, 5, 13, None, None) == OK and v(None, None, 10, 0, 13, None, None) == OK
    assert v(None, P, 10, 5, 13, P, None) == INV and v(P, None, 10, 5, 13, P, None) == INV
    assert v(P, P, 10, 5, 13, None, None) == INV
    assert v(P, P, 10, 1 << 31, 13, P, None) == UNS and v(None, P, 10, 1 << 31, 13, P, None) == INV
    assert l(P, -1, 13, P, P, P, 1 << 20, None) == INV and l(P, 5, 0, P, P, P, 1 << 20, None) == INV
    assert l(None, 0, 13, None, None, None, 0, None) == OK
    for args in ((None, 5, 13, P, P), (P, 5, 13, None, P), (P, 5, 13, P, None)):
        assert l(*args, P, 1 << 20, None) == INV
    assert l(P, 1 << 31, 13, P, P, P, 1 << 20, None) == UNS and l(P, 1 << 31, 13, P, P, None, 0, None) == UNS
    need = nbytes(5, 13)
    assert need > 0 and need % 256 == 0 and nbytes(1 << 24, 41) % 256 == 0 and nbytes(1 << 24, 41) >= need
    assert nbytes(0, 13) == 0 and nbytes(-1, 13) == 0 and nbytes(5, 0) == 0 and nbytes(1 << 31, 13) == 0
    assert l(P, 5, 13, P, P, P, need - 1, None) == WS and l(P, 5, 13, P, P, None, need, None) == WS


def test_blocks_workspace_bytes():
    f = _lib.load().conv3p_scene_blocks_workspace_bytes
    for args in ((0, 256, 8, 1.0, 1.0), (-1, 256, 8, 1.0, 1.0), ((1 << 24) + 1, 256, 8, 1.0, 1.0), (1000, 0, 8, 1.0, 1.0),
                 (1000, 65537, 8, 1.0, 1.0), (1000, 256, 0, 1.0, 1.0), (1000, 256, -1, 1.0, 1.0), (1000, 256, 8, 0.0, 1.0),
                 (1000, 256, 8, 1.0, 0.0), (1000, 256, 8, float("nan"), 1.0), (1000, 256, 8, 1.0, float("inf")),
                 (1000, 256, 8, 0.5, 1.0), (1000, 256, 8, 2.5, 1.0), (1000, 256, 8, -1.0, -1.0)):
        assert f(*args) == 0, args
    for block, stride, m in ((1.0, 1.0, 2), (1.0, 0.5, 3), (1.5, 1.0, 3), (2.0, 1.0, 3)):
        for maxb in (1, 8, 1000, 65536, 1 << 20):
            Ns = (1, 255, 256, 257, 3000, 4096, 4097, 70000, 1 << 20, (1 << 20) + 1, 3000000, 1 << 24)
            sizes = [f(N, 4096, maxb, block, stride) for N in Ns]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
            assert all(s >= N * m * m * 4 + 65536 * 4 for s, N in zip(sizes, Ns))   # the member lists and the cell counts
        sizes = [f(70000, 4096, maxb, block, stride) for maxb in (1, 2, 100, 65536)]
        assert sizes == sorted(sizes)
    assert f(1000, 1, 8, 1.0, 1.0) == f(1000, 65536, 8, 1.0, 1.0)            # the output is not in the workspace


def test_python_checks_come_before_device_work():
    x = torch.zeros(50, 6)                                                   # on the CPU: a good call gets to the device check
    lab = torch.zeros(50, dtype=torch.uint8)
    bad = [dict(data=torch.zeros(50, 2)), dict(data=torch.zeros(50, 6, dtype=torch.float64)), dict(data=torch.zeros(2, 50, 6)),
           dict(data=np.zeros((50, 6), np.float32)), dict(data=torch.zeros(50, 12)[:, ::2]),
           dict(labels=torch.zeros(50)), dict(labels=torch.zeros(49, dtype=torch.uint8)),
           dict(labels=torch.zeros(50, 1, dtype=torch.int64)), dict(num_point=0), dict(num_point=65537), dict(num_point=2.5),
           dict(block=0.0), dict(block=float("nan")), dict(stride=-1.0), dict(stride=float("inf")), dict(block=1.0, stride=2.0),
           dict(block=2.5, stride=1.0), dict(max_blocks=-1), dict(max_blocks=1.5), dict(min_points=1.5), dict(seed=-1),
           dict(step=1 << 64), dict(out=object())]
    for kw in bad:
        a = dict(data=x, labels=lab, num_point=16)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument) as e:
            scene.scene_blocks(**a)
        assert "HIP device" not in str(e.value), kw
    for kw in (dict(), dict(labels=None), dict(stride=0.5), dict(block=2.0), dict(max_blocks=0), dict(max_blocks=3, min_points=0)):
        a = dict(data=x, labels=lab, num_point=16)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument, match="HIP device"):       # the "no CPU path" check comes last
            scene.scene_blocks(**a)
    for args in ((-1, 13), (5, 0), (5.0, 13), (1 << 31, 13)):
        with pytest.raises(Conv3pInvalidArgument) as e:
            scene.SceneVotes(*args, device="cpu")
        assert "HIP device" not in str(e.value)
    with pytest.raises(Conv3pInvalidArgument, match="HIP device"):
        scene.SceneVotes(5, 13, device="cpu")


def test_default_max_blocks_is_a_bound_from_the_shape():
    assert scene.default_max_blocks(3000) == 120 and scene.default_max_blocks(3000, 1.0, 0.5) == 270
    assert scene.default_max_blocks(3000, 1.0, 1.0, 0) == 12000 and scene.default_max_blocks(10) == 1
    assert scene.default_max_blocks(1 << 24, 1.0, 0.5, 1) == 65536
    for name, (N, seed, extent, stride, q) in FIXTURES.items():
        r = ref.scene_blocks_ref(ref.room(N, seed, extent, quantum=q), None, 16, 1.0, stride, 100, 1 << 16)
        assert r["stats"][1] <= scene.default_max_blocks(N, 1.0, stride, 100), name


FIXTURES = {"A": (3000, 2, (4.2, 3.1, 3.0), 1.0, None), "B": (3000, 2, (4.2, 3.1, 3.0), 0.5, None),
            "C": (1500, 3, (2.0, 2.0, 3.0), 0.5, 0.25), "D": (70000, 5, (6.3, 4.4, 3.0), 1.0, None)}


def test_fixture_shapes():
    """What tests/test_scene.py relies on, from the definition alone."""
    shapes = {}
    for name, (N, seed, extent, stride, q) in FIXTURES.items():
        r = ref.scene_blocks_ref(ref.room(N, seed, extent, quantum=q), None, 16, 1.0, stride, 100, 1 << 16)
        st = r["stats"]
        counts = np.array([len(m) for m in r["members"].values()])
        shapes[name] = (int(st[2]), int(st[3]), int(st[1]), int(st[2] * st[3] - st[1]), counts, r)
    nbx, nby, kept, dropped, counts, _ = shapes["A"]
    assert (nbx, nby, kept, dropped) == (5, 4, 11, 9)
    assert 250 in counts and 246 in counts and 322 in counts                # = P, < P, > P at P = 250
    nbx, nby, kept, dropped, counts, _ = shapes["B"]
    assert (nbx, nby, kept, dropped) == (8, 6, 31, 17)
    assert int((counts > 256).sum()) == 15 and int((counts < 256).sum()) == 16
    nbx, nby, kept, dropped, counts, r = shapes["C"]
    assert (nbx, nby, kept, dropped) == (3, 3, 9, 0)
    _, s, _, _ = ref.room_frame(ref.room(*FIXTURES["C"][:3], quantum=0.25))
    on_edge = np.isin(s[:, 0], [0.5, 1.0, 1.5]) | np.isin(s[:, 1], [0.5, 1.0, 1.5])
    assert int(on_edge.sum()) >= 200
    times = np.bincount(np.concatenate(list(r["members"].values())), minlength=1500)
    assert times.max() == 9
    nbx, nby, kept, dropped, counts, _ = shapes["D"]
    assert (nbx, nby, kept, dropped) == (7, 5, 35, 0)
    assert int(counts.sum()) == 70001


def _rooms():
    yield "A", ref.room(3000, 2, (4.2, 3.1, 3.0)), dict(num_point=250, stride=1.0)
    yield "C", ref.room(1500, 3, (2.0, 2.0, 3.0), quantum=0.25), dict(num_point=256, stride=0.5)
    small = ref.room(400, 7, (2.4, 1.7, 3.0))
    small[5, 0] = np.nan
    small[17, 2] = np.inf
    small[int(np.argmin(small[:, 0])), 1] = -np.inf
    yield "small", small, dict(num_point=32, stride=0.5, min_points=10)
    yield "K3", ref.room(300, 8, (1.5, 1.5, 3.0), K=3), dict(num_point=40, stride=1.0, min_points=0)
    yield "one", ref.room(1, 9, (1.0, 1.0, 3.0)), dict(num_point=8, stride=1.0, min_points=1)
    yield "none", np.full((7, 6), np.nan, np.float32), dict(num_point=8, stride=1.0, min_points=1)


@pytest.mark.parametrize("name,data,kw", list(_rooms()), ids=[r[0] for r in _rooms()])
def test_the_two_restatements_agree_and_indices_are_members(name, data, kw):
    labels = np.random.default_rng(11).integers(0, 13, size=data.shape[0]).astype(np.uint8)
    a = dict(num_point=64, block=1.0, stride=1.0, min_points=100, max_blocks=40, seed=5, step=3)
    a.update(kw)
    r1, r2 = ref.scene_blocks_ref(data, labels, **a), ref.scene_blocks_naive(data, labels, **a)
    for k in ("data", "labels", "index", "block_cell", "block_count", "stats"):
        assert np.array_equal(r1[k], r2[k], equal_nan=True), (name, k)
    assert r1["members"].keys() == r2["members"].keys()
    for c in r1["members"]:
        assert np.array_equal(r1["members"][c], r2["members"][c])
        assert np.all(np.diff(r1["members"][c]) > 0)
    nb = int(r1["stats"][0])
    assert nb == min(int(r1["stats"][1]), a["max_blocks"]) and (nb > 0 or name == "none")
    for b in range(nb):
        c, n = int(r1["block_cell"][b]), int(r1["block_count"][b])
        members = r1["members"][c]
        assert n == len(members) and np.isin(r1["index"][b], members).all()
        if n <= a["num_point"]:
            assert np.array_equal(r1["index"][b][:n], members)
        assert np.array_equal(r1["labels"][b], labels[r1["index"][b]].astype(np.int32))
    assert np.all(r1["index"][nb:] == -1) and np.all(r1["block_cell"][nb:] == -1) and not r1["data"][nb:].any()
    assert np.isfinite(r1["data"]).all()


def test_vote_restatement():
    votes = np.zeros((6, 4), np.int32)
    ref.vote_ref(votes, [0, 1, 1, 3, 4, -1, 2, 2], [0, 0, 0, 5, 2, 3, -1, 6], 4)
    assert votes.tolist() == [[1, 2, 0, 0], [0] * 4, [0] * 4, [0] * 4, [0] * 4, [0, 0, 0, 1]]
    votes[2] = [0, 3, 3, 1]
    lab, st = ref.vote_labels_ref(votes)
    assert lab.tolist() == [1, -1, 1, -1, -1, 3] and st.tolist() == [3, 3]
