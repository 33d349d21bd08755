"""CPU tests (not gpu) of the covering mode and the votes by summed probabilities (include/conv3p.h:
conv3p_scene_blocks_cover_f32, conv3p_scene_vote_scores_f32, conv3p_scene_score_labels and their _bytes functions): the
symbols, the status codes and their order -- all decided before any HIP call, so bogus (never dereferenced) pointers are
fine -- the workspace sizes, the Python checks that come before device work, and the numpy restatement itself
(tests/scene_cover_ref.py): its two forms agree, the covering guarantee holds on the fixtures of
tests/test_scene_cover.py, and those fixtures have the shapes that file relies on."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import pointwise_amd
from pointwise_amd import _lib, scene
from pointwise_amd.conv3p_op import Conv3pInvalidArgument
from tests import scene_cover_ref as cref
from tests import scene_ref as ref

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
P = ctypes.c_void_p(4096)
NAMES = ("conv3p_scene_blocks_cover_workspace_bytes", "conv3p_scene_blocks_cover_f32", "conv3p_scene_vote_scores_f32",
         "conv3p_scene_score_labels_workspace_bytes", "conv3p_scene_score_labels")

FIXTURES, fixture = cref.FIXTURES, cref.fixture


def test_symbols_header_and_abi_version():
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    assert lib.conv3p_abi_version() == 5 and _lib.ABI_VERSION == 5          # additions do not move it
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"             # the launches are outside the bracket
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conv3p.h")).read()
    for n in NAMES:
        assert n + "(" in header
    assert "SceneScores" in pointwise_amd.__all__ and pointwise_amd.SceneScores is scene.SceneScores
    assert scene.SceneScores.SCALE == 1 << 30
    assert list(inspect.signature(scene.scene_blocks).parameters)[-2:] == ["out", "cover"]
    assert inspect.signature(scene.scene_blocks).parameters["cover"].default is False
    assert list(inspect.signature(scene.default_max_blocks).parameters)[-1] == "num_point"


def _blocks(**kw):
    a = dict(data=P, labels=P, N=1000, K=6, lb=1, block=1.0, stride=1.0, P=256, minp=100, maxb=8, seed=1, step=2, out=P,
             lout=P, iout=P, cell=P, cnt=P, stats=P, ws=P, wsb=1 << 40)
    a.update(kw)
    return _lib.load().conv3p_scene_blocks_cover_f32(*[a[k] for k in (
        "data", "labels", "N", "K", "lb", "block", "stride", "P", "minp", "maxb", "seed", "step", "out", "lout", "iout",
        "cell", "cnt", "stats", "ws", "wsb")], None)


def test_cover_status_codes_and_their_order():
    f = _lib.load().conv3p_scene_blocks_cover_workspace_bytes
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
    for kw in (dict(), dict(N=1 << 24, P=65536), dict(block=1.0, stride=0.5), dict(block=2.0, stride=1.0), dict(N=1, P=1),
               dict(maxb=1 << 20, P=1)):
        a = dict(N=1000, P=256, maxb=8, block=1.0, stride=1.0)
        a.update(kw)
        need = f(a["N"], a["P"], a["maxb"], a["block"], a["stride"])
        assert need > 0
        assert _blocks(wsb=need - 1, **kw) == WS and _blocks(ws=None, **kw) == WS
        assert _blocks(ws=ctypes.c_void_p(4096 + 8), **kw) == WS             # misaligned


def test_scores_status_codes_and_their_order():
    lib = _lib.load()
    v, l, nbytes = lib.conv3p_scene_vote_scores_f32, lib.conv3p_scene_score_labels, lib.conv3p_scene_score_labels_workspace_bytes
    assert v(P, P, 10, -1, 13, P, P, None) == INV and v(P, P, 10, 5, 0, P, P, None) == INV
    assert v(P, P, 10, 5, -4, P, P, None) == INV
    assert v(None, None, 0, -1, 13, None, None, None) == INV                 # before rows == 0
    assert v(None, None, 0, 5, 13, None, None, None) == OK and v(None, None, 10, 0, 13, None, None, None) == OK
    assert v(None, None, 0, 5, 129, None, None, None) == OK                  # OK for nothing to do comes before UNSUPPORTED
    for args in ((None, P, 10, 5, 13, P, P), (P, None, 10, 5, 13, P, P), (P, P, 10, 5, 13, None, P), (P, P, 10, 5, 13, P, None)):
        assert v(*args, None) == INV
    assert v(P, P, 10, 1 << 31, 13, P, P, None) == UNS and v(None, P, 10, 1 << 31, 13, P, P, None) == INV
    assert v(P, P, 10, 5, 129, P, P, None) == UNS and v(P, P, 10, 5, 129, None, P, None) == INV
    assert l(P, -1, 13, P, P, P, 1 << 20, None) == INV and l(P, 5, 0, P, P, P, 1 << 20, None) == INV
    assert l(None, 0, 13, None, None, None, 0, None) == OK
    for args in ((None, 5, 13, P, P), (P, 5, 13, None, P), (P, 5, 13, P, None)):
        assert l(*args, P, 1 << 20, None) == INV
    assert l(P, 1 << 31, 13, P, P, P, 1 << 20, None) == UNS and l(P, 1 << 31, 13, P, P, None, 0, None) == UNS
    assert l(P, 5, 129, P, P, None, 0, None) == UNS
    need = nbytes(5, 13)
    assert need > 0 and need % 256 == 0 and nbytes(1 << 24, 128) % 256 == 0 and nbytes(1 << 24, 128) >= need
    assert nbytes(0, 13) == 0 and nbytes(-1, 13) == 0 and nbytes(5, 0) == 0 and nbytes(1 << 31, 13) == 0
    assert nbytes(5, 129) == 0
    assert l(P, 5, 13, P, P, P, need - 1, None) == WS and l(P, 5, 13, P, P, None, need, None) == WS


def test_cover_workspace_bytes():
    f, plain = _lib.load().conv3p_scene_blocks_cover_workspace_bytes, _lib.load().conv3p_scene_blocks_workspace_bytes
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
            # the member lists, the cell counts and a table entry per block
            assert all(s >= N * m * m * 4 + 65536 * 4 + maxb * 16 for s, N in zip(sizes, Ns))
            assert all(s > plain(N, 4096, maxb, block, stride) for s, N in zip(sizes, Ns))
        sizes = [f(70000, 4096, maxb, block, stride) for maxb in (1, 2, 100, 65536, 65537, 1 << 20, (1 << 31) - 1)]
        assert sizes == sorted(sizes) and sizes[-2] < sizes[-1]             # blocks past the cells still need the table
    assert f(1000, 1, 8, 1.0, 1.0) == f(1000, 65536, 8, 1.0, 1.0)            # the output is not in the workspace


def test_python_checks_come_before_device_work():
    x = torch.zeros(50, 6)                                                   # on the CPU: a good call gets to the device check
    lab = torch.zeros(50, dtype=torch.uint8)
    bad = [dict(data=torch.zeros(50, 2)), dict(labels=torch.zeros(50)), dict(num_point=0), dict(num_point=65537),
           dict(block=1.0, stride=2.0), dict(max_blocks=-1), dict(min_points=1.5), dict(step=1 << 64), dict(out=object()),
           dict(cover=1), dict(cover=None), dict(cover="yes")]
    for kw in bad:
        a = dict(data=x, labels=lab, num_point=16, cover=True)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument) as e:
            scene.scene_blocks(**a)
        assert "HIP device" not in str(e.value), kw
    for kw in (dict(), dict(labels=None), dict(stride=0.5), dict(max_blocks=0), dict(max_blocks=3, min_points=0), dict(cover=False)):
        a = dict(data=x, labels=lab, num_point=16, cover=True)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument, match="HIP device"):       # the "no CPU path" check comes last
            scene.scene_blocks(**a)
    for args in ((-1, 13), (5, 0), (5.0, 13), (1 << 31, 13), (5, 129), (5, 13.0)):
        with pytest.raises(Conv3pInvalidArgument) as e:
            scene.SceneScores(*args, device="cpu")
        assert "HIP device" not in str(e.value)
    with pytest.raises(Conv3pInvalidArgument, match="HIP device"):
        scene.SceneScores(5, 13, device="cpu")


def test_default_max_blocks_with_num_point():
    d = scene.default_max_blocks
    assert d(3000) == 120 and d(3000, 1.0, 0.5) == 270                      # without num_point: as before
    assert d(3000, 1.0, 1.0, 100, 64) == 120 + 12000 // 64 and d(3000, 1.0, 0.5, 100, 64) == 270 + 27000 // 64
    assert d(3000, num_point=1) == 120 + 12000 and d(10, num_point=4096) == 1
    assert d(1 << 24, 1.0, 0.5, 1, 1) == 65536 + 9 * (1 << 24)
    for name in FIXTURES:
        data, _, a, want = fixture(name)
        assert int(want["stats"][6]) <= d(data.shape[0], a["block"], a["stride"], a["min_points"], a["num_point"]), name


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_shapes_and_the_covering_guarantee(name):
    """What tests/test_scene_cover.py relies on, from the definition alone."""
    data, labels, a, want = fixture(name)
    shape = FIXTURES[name][2]
    assert cref.shape_of(want, a["num_point"]) == shape
    assert int(want["stats"][6]) == shape[2] == int(want["stats"][0]) and int(want["stats"][1]) == shape[0]
    assert cref.check_cover(want, a["num_point"]) == shape[2]
    idx = want["index"]
    assert np.array_equal(want["labels"], labels[idx].astype(np.int32)) and np.isfinite(want["data"]).all()
    emitted = np.zeros(data.shape[0], bool)
    emitted[idx.reshape(-1)] = True
    in_kept = np.zeros(data.shape[0], bool)
    for m in want["members"].values():
        in_kept[m] = True
    assert np.array_equal(emitted, in_kept)                                  # every row of a kept cell is emitted
    if name == "A64min1":
        assert emitted.all()                                                 # all 3000 rows are in kept cells
        plain = ref.scene_blocks_ref(data, None, **dict(a, max_blocks=20))
        assert np.unique(plain["index"]).size == 911                         # what the plain mode shows the model
    if name == "A64":
        assert int(in_kept.sum()) == 2464
        assert np.unique(ref.scene_blocks_ref(data, None, **dict(a, max_blocks=11))["index"]).size == 600
    if name == "D512":
        assert int(in_kept.sum()) == 70000
        assert np.unique(ref.scene_blocks_ref(data, None, **dict(a, max_blocks=35))["index"]).size == 14657
    if name == "A512":                                                       # no cell exceeds P: the plain mode's outputs
        plain = ref.scene_blocks_ref(data, labels, **a)
        for k in ("data", "labels", "index", "block_cell", "block_count"):
            assert np.array_equal(plain[k], want[k]), k
        assert plain["stats"].tolist()[:6] == want["stats"].tolist()[:6] and int(plain["stats"][6]) == 0


def _rooms():
    yield "A", ref.room(3000, 2, (4.2, 3.1, 3.0)), dict(num_point=250, stride=1.0)
    yield "Acut", ref.room(3000, 2, (4.2, 3.1, 3.0)), dict(num_point=64, stride=1.0, max_blocks=9)
    yield "C", ref.room(1500, 3, (2.0, 2.0, 3.0), quantum=0.25), dict(num_point=100, stride=0.5, max_blocks=50)
    small = ref.room(400, 7, (2.4, 1.7, 3.0))
    small[5, 0] = np.nan
    small[17, 2] = np.inf
    small[int(np.argmin(small[:, 0])), 1] = -np.inf
    yield "small", small, dict(num_point=7, stride=0.5, min_points=10, max_blocks=200)
    yield "K3", ref.room(300, 8, (1.5, 1.5, 3.0), K=3), dict(num_point=40, stride=1.0, min_points=0)
    yield "P1", ref.room(60, 8, (1.5, 1.5, 3.0)), dict(num_point=1, stride=1.0, min_points=1, max_blocks=80)
    yield "one", ref.room(1, 9, (1.0, 1.0, 3.0)), dict(num_point=8, stride=1.0, min_points=1)
    yield "none", np.full((7, 6), np.nan, np.float32), dict(num_point=8, stride=1.0, min_points=1)


@pytest.mark.parametrize("name,data,kw", list(_rooms()), ids=[r[0] for r in _rooms()])
def test_the_two_restatements_agree(name, data, kw):
    labels = np.random.default_rng(11).integers(0, 13, size=data.shape[0]).astype(np.uint8)
    a = dict(num_point=64, block=1.0, stride=1.0, min_points=100, max_blocks=40, seed=5, step=3)
    a.update(kw)
    r1, r2 = cref.cover_blocks_ref(data, labels, **a), cref.cover_blocks_naive(data, labels, **a)
    for k in ("data", "labels", "index", "block_cell", "block_count", "stats"):
        assert np.array_equal(r1[k], r2[k], equal_nan=True), (name, k)
    assert r1["members"].keys() == r2["members"].keys()
    nb, need = int(r1["stats"][0]), int(r1["stats"][6])
    assert nb == min(need, a["max_blocks"]) and (nb > 0 or name == "none")
    assert need == sum(-(-len(m) // a["num_point"]) for m in r1["members"].values())
    if name == "Acut":
        assert nb < need and int(r1["block_cell"][nb - 1]) == int(r1["block_cell"][nb - 2])   # cut inside a cell
    else:
        assert cref.check_cover(r1, a["num_point"]) == nb
    assert np.all(r1["index"][nb:] == -1) and np.all(r1["block_cell"][nb:] == -1) and not r1["data"][nb:].any()
    assert np.all(r1["block_count"][nb:] == 0) and np.all(r1["labels"][nb:] == -1)


def test_parts_of_a_cell():
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 322, 4097, 1 << 24):
        for Pn in (1, 2, 64, 65, 4096, 65536):
            if n // Pn > 5000:
                continue
            parts = cref.parts_of(n, Pn)
            assert len(parts) == -(-n // Pn) and parts[0][0] == 0 and sum(nj for _, nj in parts) == n
            assert all(1 <= nj <= Pn for _, nj in parts)
            assert all(parts[j][0] + parts[j][1] == parts[j + 1][0] for j in range(len(parts) - 1))
            if len(parts) > 1:
                assert min(nj for _, nj in parts) >= Pn // 2
    assert cref.parts_of(64, 64) == [(0, 64)] and cref.parts_of(65, 64) == [(0, 32), (32, 33)]
    assert cref.parts_of(128, 64) == [(0, 64), (64, 64)] and cref.parts_of(129, 64) == [(0, 43), (43, 43), (86, 43)]


def test_scores_restatement():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((200, 13)) * 20).astype(np.float32)
    x[3] = 7.5                                                               # equal logits
    x[10, 4] = np.nan
    x[11, 0] = np.inf
    x[12, 12] = -np.inf
    index = rng.integers(-1, 42, size=200).astype(np.int32)                 # N = 40: -1, 40 and 41 do not vote
    index[10:13] = (1, 2, 50)
    ok, refused = cref.voters(x, index, 40)
    assert not ok[10:13].any() and refused[10:13].tolist() == [True, True, False]
    assert int(ok.sum()) == int(((index >= 0) & (index < 40)).sum()) - 2
    want, votes = cref.scores_ref64(x, index, 40)
    assert np.allclose(want.sum(axis=1), votes) and votes.sum() == ok.sum()
    fixed = np.zeros((40, 13), np.float64)
    np.add.at(fixed, index[ok].astype(np.int64), cref.softmax_fixed(x[ok]))
    assert np.all(np.abs(fixed / cref.SCALE - want) <= votes[:, None] * cref.SCORE_TOL)   # the restatement in the bound
    assert np.array_equal(cref.softmax_fixed(x[3:4]), np.rint(np.full((1, 13), np.float32(1) / np.float32(13)) * 2.0 ** 30))
    scores = np.array([[0, 0, 0], [5, 9, 9], [3, 3, 1], [0, 0, 1 << 40], [7, 0, 0]], np.int64)
    lab, st = cref.score_labels_ref(scores)
    assert lab.tolist() == [-1, 1, 0, 2, 0] and st.tolist() == [4, 1]
    assert np.array_equal(cref.score_labels_naive(scores), lab)
    big = rng.integers(0, 1 << 50, size=(300, 7))
    big[rng.random((300, 7)) < 0.5] = 0
    assert np.array_equal(cref.score_labels_naive(big), cref.score_labels_ref(big)[0])
