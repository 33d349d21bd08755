"""Scene tiling and voting on the device (-m gpu) against the numpy restatement of the definition (tests/scene_ref.py):
every output compared with np.array_equal -- the contract is the bits, so there is no tolerance anywhere in this file.
The rooms A-D are those whose shape tests/test_scene_host.py::test_fixture_shapes asserts from the definition alone."""
import numpy as np
import pytest

from tests import scene_ref as ref

NCLS = 13
ROOMS = {
    # name: (room arguments, call arguments)
    "A": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=250, stride=1.0, max_blocks=16)),
    "B": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=256, stride=0.5, max_blocks=40)),
    "C": (dict(N=1500, seed=3, extent=(2.0, 2.0, 3.0), quantum=0.25), dict(num_point=256, stride=0.5, max_blocks=12)),
    "D": (dict(N=70000, seed=5, extent=(6.3, 4.4, 3.0)), dict(num_point=512, stride=1.0, max_blocks=40)),
}
KEYS = ("data", "labels", "index", "block_cell", "block_count", "stats")


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def call_args(kw):
    a = dict(num_point=256, block=1.0, stride=1.0, min_points=100, max_blocks=16, seed=7, step=3)
    a.update(kw)
    return a


_CACHE = {}


def fixture(name):
    """(room, uint8 labels, call arguments, reference) of room `name`: computed once, never modified."""
    if name not in _CACHE:
        rk, ck = ROOMS[name]
        data = ref.room(**rk)
        labels = np.random.default_rng(rk["seed"] + 50).integers(0, NCLS, size=data.shape[0]).astype(np.uint8)
        a = call_args(ck)
        _CACHE[name] = (data, labels, a, ref.scene_blocks_ref(data, labels, **a))
    return _CACHE[name]


def run(dev, data, labels, a, out=None):
    import torch
    from pointwise_amd import scene
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    lab = torch.from_numpy(labels).to(dev) if labels is not None else None
    return scene.scene_blocks(d, lab, out=out, **a)


def got_of(sb):
    return {k: (getattr(sb, k).cpu().numpy() if getattr(sb, k) is not None else None) for k in KEYS}


def check(got, want, what=""):
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROOMS))
def test_rooms_bit_for_bit(dev, name):
    data, labels, a, want = fixture(name)
    sb = run(dev, data, labels, a)
    check(got_of(sb), want, name)
    nb = sb.num_blocks()
    assert nb == int(want["stats"][0]) == int(want["stats"][1]) and int(want["stats"][7]) == 0
    t = sb.trim()
    assert t.data.shape[0] == nb and t.index.shape[0] == nb and t.labels.shape[0] == nb and t.block_cell.shape[0] == nb
    assert t.data.data_ptr() == sb.data.data_ptr() and tuple(t.points.shape) == (nb, a["num_point"], 3)
    assert np.array_equal(sb.points.cpu().numpy(), want["data"][..., 0:3])


@pytest.mark.gpu
def test_k3_and_the_label_types(dev):
    data, labels, a, want = fixture("A")
    for dt in (np.int32, np.int64):
        check(got_of(run(dev, data, labels.astype(dt), a)), want, dt)
    wide = labels.astype(np.int64) + (1 << 32) - 3            # the cast to int32 keeps the low word
    w = ref.scene_blocks_ref(data, wide, **a)
    assert np.array_equal(w["labels"][w["index"] >= 0], (labels.astype(np.int32) - 3)[w["index"][w["index"] >= 0]])
    check(got_of(run(dev, data, wide, a)), w, "int64 beyond int32")
    none = got_of(run(dev, data, None, a))
    assert none["labels"] is None
    for k in KEYS:
        if k != "labels":
            assert np.array_equal(none[k], want[k]), k
    xyz = np.ascontiguousarray(data[:, 0:3])
    check(got_of(run(dev, xyz, labels, a)), ref.scene_blocks_ref(xyz, labels, **a), "K = 3")


@pytest.mark.gpu
def test_nonfinite_rows_including_the_extremes(dev):
    data, labels, a, _ = fixture("A")
    d = data.copy()
    order_x, order_y = np.argsort(d[:, 0]), np.argsort(d[:, 1])
    d[order_x[0], 0] = np.nan                                  # the room's extreme rows leave the bounds
    d[order_x[-1], 1] = np.inf
    d[order_y[0], 2] = -np.inf
    d[order_y[-1], 0] = -np.inf
    d[100:140, 2] = np.nan
    d[2000, 4] = np.nan                                        # a further channel does not make a row non-finite
    want = ref.scene_blocks_ref(d, labels, **a)
    bad = int((~np.isfinite(d[:, 0:3]).all(axis=1)).sum())
    assert int(want["stats"][4]) == bad >= 42 and int(want["stats"][0]) > 0
    got = got_of(run(dev, d, labels, a))
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=(k == "data")), k
    assert not np.isin(got["index"], np.flatnonzero(~np.isfinite(d[:, 0:3]).all(axis=1))).any()
    allnan = np.full((300, 6), np.nan, np.float32)
    w = ref.scene_blocks_ref(allnan, None, **a)
    assert w["stats"].tolist() == [0, 0, 0, 0, 300, 0, 0, 0]
    check(got_of(run(dev, allnan, None, a)), w, "no finite row")


@pytest.mark.gpu
def test_max_blocks_below_the_kept_cells(dev):
    data, labels, a, full = fixture("B")
    for mb in (1, 7):
        b = dict(a, max_blocks=mb)
        want = ref.scene_blocks_ref(data, labels, **b)
        assert int(want["stats"][0]) == mb and int(want["stats"][1]) == 31
        check(got_of(run(dev, data, labels, b)), want, mb)
        assert np.array_equal(want["data"], full["data"][:mb])             # the first blocks of the full call


@pytest.mark.gpu
def test_degenerate_rooms(dev):
    one = ref.room(1, 9, (1.0, 1.0, 3.0))
    same = np.repeat(ref.room(1, 10, (1.0, 1.0, 3.0)), 700, axis=0)
    for data, kw in ((one, dict(min_points=1, num_point=8)), (one, dict(min_points=0, num_point=1)),
                     (one, dict(min_points=2, num_point=8)), (same, dict(min_points=100, num_point=256)),
                     (same, dict(min_points=100, num_point=1024, stride=0.5))):
        a = call_args(dict(kw, max_blocks=3))
        lab = np.arange(data.shape[0]).astype(np.int32)
        want = ref.scene_blocks_ref(data, lab, **a)
        assert int(want["stats"][2]) == 1 and int(want["stats"][3]) == 1
        check(got_of(run(dev, data, lab, a)), want, kw)
        nb = int(want["stats"][0])
        assert nb == (0 if kw["min_points"] == 2 else 1)
        assert not want["data"][:nb, :, 6:9].any()                          # lim == 0: the normalised xyz is 0


@pytest.mark.gpu
def test_many_cells_and_too_many_cells(dev):
    data, labels, _, _ = fixture("A")
    # 8192 < cells <= 65536: the count pass leaves its LDS histogram
    a = call_args(dict(block=0.05, stride=0.03, min_points=3, num_point=8, max_blocks=300))
    want = ref.scene_blocks_ref(data, labels, **a)
    assert 8192 < int(want["stats"][2]) * int(want["stats"][3]) <= 65536 and 0 < int(want["stats"][0]) <= 300
    check(got_of(run(dev, data, labels, a)), want, "many cells")
    b = call_args(dict(block=0.01, stride=0.01, min_points=1, num_point=8, max_blocks=5))
    want = ref.scene_blocks_ref(data, labels, **b)
    assert want["stats"].tolist()[0:2] == [0, 0] and int(want["stats"][7]) == 1
    assert int(want["stats"][2]) * int(want["stats"][3]) > 65536
    got = got_of(run(dev, data, labels, b))
    check(got, want, "too many cells")
    assert not got["data"].any() and np.all(got["index"] == -1) and np.all(got["labels"] == -1)


@pytest.mark.gpu
def test_reproducible_step_changes_draws_only_and_out_reuse(dev):
    data, labels, a, want = fixture("A")
    first = run(dev, data, labels, a)
    g1 = got_of(first)
    check(got_of(run(dev, data, labels, a)), g1, "two calls")
    b = dict(a, step=a["step"] + 1)
    w2 = ref.scene_blocks_ref(data, labels, **b)
    g2 = got_of(run(dev, data, labels, b))
    check(g2, w2, "another step")
    P, moved = a["num_point"], 0
    for blk in range(int(want["stats"][0])):
        n = int(want["block_count"][blk])
        keep = min(n, P) if n <= P else 0
        assert np.array_equal(g1["index"][blk, :keep], g2["index"][blk, :keep])
        moved += int((g1["index"][blk, keep:] != g2["index"][blk, keep:]).sum())
    assert moved > 0
    for k in ("block_cell", "block_count", "stats"):
        assert np.array_equal(g1[k], g2[k])
    again = run(dev, data, labels, b, out=first)                           # out=: the same tensors, written again
    assert again is first
    check(got_of(first), w2, "out reuse")
    # an empty room and max_blocks == 0 launch nothing and still give the filler
    from pointwise_amd import scene
    import torch
    e = scene.scene_blocks(torch.zeros((0, 6), device=dev), None, num_point=4, max_blocks=2)
    assert e.num_blocks() == 0 and e.index.tolist() == [[-1] * 4] * 2 and not e.data.any()
    z = run(dev, data, labels, dict(a, max_blocks=0))
    assert z.num_blocks() == 0 and tuple(z.data.shape) == (0, 250, 9)


def _votes(dev, N, C, passes):
    import torch
    from pointwise_amd import scene
    sv = scene.SceneVotes(N, C, dev)
    want = np.zeros((N, C), np.int32)
    for pred, index in passes:
        sv.add(torch.from_numpy(pred).to(dev), torch.from_numpy(index).to(dev))
        ref.vote_ref(want, pred, index, C)
    return sv, want


@pytest.mark.gpu
@pytest.mark.parametrize("C", [13, 41])
def test_vote_against_numpy(dev, C):
    rng = np.random.default_rng(400 + C)
    N, rows = 5000, (7, 1000)
    passes = []
    for _ in range(2):                                                      # accumulation over two calls
        index = rng.integers(-1, N + 2, size=rows).astype(np.int32)        # -1 and past-the-end indices are ignored
        index[:, 0:300] = rng.integers(0, 40, size=(rows[0], 300))         # many votes on few rows
        pred = rng.integers(-2, C + 2, size=rows).astype(np.int32)         # out-of-range predictions are ignored
        passes.append((pred, index))
    sv, want = _votes(dev, N, C, passes[:1])
    assert np.array_equal(sv.votes.cpu().numpy(), want)
    lab1, st1 = ref.vote_labels_ref(want)
    assert np.array_equal(sv.labels().cpu().numpy(), lab1) and sv.counts().tolist() == st1.tolist()
    sv, want = _votes(dev, N, C, passes)
    assert np.array_equal(sv.votes.cpu().numpy(), want) and want.sum() > 0
    lab, st = ref.vote_labels_ref(want)
    assert (lab == -1).any() and st[0] > 0 and st[1] > 0
    assert sv.labels().dtype.is_floating_point is False
    assert np.array_equal(sv.labels().cpu().numpy(), lab) and sv.counts().tolist() == st.tolist()
    sv.reset()
    assert not sv.votes.any() and sv.counts().tolist() == [0, N] and np.all(sv.labels().cpu().numpy() == -1)


@pytest.mark.gpu
def test_vote_ties_and_unvoted_rows(dev):
    index = np.array([0, 0, 1, 1, 1, 1, 3, 3, 3, -1, 5], np.int32)
    pred = np.array([4, 2, 7, 3, 7, 3, 12, 0, 6, 1, 13], np.int32)          # row 5's only prediction is out of range
    sv, want = _votes(dev, 6, 13, [(pred, index)])
    assert np.array_equal(sv.votes.cpu().numpy(), want)
    assert sv.labels().tolist() == [2, 3, -1, 0, -1, -1] and sv.counts().tolist() == [3, 3]


@pytest.mark.gpu
def test_room_to_blocks_to_votes_to_confusion(dev):
    import torch
    from pointwise_amd import _lib
    data, labels, a, want = fixture("A")
    N = data.shape[0]
    sb = run(dev, data, labels, a)
    fake = np.random.default_rng(77).integers(0, NCLS, size=N).astype(np.int32)     # a fixed prediction per room row
    index = sb.index.cpu().numpy()
    pred = np.where(index >= 0, fake[np.maximum(index, 0)], 0).astype(np.int32)     # filler rows: ignored by their index
    sv, votes = _votes(dev, N, NCLS, [(pred, index)])
    assert np.array_equal(sv.votes.cpu().numpy(), votes)
    covered = np.zeros(N, bool)
    covered[index[index >= 0]] = True
    voted = sv.labels().cpu().numpy()
    assert np.array_equal(voted[covered], fake[covered]) and np.all(voted[~covered] == -1)
    assert sv.counts().tolist() == [int(covered.sum()), int((~covered).sum())] and 0 < covered.sum() < N
    lib = _lib.load()
    conf = torch.zeros((NCLS, NCLS), dtype=torch.int64, device=dev)
    nbytes = lib.conv3p_seg_confusion_workspace_bytes(N, NCLS)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    room_labels = torch.from_numpy(fake).to(dev)                                     # the room's labels: the fake truth
    assert lib.conv3p_seg_confusion(room_labels.data_ptr(), sv.labels().data_ptr(), N, NCLS, conf.data_ptr(), ws.data_ptr(),
                                    nbytes, torch.cuda.current_stream(dev).cuda_stream) == 0
    c = conf.cpu().numpy()
    assert np.array_equal(np.diag(c), np.bincount(fake[covered], minlength=NCLS)) and c.sum() == np.trace(c) == covered.sum()
