"""The covering mode of the scene partition on the device (-m gpu) against the numpy restatement of its definition
(tests/scene_cover_ref.py): every output compared with np.array_equal -- the contract is the bits, so there is no
tolerance anywhere in this file.  The fixtures are those whose shape
tests/test_scene_cover_host.py::test_fixture_shapes_and_the_covering_guarantee asserts from the definition alone."""
import numpy as np
import pytest

from tests import scene_cover_ref as cref
from tests import scene_ref as ref

KEYS = ("data", "labels", "index", "block_cell", "block_count", "stats")


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def run(dev, data, labels, a, out=None, cover=True):
    import torch
    from pointwise_amd import scene
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    lab = torch.from_numpy(labels).to(dev) if labels is not None else None
    return scene.scene_blocks(d, lab, out=out, cover=cover, **a)


def got_of(sb):
    return {k: (getattr(sb, k).cpu().numpy() if getattr(sb, k) is not None else None) for k in KEYS}


def check(got, want, what=""):
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cref.FIXTURES))
def test_fixtures_bit_for_bit(dev, name):
    data, labels, a, want = cref.fixture(name)
    sb = run(dev, data, labels, a)
    got = got_of(sb)
    check(got, want, name)
    got["members"] = want["members"]
    assert cref.check_cover(got, a["num_point"]) == cref.FIXTURES[name][2][2]      # the guarantee, on the device's output
    assert sb.num_blocks() == sb.blocks_needed() == cref.FIXTURES[name][2][2] and int(want["stats"][7]) == 0
    t = sb.trim()
    assert t.data.shape[0] == sb.num_blocks() and t.data.data_ptr() == sb.data.data_ptr()


def part_boundary_room():
    """Cells (i, 0), i = 0..3, of P, P + 1, 2 P and 2 P + 1 rows at P = 64, every row strictly inside its cell but the
    room's minimum corner; the rows shuffled."""
    rng = np.random.default_rng(64)
    rows = []
    for i, n in enumerate((64, 65, 128, 129)):
        xy = rng.uniform(0.125, 0.875, size=(n, 2))
        xy[:, 0] += i
        rows.append(xy)
    xy = np.concatenate(rows)
    xy[0] = 0.0
    xyz = np.concatenate([xy, rng.uniform(0, 3, size=(len(xy), 1))], axis=1)
    data = np.concatenate([xyz, rng.random((len(xy), 3))], axis=1).astype(np.float32)
    return np.ascontiguousarray(data[rng.permutation(len(data))])


@pytest.mark.gpu
def test_part_boundaries(dev):
    data = part_boundary_room()
    labels = (np.arange(data.shape[0]) % 13).astype(np.uint8)
    a = cref.call_args(dict(num_point=64, min_points=10, max_blocks=10))
    want = cref.cover_blocks_ref(data, labels, **a)
    assert [len(want["members"][c]) for c in sorted(want["members"])] == [64, 65, 128, 129]
    assert want["block_cell"].tolist() == [0, 1, 1, 2, 2, 3, 3, 3, -1, -1]
    assert want["block_count"].tolist() == [64, 32, 33, 64, 64, 43, 43, 43, 0, 0]
    assert want["stats"].tolist() == [8, 4, 4, 1, 0, 0, 8, 0]
    got = got_of(run(dev, data, labels, a))
    check(got, want, "part boundaries")
    got["members"] = want["members"]
    assert cref.check_cover(got, 64) == 8


@pytest.mark.gpu
def test_max_blocks_cuts_a_cell_between_parts(dev):
    data, labels, a, full = cref.fixture("A64")
    assert int(full["block_cell"][8]) == int(full["block_cell"][9])          # block 9 is a further part of block 8's cell
    for mb in (1, 9, 43, 50):
        b = dict(a, max_blocks=mb)
        want = cref.cover_blocks_ref(data, labels, **b)
        nb = min(mb, 44)
        assert int(want["stats"][0]) == nb and int(want["stats"][6]) == 44 and int(want["stats"][1]) == 11
        sb = run(dev, data, labels, b)
        got = got_of(sb)
        check(got, want, mb)
        assert (sb.num_blocks(), sb.blocks_needed()) == (nb, 44)
        assert np.array_equal(got["data"][:nb], full["data"][:nb])           # the first blocks of the full call
        assert np.all(got["index"][nb:] == -1) and np.all(got["labels"][nb:] == -1) and not got["data"][nb:].any()
        assert np.all(got["block_cell"][nb:] == -1) and np.all(got["block_count"][nb:] == 0)


@pytest.mark.gpu
def test_default_max_blocks_and_nothing_to_do(dev):
    import torch
    from pointwise_amd import scene
    data, labels, a, full = cref.fixture("B64")
    b = dict(a, max_blocks=None)
    sb = run(dev, data, labels, b)
    mb = scene.default_max_blocks(3000, 1.0, 0.5, 100, 64)
    assert sb.data.shape[0] == mb >= 130
    check(got_of(sb), cref.cover_blocks_ref(data, labels, **dict(a, max_blocks=mb)), "max_blocks=None")
    e = scene.scene_blocks(torch.zeros((0, 6), device=dev), None, num_point=4, max_blocks=2, cover=True)
    assert e.num_blocks() == 0 and e.blocks_needed() == 0 and e.index.tolist() == [[-1] * 4] * 2 and not e.data.any()
    z = run(dev, data, labels, dict(a, max_blocks=0))
    assert z.num_blocks() == 0 and tuple(z.data.shape) == (0, 64, 9)


@pytest.mark.gpu
def test_nonfinite_rows_including_the_extremes(dev):
    data, labels, a, _ = cref.fixture("A64")
    d = data.copy()
    order_x, order_y = np.argsort(d[:, 0]), np.argsort(d[:, 1])
    d[order_x[0], 0] = np.nan                                  # the room's extreme rows leave the bounds
    d[order_x[-1], 1] = np.inf
    d[order_y[0], 2] = -np.inf
    d[order_y[-1], 0] = -np.inf
    d[100:140, 2] = np.nan
    d[2000, 4] = np.nan                                        # a further channel does not make a row non-finite
    a = dict(a, max_blocks=48)
    want = cref.cover_blocks_ref(d, labels, **a)
    bad = ~np.isfinite(d[:, 0:3]).all(axis=1)
    assert int(want["stats"][4]) == int(bad.sum()) >= 42 and 0 < int(want["stats"][0]) == int(want["stats"][6]) <= 48
    got = got_of(run(dev, d, labels, a))
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=(k == "data")), k
    assert not np.isin(got["index"], np.flatnonzero(bad)).any()
    allnan = np.full((300, 6), np.nan, np.float32)
    w = cref.cover_blocks_ref(allnan, None, **a)
    assert w["stats"].tolist() == [0, 0, 0, 0, 300, 0, 0, 0]
    check(got_of(run(dev, allnan, None, a)), w, "no finite row")


@pytest.mark.gpu
def test_k3_and_the_label_types(dev):
    data, labels, a, want = cref.fixture("A250")
    for dt in (np.int32, np.int64):
        check(got_of(run(dev, data, labels.astype(dt), a)), want, dt)
    wide = labels.astype(np.int64) + (1 << 32) - 3            # the cast to int32 keeps the low word
    check(got_of(run(dev, data, wide, a)), cref.cover_blocks_ref(data, wide, **a), "int64 beyond int32")
    none = got_of(run(dev, data, None, a))
    assert none["labels"] is None
    for k in KEYS:
        if k != "labels":
            assert np.array_equal(none[k], want[k]), k
    xyz = np.ascontiguousarray(data[:, 0:3])
    check(got_of(run(dev, xyz, labels, a)), cref.cover_blocks_ref(xyz, labels, **a), "K = 3")


@pytest.mark.gpu
def test_reproducible_step_changes_draws_only_and_out_reuse(dev):
    data, labels, a, want = cref.fixture("A250")
    first = run(dev, data, labels, a)
    g1 = got_of(first)
    check(g1, want, "first")
    check(got_of(run(dev, data, labels, a)), g1, "two calls")               # bitwise reproducible
    b = dict(a, step=a["step"] + 1)
    w2 = cref.cover_blocks_ref(data, labels, **b)
    g2 = got_of(run(dev, data, labels, b))
    check(g2, w2, "another step")
    moved = 0
    for blk in range(int(want["stats"][0])):
        n = int(want["block_count"][blk])
        assert np.array_equal(g1["index"][blk, :n], g2["index"][blk, :n])   # the members stay
        moved += int((g1["index"][blk, n:] != g2["index"][blk, n:]).sum())
    assert moved > 0
    for k in ("block_cell", "block_count", "stats"):
        assert np.array_equal(g1[k], g2[k])
    again = run(dev, data, labels, b, out=first)                           # out=: the same tensors, written again
    assert again is first
    check(got_of(first), w2, "out reuse")
    plain = run(dev, data, labels, a, out=first, cover=False)              # ... and by the other mode, whose workspace is smaller
    assert plain is first
    check(got_of(first), ref.scene_blocks_ref(data, labels, **a), "out reuse by the plain mode")


@pytest.mark.gpu
def test_an_unsplit_room_equals_the_plain_mode(dev):
    data, labels, a, want = cref.fixture("A512")
    cover, plain = got_of(run(dev, data, labels, a)), got_of(run(dev, data, labels, a, cover=False))
    for k in ("data", "labels", "index", "block_cell", "block_count"):
        assert np.array_equal(cover[k], plain[k]), k
    assert cover["stats"].tolist() == plain["stats"].tolist()[:6] + [11, 0] and int(plain["stats"][6]) == 0
    check(plain, ref.scene_blocks_ref(data, labels, **a), "the plain mode")


@pytest.mark.gpu
def test_many_cells_and_too_many_cells(dev):
    data, labels, _, _ = cref.fixture("A64")
    # 8192 < cells <= 65536: the count pass leaves its LDS histogram; P = 2 splits most kept cells
    a = cref.call_args(dict(block=0.05, stride=0.03, min_points=3, num_point=2, max_blocks=700))
    want = cref.cover_blocks_ref(data, labels, **a)
    assert 8192 < int(want["stats"][2]) * int(want["stats"][3]) <= 65536
    assert 0 < int(want["stats"][1]) < int(want["stats"][0]) == 700 < int(want["stats"][6])
    check(got_of(run(dev, data, labels, a)), want, "many cells")
    b = cref.call_args(dict(block=0.01, stride=0.01, min_points=1, num_point=8, max_blocks=5))
    want = cref.cover_blocks_ref(data, labels, **b)
    assert want["stats"].tolist() == [0, 0] + want["stats"].tolist()[2:4] + [0, 0, 0, 1]
    got = got_of(run(dev, data, labels, b))
    check(got, want, "too many cells")
    assert not got["data"].any() and np.all(got["index"] == -1) and np.all(got["labels"] == -1)
