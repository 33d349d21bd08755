"""GPU tests (-m gpu) of the many-rooms tiling, scene.scene_blocks_rooms on conv3p_scene_blocks_rooms_f32: every output
bit for bit against tests/scene_rooms_ref.py (the single-room references concatenated) and against the device's own
single-room calls, degenerate rooms, the cuts of max_blocks, a member list longer than any tile of the sort, more cells
than the single call's LDS histogram, the three errors only the device knows, label types, reproducibility, and one vote
table over the rows of all rooms."""
import numpy as np
import pytest

from tests import scene_cover_ref as cref
from tests import scene_ref as base
from tests import scene_rooms_ref as rr

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def as_np(sb):
    g = lambda t: None if t is None else t.cpu().numpy()
    return {"data": g(sb.data), "labels": g(sb.labels), "index": g(sb.index), "block_cell": g(sb.block_cell),
            "block_count": g(sb.block_count), "block_room": g(sb.block_room), "room_blocks": g(sb.room_blocks),
            "room_stats": g(sb.room_stats), "stats": g(sb.stats)}


def run(data, rs, labels, device_rooms=False, **kw):
    import torch
    from pointwise_amd import scene
    dev = _dev()
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    r = torch.from_numpy(np.asarray(rs, dtype=np.int32)).to(dev) if device_rooms else rs
    return scene.scene_blocks_rooms(d, r, lab, **kw)


CASES = [(s, m, c) for c in (False, True) for s in (1.0, 0.5) for m in (100, 1)]


@pytest.mark.parametrize("stride,min_points,cover", CASES)
def test_three_rooms_against_the_reference(stride, min_points, cover):
    data, rs, labels = rr.three_rooms()
    a, mb, want = rr.three_rooms_ref(stride, min_points, cover)
    sb = run(data, rs, labels, max_blocks=mb + 3, cover=cover, **a)         # three fillers behind the emitted blocks
    want3 = rr.rooms_blocks_ref(data, labels, rs, max_blocks=mb + 3, cover=cover, **a)
    rr.assert_equal(as_np(sb), want3, "three rooms")
    assert sb.num_blocks() == mb and sb.blocks_needed() == (mb if cover else 0)
    t = sb.trim()
    assert t.data.shape[0] == mb and np.array_equal(t.block_room.cpu().numpy(), want["block_room"])
    for r in range(3):
        v = t.room(r)
        b0, b1 = int(want["room_blocks"][r]), int(want["room_blocks"][r + 1])
        assert np.array_equal(v.index.cpu().numpy(), want["index"][b0:b1]) and v.stats.tolist() == want["room_stats"][r].tolist()
    if cover and min_points == 1:                                            # every finite row of every room, once
        n = t.block_count.cpu().numpy()
        idx = t.index.cpu().numpy()
        seen = np.concatenate([idx[b, :n[b]] for b in range(mb)])
        assert np.array_equal(np.unique(seen), np.arange(data.shape[0]))


@pytest.mark.parametrize("stride,min_points,cover", CASES)
def test_three_rooms_against_the_single_room_calls_of_the_device(stride, min_points, cover):
    import torch
    from pointwise_amd import scene
    dev = _dev()
    data, rs, labels = rr.three_rooms()
    a, need, _ = rr.three_rooms_ref(stride, min_points, cover)
    for mb in (need, need - 3):
        got = as_np(run(data, rs, labels, device_rooms=True, max_blocks=mb, cover=cover, **a))
        first = 0
        for r in range(3):
            lo, hi = int(rs[r]), int(rs[r + 1])
            mbr = max(0, mb - first)
            one = scene.scene_blocks(torch.from_numpy(data[lo:hi]).to(dev), torch.from_numpy(labels[lo:hi]).to(dev),
                                     max_blocks=max(mbr, 1), cover=cover, **dict(a, seed=a["seed"] + r))
            st = one.stats.tolist()
            nb = min(st[0], mbr)
            b0 = int(got["room_blocks"][r])
            assert int(got["room_blocks"][r + 1]) - b0 == nb
            assert np.array_equal(got["data"][b0:b0 + nb].view(np.uint32), one.data[:nb].cpu().numpy().view(np.uint32))
            assert np.array_equal(got["index"][b0:b0 + nb] - lo, one.index[:nb].cpu().numpy())
            assert np.array_equal(got["labels"][b0:b0 + nb], one.labels[:nb].cpu().numpy())
            assert np.array_equal(got["block_cell"][b0:b0 + nb], one.block_cell[:nb].cpu().numpy())
            assert np.array_equal(got["block_count"][b0:b0 + nb], one.block_count[:nb].cpu().numpy())
            assert (got["block_room"][b0:b0 + nb] == r).all()
            assert got["room_stats"][r].tolist() == [nb] + st[1:]
            first += st[6] if cover else st[1]


def degenerate_rooms():
    """Empty rooms at the start, in the middle and at the end; a room of non-finite rows only; a normal room with some
    non-finite rows; a room whose +-3e38 rows overflow its extent (its own error) -- normal rooms between them."""
    a = base.room(**rr.ROOM_A)
    bad = base.room(5, 31, (1.0, 1.0, 1.0))
    bad[:, 0] = [np.inf, np.nan, -np.inf, np.nan, np.inf]
    mixed = base.room(800, 32, (2.4, 1.9, 3.0))
    mixed[7, 0], mixed[100, 1], mixed[799, 2], mixed[400, 0] = np.inf, np.nan, -np.inf, -np.inf
    huge = base.room(600, 33, (2.0, 2.0, 3.0))
    huge[5, 0], huge[6, 1] = 3e38, -3e38
    c = base.room(**rr.ROOM_C)
    return rr.concat([a[:0], a, bad, a[:0], mixed, huge, c, a[:0]])


@pytest.mark.parametrize("cover", [False, True])
def test_degenerate_rooms_among_normal_ones(cover):
    data, rs, labels = degenerate_rooms()
    a = rr.call_args(min_points=50, stride=0.5)
    need = rr.blocks_needed(rr.rooms_blocks_ref(data, None, rs, max_blocks=0, cover=cover, **a), cover)
    want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=need + 2, cover=cover, **a)
    ws = want["room_stats"]
    assert ws[0].tolist() == ws[3].tolist() == ws[7].tolist() == [0] * 8 and ws[2].tolist() == [0, 0, 0, 0, 5, 0, 0, 0]
    assert ws[4][4] == 4 and ws[4][0] > 0 and ws[5][7] == 1 and ws[5][0] == 0 and ws[6][0] > 0
    assert want["stats"][7] == 1 and want["stats"][4] == 9 and want["stats"][0] == need
    rr.assert_equal(as_np(run(data, rs, labels, max_blocks=need + 2, cover=cover, **a)), want, "degenerate rooms")


def test_max_blocks_cuts():
    data, rs, labels = rr.three_rooms()
    a, need, full = rr.three_rooms_ref(1.0, 100, False)
    rb = full["room_blocks"].tolist()
    assert rb == [0, 11, 11, 15]
    for mb in (11, 5, 13, 1):                 # between two rooms, inside the first room, inside the last, a single block
        want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=mb, cover=False, **a)
        rr.assert_equal(as_np(run(data, rs, labels, max_blocks=mb, cover=False, **a)), want, "plain cut at %d" % mb)
    # max_blocks below the first room's need: the later rooms have max_blocks_r = 0 and still report words 1-7
    assert want["room_stats"][2].tolist() == [0, 4, 2, 2, 0, 0, 0, 0] and want["room_blocks"].tolist() == [0, 1, 1, 1]
    a, need, full = rr.three_rooms_ref(1.0, 100, True)
    cell = full["block_cell"]
    inside = [b for b in range(1, need) if cell[b] == cell[b - 1] and full["block_room"][b] == full["block_room"][b - 1]]
    assert inside and full["room_blocks"].tolist() == [0, 44, 44, 74]
    for mb in (inside[0], inside[-1], 44, 3):  # between two parts of a cell (first room, last room), between two rooms
        want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=mb, cover=True, **a)
        assert want["stats"][0] == mb and want["stats"][6] == 74
        rr.assert_equal(as_np(run(data, rs, labels, max_blocks=mb, cover=True, **a)), want, "covering cut at %d" % mb)
    assert want["room_stats"][2].tolist() == [0, 4, 2, 2, 0, 0, 30, 0]


def test_a_member_list_longer_than_every_tile():
    """70000 rows in ONE cell, then room D: a list longer than a sort tile, a row tile and 65536."""
    one_cell = base.room(70000, 41, (0.9, 0.9, 3.0))
    one_cell[:, :2] = np.clip(one_cell[:, :2], 0.0, 0.9)                     # the walls' scatter stays inside the cell
    room_d, _, a_d, want_d = cref.fixture("D512")
    data, rs, labels = rr.concat([one_cell, room_d])
    a = rr.call_args(num_point=512)
    q = -(-70000 // 512)
    mb = q + 152
    sb = run(data, rs, labels, max_blocks=mb, cover=True, **a)
    got = as_np(sb)
    assert got["stats"].tolist() == [mb, 1 + 35, 2, 1 + 35, 0, 0, mb, 0] and got["room_blocks"].tolist() == [0, q, mb]
    n = got["block_count"]
    assert (got["block_cell"][:q] == 0).all() and n[:q].sum() == 70000
    assert np.array_equal(np.concatenate([got["index"][b, :n[b]] for b in range(q)]), np.arange(70000))
    # room D behind it: its single-room reference, the draws keyed seed + 1
    want = cref.cover_blocks_ref(room_d, labels[70000:], **dict(a_d, seed=a_d["seed"] + 1))
    assert np.array_equal(got["index"][q:] - 70000, want["index"]) and np.array_equal(got["labels"][q:], want["labels"])
    assert np.array_equal(got["data"][q:].view(np.uint32), want["data"].view(np.uint32))
    assert np.array_equal(got["block_cell"][q:], want["block_cell"]) and np.array_equal(n[q:], want["block_count"])
    assert got["room_stats"][1].tolist() == want["stats"].tolist()
    # and the one-cell room against the reference of its first and last blocks' own rows (the whole is `arange` above)
    first = cref.cover_blocks_ref(one_cell, labels[:70000], **dict(a, max_blocks=2))
    assert np.array_equal(got["data"][:2].view(np.uint32), first["data"][:2].view(np.uint32))
    assert np.array_equal(got["index"][:2], first["index"][:2])


def test_more_cells_than_the_single_calls_histogram():
    wide = base.room(20000, 42, (100.0, 100.0, 3.0))
    data, rs, labels = rr.concat([base.room(**rr.ROOM_A), wide])
    a = rr.call_args(min_points=1)
    need = rr.blocks_needed(rr.rooms_blocks_ref(data, None, rs, max_blocks=0, **a), False)
    want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=need + 1, **a)
    assert want["room_stats"][1][2] * want["room_stats"][1][3] > 8192 and want["room_stats"][1][1] > 4096
    rr.assert_equal(as_np(run(data, rs, labels, max_blocks=need + 1, **a)), want, "many cells")


def test_a_room_of_too_many_cells_between_two_normal_rooms():
    far = base.room(2, 43, (1.0, 1.0, 1.0))
    far[0, :2], far[1, :2] = (0.0, 0.0), (300.0, 300.0)
    data, rs, labels = rr.concat([base.room(**rr.ROOM_A), far, base.room(**rr.ROOM_C)])
    a = rr.call_args()
    want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=20, **a)
    assert want["room_stats"][1].tolist() == [0, 0, 300, 300, 0, 0, 0, 1] and want["stats"][7] == 1
    assert want["room_blocks"].tolist() == [0, 11, 11, 15]
    got = as_np(run(data, rs, labels, max_blocks=20, **a))
    assert got["stats"][7] & 1 and got["room_stats"][1][7] == 1
    rr.assert_equal(got, want, "error room")


def test_a_malformed_device_room_start():
    data, rs, labels = rr.three_rooms()
    N = data.shape[0]
    for bad in ([0, 3001, 3000, N], [0, 3000, 3001, N + 1], [-1, 3000, 3001, N]):
        want = rr.rooms_blocks_ref(data, labels, bad, max_blocks=6, **rr.call_args())
        got = as_np(run(data, bad, labels, device_rooms=True, max_blocks=6, **rr.call_args()))
        assert got["stats"][7] == 2 and not got["room_blocks"].any() and (got["block_room"] == -1).all()
        rr.assert_equal(got, want, "malformed room_start")


def test_too_many_cells_over_all_rooms():
    far = base.room(2, 44, (1.0, 1.0, 1.0))
    far[0, :2], far[1, :2] = (0.0, 0.0), (255.0, 255.0)
    data, rs, labels = rr.concat([far] * 17)
    want = rr.rooms_blocks_ref(data, labels, rs, max_blocks=4, **rr.call_args(min_points=1))
    assert want["stats"].tolist() == [0, 0, 17, 17 * 255 * 255, 0, 0, 0, 4]
    got = as_np(run(data, rs, labels, max_blocks=4, **rr.call_args(min_points=1)))
    assert got["stats"][7] & 4 and (got["index"] == -1).all() and not got["room_blocks"].any()
    rr.assert_equal(got, want, "too many cells")
    # sixteen rooms of 256 x 256 cells are exactly 2^20: no error.  Two kept cells of one member a room, so every slot of
    # a block is that member, whatever the draws
    far[1, :2] = (256.0, 256.0)
    data, rs, labels = rr.concat([far] * 16)
    got = as_np(run(data, rs, labels, max_blocks=40, **rr.call_args(min_points=1)))
    assert got["stats"].tolist() == [32, 32, 16, 1 << 20, 0, 0, 0, 0]
    assert got["room_blocks"].tolist() == list(range(0, 33, 2)) and (got["room_stats"] == [2, 2, 256, 256, 0, 0, 0, 0]).all()
    assert np.array_equal(got["index"][:32], np.broadcast_to(np.arange(32, dtype=np.int32)[:, None], (32, 64)))
    assert got["block_cell"][:32].tolist() == [0, 65535] * 16 and got["block_count"][:32].tolist() == [1] * 32
    assert got["block_room"].tolist() == [b // 2 for b in range(32)] + [-1] * 8 and (got["index"][32:] == -1).all()
    assert np.array_equal(got["labels"][:32, 0], labels.astype(np.int32))
    one = base.scene_blocks_ref(far, None, 64, 1.0, 1.0, 1, 2)
    for r in range(16):
        assert np.array_equal(got["data"][2 * r:2 * r + 2].view(np.uint32), one["data"].view(np.uint32))


@pytest.mark.parametrize("dtype", [None, np.int32, np.int64])
def test_three_channels_without_labels_and_wide_labels(dtype):
    data, rs, labels = rr.three_rooms()
    a, mb, _ = rr.three_rooms_ref(0.5, 100, True)
    if dtype is None:
        data, lab = np.ascontiguousarray(data[:, :3]), None
    else:
        lab = (labels.astype(np.int64) * 1000003 - 5).astype(dtype)         # int64 values are cast to int32 by the call
    want = rr.rooms_blocks_ref(data, lab, rs, max_blocks=mb, cover=True, **a)
    rr.assert_equal(as_np(run(data, rs, lab, max_blocks=mb, cover=True, **a)), want, str(dtype))


def test_reproducible_and_another_step_changes_the_draws_only():
    import torch
    from pointwise_amd import scene
    data, rs, labels = rr.three_rooms()
    a, mb, _ = rr.three_rooms_ref(1.0, 1, False)
    P = a["num_point"]
    one = run(data, rs, labels, max_blocks=mb + 2, **a)
    first = as_np(one)
    rr.assert_equal(as_np(run(data, rs, labels, max_blocks=mb + 2, **a)), first, "second call")
    other = as_np(run(data, rs, labels, max_blocks=mb + 2, **dict(a, step=a["step"] + 1)))
    for k in ("block_cell", "block_count", "block_room", "room_blocks", "room_stats", "stats"):
        assert np.array_equal(other[k], first[k]), k
    n = first["block_count"]
    changed = False
    for b in range(mb):
        if n[b] <= P:
            assert np.array_equal(other["index"][b, :n[b]], first["index"][b, :n[b]])
        changed = changed or not np.array_equal(other["index"][b], first["index"][b])
    assert changed and (n[:mb] <= P).any() and (n[:mb] > P).any()
    # out= reuse: the buffers of the first call, poisoned, written again
    dev = one.data.device
    for t in (one.data, one.index, one.labels, one.block_cell, one.block_count, one.block_room, one.room_blocks,
              one.room_stats, one.stats, one.workspace):
        t.fill_(77)
    again = scene.scene_blocks_rooms(torch.from_numpy(data).to(dev), rs, torch.from_numpy(labels).to(dev),
                                     max_blocks=mb + 2, out=one, **a)
    assert again is one
    rr.assert_equal(as_np(again), first, "out= reuse")


def test_one_vote_table_over_the_rows_of_all_rooms():
    import torch
    from pointwise_amd import scene
    dev = _dev()
    data, rs, labels = rr.three_rooms()
    data = data.copy()
    data[10, 0], data[3500, 1] = np.nan, np.inf                              # a row of room A and one of room C
    N, C = data.shape[0], 13
    a = rr.call_args(min_points=1)
    sb = run(data, rs, labels, cover=True, **a).trim()
    assert sb.stats[7].item() == 0 and sb.num_blocks() == sb.blocks_needed()
    lab = sb.labels.long().clamp(min=0)
    logits = torch.full(tuple(sb.index.shape) + (C,), -4.0, dtype=torch.float32, device=dev)
    logits.scatter_(2, lab.unsqueeze(-1), 6.0)                               # one-hot-ish: the row's own label wins
    scores = scene.SceneScores(N, C, dev)
    scores.add(logits.contiguous(), sb.index.contiguous())
    got = scores.labels().cpu().numpy()
    finite = np.isfinite(data[:, :3]).all(axis=1)
    assert (got[finite] >= 0).all() and (got[~finite] == -1).all() and (~finite).sum() == 2
    assert np.array_equal(got[finite], labels[finite].astype(np.int32))
    assert scores.counts().tolist() == [N - 2, 2]
