"""numpy restatement of conv3p_scene_blocks_rooms_f32 (include/conv3p.h, steps a-e): the concatenation of the single-room
references -- tests/scene_ref.py's scene_blocks_ref (plain) or tests/scene_cover_ref.py's cover_blocks_ref (covering),
run per room with the key seed + r and max_blocks_r -- with index moved to global rows, and block_room, room_blocks,
room_stats and stats built around them.  rooms_blocks_naive is the same over the _naive functions, for small rooms.
The minimum of step 2 is IEEE 754-2019's: -0.0 is below +0.0, as the device's min instruction takes them, so it does not
depend on the order of the reduction.  numpy's min over both zeros returns whichever its loop ends on, so while _rooms
calls the single-room references it puts a room_frame in their place that repairs the sign of a zero minimum (the
_naive functions take their own minimum: their rooms must not hold -0.0 at a minimum).  The replacement rebinds
scene_ref.room_frame for the time of the call and puts it back: it is global to the process and not thread-safe, so
nothing else may call tests/scene_ref.py from another thread meanwhile; the place for the IEEE minimum is
scene_ref.room_frame itself."""
import contextlib

import numpy as np

from tests import scene_cover_ref as cref
from tests import scene_ref as base

F = np.float32
ROOMS_MAX_CELLS = 1 << 20
MAX_ROOM_ROWS = 1 << 24


def malformed(room_start, N):
    rs = np.asarray(room_start, dtype=np.int64)
    d = np.diff(rs)
    return bool(rs[0] < 0 or rs[-1] > N or (d < 0).any() or (d > MAX_ROOM_ROWS).any())


_numpy_room_frame = base.room_frame


def room_frame(data):
    """scene_ref.room_frame with the IEEE 754-2019 minimum: a zero minimum is -0.0 if any finite row holds -0.0 there."""
    fin, s, lo, lim = _numpy_room_frame(data)
    if fin.any():
        xyz = np.asarray(data)[:, 0:3].astype(F)[fin]
        lo = lo.copy()
        for a in range(3):
            if lo[a] == 0:
                lo[a] = F(-0.0) if np.signbit(xyz[xyz[:, a] == 0, a]).any() else F(0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.asarray(data)[:, 0:3].astype(F) - lo[None, :]
            lim = s[fin].max(axis=0)
    return fin, s, lo, lim


@contextlib.contextmanager
def _ieee_minimum():
    base.room_frame = room_frame
    try:
        yield
    finally:
        base.room_frame = _numpy_room_frame


def _rooms_body(data, labels, room_start, num_point, block, stride, min_points, max_blocks, seed, step, cover, plain_fn, cover_fn):
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    rs = np.asarray(room_start, dtype=np.int64)
    R = rs.size - 1
    P = int(num_point)
    res = base._empty(max_blocks, P, K, labels is not None)
    del res["members"]
    res["block_room"] = np.full(max_blocks, -1, np.int32)
    res["room_blocks"] = np.zeros(R + 1, np.int32)
    res["room_stats"] = np.zeros((R, 8), np.int32)
    res["members"] = {}                                  # {(room, cell): global member rows}
    st = res["stats"]
    st[2] = R
    if malformed(rs, N):
        st[7] = 2
        return res
    fn = cover_fn if cover else plain_fn
    lab = None if labels is None else np.asarray(labels)
    # the rooms' own frames first: the sum of the cells decides whether anything is emitted at all
    frames = [fn(data[rs[r]:rs[r + 1]], None, 1, block, stride, min_points, 0) if rs[r + 1] > rs[r] else None
              for r in range(R)]
    cells = sum(int(f["stats"][2]) * int(f["stats"][3]) for f in frames if f is not None and not f["stats"][7])
    err = 1 if any(f is not None and f["stats"][7] for f in frames) else 0
    st[3] = min(cells, 2 ** 31 - 1)
    st[4] = sum(int(f["stats"][4]) for f in frames if f is not None)
    if cells > ROOMS_MAX_CELLS:
        st[7] = err | 4
        for r, f in enumerate(frames):
            if f is not None:
                res["room_stats"][r, [2, 3, 4, 7]] = f["stats"][[2, 3, 4, 7]]
        return res
    st[7] = err
    first = 0                                            # the blocks the rooms before r need
    for r in range(R):
        a, b = int(rs[r]), int(rs[r + 1])
        res["room_blocks"][r] = min(first, max_blocks)
        if b == a:
            continue
        mb = max(0, max_blocks - first)
        one = fn(data[a:b], None if lab is None else lab[a:b], P, block, stride, min_points, mb,
                 seed=(seed + r) % 2 ** 64, step=step)
        s1 = one["stats"]
        nb = int(s1[0])
        b0 = min(first, max_blocks)
        res["data"][b0:b0 + nb] = one["data"][:nb]
        res["index"][b0:b0 + nb] = one["index"][:nb] + a
        if lab is not None:
            res["labels"][b0:b0 + nb] = one["labels"][:nb]
        res["block_cell"][b0:b0 + nb] = one["block_cell"][:nb]
        res["block_count"][b0:b0 + nb] = one["block_count"][:nb]
        res["block_room"][b0:b0 + nb] = r
        res["room_stats"][r] = s1
        for c, m in one["members"].items():
            res["members"][(r, c)] = m + a
        first += int(s1[6]) if cover else int(s1[1])
        st[1] += s1[1]
        st[5] += s1[5]
    res["room_blocks"][R] = min(first, max_blocks)
    st[0] = min(first, max_blocks)
    st[6] = first if cover else 0
    return res


def _rooms(*args):
    with _ieee_minimum():
        return _rooms_body(*args)


def rooms_blocks_ref(data, labels, room_start, num_point, block, stride, min_points, max_blocks, seed=0, step=0, cover=False):
    return _rooms(data, labels, room_start, num_point, block, stride, min_points, max_blocks, seed, step, cover,
                  base.scene_blocks_ref, cref.cover_blocks_ref)


def rooms_blocks_naive(data, labels, room_start, num_point, block, stride, min_points, max_blocks, seed=0, step=0, cover=False):
    return _rooms(data, labels, room_start, num_point, block, stride, min_points, max_blocks, seed, step, cover,
                  base.scene_blocks_naive, cref.cover_blocks_naive)


def blocks_needed(res, cover):
    """The blocks all rooms need, from a reference result (the plain mode's stats[6] is 0 by definition)."""
    return int(res["room_stats"][:, 6].sum()) if cover else int(res["room_stats"][:, 1].sum())


KEYS = ("data", "labels", "index", "block_cell", "block_count", "block_room", "room_blocks", "room_stats", "stats")


def assert_equal(got, want, what=""):
    """np.array_equal on every output, data as bits."""
    for k in KEYS:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (what, k)
            continue
        if k == "data":
            g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        assert g.shape == w.shape and np.array_equal(g, w), (what, k)


# ------------------------------------------------------------------------------------------------- the fixtures
ROOM_A = dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0))
ROOM_C = dict(N=1500, seed=3, extent=(2.0, 2.0, 3.0), quantum=0.25)
ROOM_D = dict(N=70000, seed=5, extent=(6.3, 4.4, 3.0))

_CACHE = {}


def concat(rooms):
    """(data, room_start, uint8 labels) of rooms given as arrays (K columns each)."""
    data = np.ascontiguousarray(np.concatenate(rooms, axis=0), dtype=F)
    rs = np.concatenate([[0], np.cumsum([len(x) for x in rooms])]).astype(np.int32)
    labels = np.random.default_rng(77).integers(0, 13, size=data.shape[0]).astype(np.uint8)
    return data, rs, labels


def three_rooms():
    """Room A, a room of one row, room C: computed once, never modified."""
    if "three" not in _CACHE:
        one = base.room(1, 11, (1.0, 1.0, 1.0))
        _CACHE["three"] = concat([base.room(**ROOM_A), one, base.room(**ROOM_C)])
    return _CACHE["three"]


def call_args(**kw):
    a = dict(num_point=64, block=1.0, stride=1.0, min_points=100, seed=7, step=3)
    a.update(kw)
    return a


def three_rooms_ref(stride, min_points, cover, max_blocks=None):
    """The reference of the three-room fixture, max_blocks = what it needs unless given: computed once per case."""
    key = ("three", stride, min_points, cover, max_blocks)
    if key not in _CACHE:
        data, rs, labels = three_rooms()
        a = call_args(stride=stride, min_points=min_points)
        mb = max_blocks
        if mb is None:
            mb = blocks_needed(rooms_blocks_ref(data, None, rs, max_blocks=0, cover=cover, **a), cover)
        _CACHE[key] = (a, mb, rooms_blocks_ref(data, labels, rs, max_blocks=mb, cover=cover, **a))
    return _CACHE[key]
