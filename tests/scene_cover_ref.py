"""numpy restatement of the covering mode (conv3p_scene_blocks_cover_f32: include/conv3p.h, steps 5', 7', 9', 10') and of
the votes by summed probabilities (conv3p_scene_vote_scores_f32, conv3p_scene_score_labels).  The partition twice:
cover_blocks_ref with array operations per block, cover_blocks_naive with Python loops over cells, parts and slots for
small rooms.  Steps 1-4, 6 and 8 are tests/scene_ref.py's; the covering mode has no counterpart in the reference tree,
so the definition in the header is the reference."""
import math

import numpy as np

from tests import scene_ref as base
from tests.cls_tail_ref import philox4x32_10

F = np.float32
SCALE = 1 << 30


def parts_of(n, P):
    """[(a_j, n_j)] of a cell of n members: q = ceil(n / P) parts, a_j = floor(j n / q)."""
    q = -(-n // P)
    a = [j * n // q for j in range(q + 1)]
    return [(a[j], a[j + 1] - a[j]) for j in range(q)]


def part_members(c, j, nj, P, seed, step):
    """Member number WITHIN the part of every slot of part j of cell c: slot t < n_j -> t, else the draw."""
    ctr = np.zeros((P, 4), dtype=np.uint32)
    ctr[:, 0] = (np.arange(P, dtype=np.int64) + j * P).astype(np.uint32)
    ctr[:, 1] = np.uint32(0x80000000 | c)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(step >> 32)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (P, 2))
    w = philox4x32_10(ctr, key)[:, 0].astype(np.uint64)
    draw = ((w * np.uint64(nj)) >> np.uint64(32)).astype(np.int64)
    slots = np.arange(P)
    return np.where(slots < nj, slots, draw)


def _emit_rows(res, b, c, nj, rows, data, labels, s, lim, block):
    """Step 8 for the P room rows of block b (tests/scene_ref.py's _emit after its choice of rows)."""
    K = data.shape[1]
    P = len(rows)
    sx, sy, sz = s[rows, 0], s[rows, 1], s[rows, 2]
    h = F(block) * F(0.5)
    out = np.empty((P, K + 3), F)
    out[:, 0] = sx - (sx.min() + h)
    out[:, 1] = sy - (sy.min() + h)
    out[:, 2] = sz
    out[:, 3:K] = data[rows, 3:K]
    for a, v in enumerate((sx, sy, sz)):
        out[:, K + a] = v / lim[a] if lim[a] != 0 else F(0)
    res["data"][b] = out
    res["index"][b] = rows
    if labels is not None:
        res["labels"][b] = np.asarray(labels)[rows].astype(np.int32)
    res["block_cell"][b] = c
    res["block_count"][b] = nj


def _cells(data, block, stride, min_points, res):
    """Steps 1-5 through scene_ref: -> (s, lim, {kept cell: members}) -- no kept cell when nothing can be emitted; fills
    the stats words that do not depend on the mode."""
    plain = base.scene_blocks_ref(data, None, 1, block, stride, min_points, 0)
    st = res["stats"]
    st[1:6] = plain["stats"][1:6]
    st[7] = plain["stats"][7]
    fin, s, lo, lim = base.room_frame(data)
    return s, lim, plain["members"]


def cover_blocks_ref(data, labels, num_point, block, stride, min_points, max_blocks, seed=0, step=0):
    """-> dict of data, labels, index, block_cell, block_count, stats and members {kept cell: its member rows}."""
    data = np.ascontiguousarray(data, dtype=F)
    P, block, stride = int(num_point), F(block), F(stride)
    res = base._empty(max_blocks, P, data.shape[1], labels is not None)
    s, lim, members = _cells(data, block, stride, min_points, res)
    res["members"] = members
    b = 0
    for c in sorted(members):
        m = members[c]
        for j, (a, nj) in enumerate(parts_of(len(m), P)):
            if b < max_blocks:
                rows = m[a + part_members(c, j, nj, P, seed, step)]
                _emit_rows(res, b, c, nj, rows, data, labels, s, lim, block)
            b += 1
    res["stats"][0] = min(b, max_blocks)
    res["stats"][6] = b
    return res


def cover_blocks_naive(data, labels, num_point, block, stride, min_points, max_blocks, seed=0, step=0):
    """The same by Python loops over cells, parts and slots, on scene_blocks_naive's cells: small rooms only."""
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    P, block, stride = int(num_point), F(block), F(stride)
    res = base._empty(max_blocks, P, K, labels is not None)
    plain = base.scene_blocks_naive(data, None, 1, block, stride, min_points, 0)
    st = res["stats"]
    st[1:6] = plain["stats"][1:6]
    st[7] = plain["stats"][7]
    members = res["members"] = plain["members"]
    fin, s, lo, lim = base.room_frame(data)
    h = F(block) * F(0.5)
    b = 0
    for c in sorted(members):
        m = [int(r) for r in members[c]]
        n = len(m)
        q = int(math.ceil(n / P)) if n > P else 1
        for j in range(q):
            a0, a1 = (j * n) // q, ((j + 1) * n) // q
            nj = a1 - a0
            if b < max_blocks:
                rows = []
                for t in range(P):
                    if t < nj:
                        rows.append(m[a0 + t])
                        continue
                    ctr = np.array([[(j * P + t) & 0xFFFFFFFF, 0x80000000 | c, step & 0xFFFFFFFF, step >> 32]], dtype=np.uint32)
                    key = np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint32)
                    w = int(philox4x32_10(ctr, key)[0, 0])
                    rows.append(m[a0 + ((w * nj) >> 32)])
                bx = min(s[r, 0] for r in rows)
                by = min(s[r, 1] for r in rows)
                for t, r in enumerate(rows):
                    o = res["data"][b, t]
                    o[0] = s[r, 0] - (bx + h)
                    o[1] = s[r, 1] - (by + h)
                    o[2] = s[r, 2]
                    o[3:K] = data[r, 3:K]
                    for a in range(3):
                        o[K + a] = s[r, a] / lim[a] if lim[a] != 0 else F(0)
                    res["index"][b, t] = r
                    if labels is not None:
                        res["labels"][b, t] = np.int32(np.asarray(labels)[r])
                res["block_cell"][b] = c
                res["block_count"][b] = nj
            b += 1
    st[0] = min(b, max_blocks)
    st[6] = b
    return res


def shape_of(r, P):
    """(kept cells, split cells, blocks needed, most parts) of a reference result."""
    counts = [len(m) for m in r["members"].values()]
    q = [-(-n // P) for n in counts]
    return len(counts), sum(1 for x in q if x > 1), sum(q), max(q) if q else 0


def check_cover(r, P):
    """The covering guarantee on an uncut result: the slots t < block_count[b] over the blocks of a cell are the cell's
    member list, each row exactly once, ascending; the remaining slots are rows of the block's own part."""
    st = r["stats"]
    assert int(st[0]) == int(st[6]), "the room was cut"
    nb, seen = int(st[0]), {}
    for b in range(nb):
        c, n = int(r["block_cell"][b]), int(r["block_count"][b])
        assert 1 <= n <= P
        seen.setdefault(c, []).append(r["index"][b, :n])
        assert np.isin(r["index"][b, n:], r["index"][b, :n]).all()
        assert b == 0 or int(r["block_cell"][b - 1]) <= c
    assert sorted(seen) == sorted(r["members"])
    for c, parts in seen.items():
        assert np.array_equal(np.concatenate(parts), r["members"][c]), c
        if len(parts) > 1:
            assert min(len(p) for p in parts) >= P // 2
    return nb


# ------------------------------------------------------------------------------------------------- the fixtures
# name: (room arguments, call arguments, (kept cells, split cells, blocks needed, most parts))
FIXTURES = {
    "A250": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=250), (11, 5, 16, 2)),
    "A64": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=64), (11, 11, 44, 6)),
    "A1": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=1), (11, 11, 2464, 322)),
    "A512": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=512), (11, 0, 11, 1)),
    "A64min1": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=64, min_points=1), (20, 16, 58, 6)),
    "B64": (dict(N=3000, seed=2, extent=(4.2, 3.1, 3.0)), dict(num_point=64, stride=0.5), (31, 31, 130, 7)),
    "C100": (dict(N=1500, seed=3, extent=(2.0, 2.0, 3.0), quantum=0.25), dict(num_point=100, stride=0.5), (9, 9, 47, 6)),
    "D512": (dict(N=70000, seed=5, extent=(6.3, 4.4, 3.0)), dict(num_point=512), (35, 31, 152, 14)),
}


def call_args(kw):
    a = dict(num_point=64, block=1.0, stride=1.0, min_points=100, max_blocks=None, seed=7, step=3)
    a.update(kw)
    return a


_CACHE = {}


def fixture(name):
    """(room, uint8 labels, call arguments, reference) of fixture `name`, max_blocks = the blocks it needs: computed
    once, never modified."""
    if name not in _CACHE:
        rk, ck, shape = FIXTURES[name]
        data = base.room(**rk)
        labels = np.random.default_rng(rk["seed"] + 50).integers(0, 13, size=data.shape[0]).astype(np.uint8)
        a = call_args(dict(ck, max_blocks=shape[2]))
        _CACHE[name] = (data, labels, a, cover_blocks_ref(data, labels, **a))
    return _CACHE[name]


# ------------------------------------------------------------------------------------- votes by summed probabilities
def softmax_fixed(logits):
    """int64 (rows, C): llrintf(p_c * 2^30) with the float32 steps of the definition (numpy's exp in float32 stands
    in for the device's expf: the restatement is held to the same bound as the device)."""
    x = np.asarray(logits, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        e = np.exp((x - m).astype(F)).astype(F)
        s = np.zeros((x.shape[0], 1), F)
        for c in range(x.shape[1]):
            s[:, 0] = s[:, 0] + e[:, c]
        p = (e / s).astype(F)
        return np.rint((p * F(SCALE)).astype(F)).astype(np.float64)


def voters(logits, index, N):
    """(rows that vote, rows with a valid index refused for a non-finite logit), boolean masks."""
    index = np.asarray(index).reshape(-1).astype(np.int64)
    x = np.asarray(logits, dtype=F).reshape(index.size, -1)
    inside = (index >= 0) & (index < N)
    fin = np.isfinite(x).all(axis=1)
    return inside & fin, inside & ~fin


def scores_ref64(logits, index, N):
    """-> (float64 (N, C) sums of the float64 softmax of the voting rows, votes per room row)."""
    index = np.asarray(index).reshape(-1).astype(np.int64)
    x = np.asarray(logits, dtype=np.float64).reshape(index.size, -1)
    ok, _ = voters(logits, index, N)
    xv = x[ok]
    e = np.exp(xv - xv.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    out = np.zeros((N, x.shape[1]), np.float64)
    np.add.at(out, index[ok], p)
    return out, np.bincount(index[ok], minlength=N)


SCORE_TOL = 32 * 2.0 ** -24 + 2.0 ** -31      # a vote: the float32 softmax (tests/test_seg_head.py's DACT_TOL) + the rounding


def score_labels_ref(scores):
    """-> (labels int32 (N), int64 {voted, unvoted}) of int64 scores."""
    most = scores.max(axis=1)
    lab = np.where(most > 0, scores.argmax(axis=1), -1).astype(np.int32)
    voted = int((lab >= 0).sum())
    return lab, np.array([voted, scores.shape[0] - voted], dtype=np.int64)


def score_labels_naive(scores):
    out = []
    for row in scores.tolist():
        best, most = -1, 0
        for c, v in enumerate(row):
            if v > most:
                best, most = c, v
        out.append(best)
    return np.array(out, dtype=np.int32)
