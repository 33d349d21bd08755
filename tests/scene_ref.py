"""numpy restatement of conv3p_scene_blocks_f32 / conv3p_scene_vote / conv3p_scene_vote_labels (include/conv3p.h, the
ten steps), twice: scene_blocks_ref with array operations per cell, scene_blocks_naive with Python loops over cells and
rows for small rooms.  The Philox is tests/cls_tail_ref.py's.  Every float operation is a single float32 one."""
import math

import numpy as np

from tests.cls_tail_ref import philox4x32_10

MAX_CELLS = 65536
F = np.float32


def cells_along(lim, block, stride):
    q = math.ceil((float(lim) - float(block)) / float(stride)) + 1.0 if math.isfinite(float(lim)) else math.inf
    q = min(q, 2.0 ** 30)
    return 1 if q < 1.0 else int(q)


def draw_members(c, n, P, seed, step):
    """Member number of every slot of cell c, as if all P slots were draws."""
    ctr = np.zeros((P, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(P, dtype=np.uint32)
    ctr[:, 1] = np.uint32(0x80000000 | c)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(step >> 32)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (P, 2))
    w = philox4x32_10(ctr, key)[:, 0].astype(np.uint64)
    return ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def room_frame(data):
    """Steps 1-2 -> (finite mask, s (N, 3) float32 (garbage on other rows), lo, lim)."""
    xyz = np.asarray(data)[:, 0:3].astype(F)
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return fin, np.zeros_like(xyz), np.zeros(3, F), np.zeros(3, F)
    lo = xyz[fin].min(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        s = xyz - lo[None, :]
        lim = s[fin].max(axis=0)
    return fin, s, lo, lim


def _empty(max_blocks, P, K, with_labels):
    return {"data": np.zeros((max_blocks, P, K + 3), F), "labels": np.full((max_blocks, P), -1, np.int32) if with_labels else None,
            "index": np.full((max_blocks, P), -1, np.int32), "block_cell": np.full(max_blocks, -1, np.int32),
            "block_count": np.zeros(max_blocks, np.int32), "stats": np.zeros(8, np.int32), "members": {}}


def _emit(res, b, c, members, data, labels, s, lim, block, P, seed, step):
    n = len(members)
    slots = np.arange(P)
    m = draw_members(c, n, P, seed, step)
    if n <= P:
        m = np.where(slots < n, slots, m)
    rows = members[m]
    K = data.shape[1]
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
    res["block_count"][b] = n


def scene_blocks_ref(data, labels, num_point, block, stride, min_points, max_blocks, seed=0, step=0):
    """-> dict of data, labels, index, block_cell, block_count, stats and members {cell: its member rows, ascending}."""
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    P, block, stride = int(num_point), F(block), F(stride)
    res = _empty(max_blocks, P, K, labels is not None)
    fin, s, lo, lim = room_frame(data)
    st = res["stats"]
    st[4] = int((~fin).sum())
    if not fin.any():
        return res
    nbx, nby = cells_along(lim[0], block, stride), cells_along(lim[1], block, stride)
    st[2], st[3] = nbx, nby
    if nbx * nby > MAX_CELLS:
        st[7] = 1
        return res
    need = max(1, int(min_points))
    xbeg = np.arange(nbx).astype(F) * stride
    ybeg = np.arange(nby).astype(F) * stride
    xend, yend = xbeg + block, ybeg + block
    rows_x = [np.flatnonzero(fin & (xbeg[i] <= s[:, 0]) & (s[:, 0] <= xend[i])) for i in range(nbx)]
    b = kept = small = 0
    for i in range(nbx):
        rx = rows_x[i]
        sy = s[rx, 1]
        for j in range(nby):
            c = i * nby + j
            members = rx[(ybeg[j] <= sy) & (sy <= yend[j])]
            n = len(members)
            if n >= need:
                kept += 1
                res["members"][c] = members
                if b < max_blocks:
                    _emit(res, b, c, members, data, labels, s, lim, block, P, seed, step)
                    b += 1
            elif n > 0:
                small += 1
    st[0], st[1], st[5] = b, kept, small
    return res


def scene_blocks_naive(data, labels, num_point, block, stride, min_points, max_blocks, seed=0, step=0):
    """The same by Python loops over cells and rows: small rooms only."""
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    P, block, stride = int(num_point), F(block), F(stride)
    res = _empty(max_blocks, P, K, labels is not None)
    st = res["stats"]
    finite = [all(math.isfinite(float(data[r, a])) for a in range(3)) for r in range(N)]
    st[4] = N - sum(finite)
    rows = [r for r in range(N) if finite[r]]
    if not rows:
        return res
    lo = [min(data[r, a] for r in rows) for a in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((N, 3), F)
        for r in rows:
            for a in range(3):
                s[r, a] = data[r, a] - lo[a]
    lim = [max(s[r, a] for r in rows) for a in range(3)]
    nbx, nby = cells_along(lim[0], block, stride), cells_along(lim[1], block, stride)
    st[2], st[3] = nbx, nby
    if nbx * nby > MAX_CELLS:
        st[7] = 1
        return res
    need = max(1, int(min_points))
    b = kept = small = 0
    for i in range(nbx):
        xbeg = F(i) * stride
        xend = xbeg + block
        for j in range(nby):
            ybeg = F(j) * stride
            yend = ybeg + block
            members = np.array([r for r in rows if xbeg <= s[r, 0] <= xend and ybeg <= s[r, 1] <= yend], dtype=np.int64)
            n = len(members)
            if n >= need:
                kept += 1
                res["members"][i * nby + j] = members
                if b < max_blocks:
                    _emit(res, b, i * nby + j, members, data, labels, s, np.array(lim, F), block, P, seed, step)
                    b += 1
            elif n > 0:
                small += 1
    st[0], st[1], st[5] = b, kept, small
    return res


def vote_ref(votes, pred, index, num_class):
    """np.add.at of conv3p_scene_vote into votes (N, C), in place."""
    pred, index = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(index).reshape(-1).astype(np.int64)
    ok = (index >= 0) & (index < votes.shape[0]) & (pred >= 0) & (pred < num_class)
    np.add.at(votes, (index[ok], pred[ok]), 1)
    return votes


def vote_labels_ref(votes):
    """-> (labels int32 (N), int64 {voted, unvoted})."""
    most = votes.max(axis=1) if votes.shape[1] else np.zeros(votes.shape[0])
    lab = np.where(most > 0, votes.argmax(axis=1), -1).astype(np.int32)
    voted = int((lab >= 0).sum())
    return lab, np.array([voted, votes.shape[0] - voted], dtype=np.int64)


def room(N, seed, extent, K=6, quantum=None):
    """The tests' rooms: synth.room_like xyz (optionally rounded to multiples of `quantum`) and K - 3 random channels."""
    from pointwise_amd import synth
    xyz = synth.room_like(1, N, seed, extent)[0]
    if quantum:
        xyz = (np.round(xyz / quantum) * quantum).astype(F)
    extra = np.random.default_rng(seed + 1000).random((N, K - 3)).astype(F)
    return np.ascontiguousarray(np.concatenate([xyz, extra], axis=1))
