"""numpy restatement of the interpolated projection (include/conv3p.h: conv3p_grid_neighbors rules N1-N4,
conv3p_grid_interpolate_f32 / _i64 rules 1-5).  Every float32 step is one numpy operation on np.float32 values (a column
of rows at a time) and the chains over the selected voxels are explicit loops, so the device is compared bit for bit."""
import numpy as np

F = np.float32
FLOOR = F(1e-10)
SCALE = F(2.0 ** -30)


def neighbors_ref(voxel_cell, num_voxels, voxel_room=None, voxel_start=None):
    """voxel_cell (max_voxels, 3), the emitted voxels first and in ascending (i_x, i_y, i_z) (per room with voxel_room /
    voxel_start) -> int32 (max_voxels, 27): a binary search for every neighbouring cell in the ascending cells, as the
    device does it (np.searchsorted on the triples packed into one integer, 21 bits a coordinate)."""
    cell = np.asarray(voxel_cell, np.int64)
    M = cell.shape[0]
    ne = max(0, min(int(num_voxels), M))
    out = np.full((M, 27), -1, np.int32)
    if voxel_room is None:
        spans = [(0, ne)]
    else:
        assert (np.asarray(voxel_room[:ne]) == np.repeat(np.arange(len(voxel_start) - 1), np.diff(np.minimum(voxel_start, ne)))).all()
        spans = [(max(0, int(a)), min(ne, int(b))) for a, b in zip(voxel_start[:-1], voxel_start[1:])]
    B = np.int64(1 << 21)
    for a, b in spans:
        if a >= b:
            continue
        c = cell[a:b] + 1                                  # 1 .. 2^20: a neighbour's coordinate is never negative
        keys = (c[:, 0] * B + c[:, 1]) * B + c[:, 2]
        assert (np.diff(keys) > 0).all()
        for t in range(27):
            want = keys + ((t // 9 - 1) * B + (t // 3) % 3 - 1) * B + t % 3 - 1
            pos = np.searchsorted(keys, want)
            hit = (pos < b - a) & (keys[np.minimum(pos, b - a - 1)] == want)
            out[a:b, t] = np.where(hit, a + pos, -1)
    return out


def neighbors_brute(voxel_cell, num_voxels, voxel_room=None):
    """The same table from a dictionary of the emitted cells."""
    cell = np.asarray(voxel_cell, np.int64)
    M = cell.shape[0]
    ne = max(0, min(int(num_voxels), M))
    where = {}
    for v in range(ne):
        where[(int(voxel_room[v]) if voxel_room is not None else 0,) + tuple(int(x) for x in cell[v])] = v
    out = np.full((M, 27), -1, np.int32)
    for v in range(ne):
        r = int(voxel_room[v]) if voxel_room is not None else 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    out[v, (dx + 1) * 9 + (dy + 1) * 3 + dz + 1] = where.get(
                        (r, int(cell[v, 0]) + dx, int(cell[v, 1]) + dy, int(cell[v, 2]) + dz), -1)
    return out


def interpolate_ref(data, inverse, voxel_data, neigh, voxel_scores, k=3, valid_labels=None, detail=False):
    """-> labels int32 (N), scores float32 (N, C), stats int64 (3) = {interpolated, no voxel, no candidate}.  voxel_scores
    float32 (M, C), or int64 (M, C) fixed-point sums taken as float32(s) * 2^-30.  detail: also the selected voxels per
    row (N, 8) int32, -1 behind them, and the rows with a tie at the k-th place (the last kept d2 equals the first
    dropped one).  Vectorised over the rows; every float32 step is one numpy float32 operation, the chains over the rank
    j are explicit loops."""
    data, voxel_data = np.asarray(data, F), np.asarray(voxel_data, F)
    inverse, neigh = np.asarray(inverse, np.int32), np.asarray(neigh, np.int32)
    sc = np.asarray(voxel_scores)
    if sc.dtype == np.int64:
        sc = (sc.astype(F) * SCALE).astype(F)                 # astype rounds to nearest even; the scaling is exact
    assert sc.dtype == F and sc.ndim == 2 and 1 <= k <= 8
    M, C = sc.shape
    N = data.shape[0]
    labels = np.full((N,), -1, np.int32)
    out = np.zeros((N, C), F)
    chosen = np.full((N, 8), -1, np.int32)
    has = (inverse >= 0) & (inverse < M)                      # rule 1
    stats = np.array([0, int((~has).sum()), 0], np.int64)
    if N == 0 or M == 0 or not has.any():
        return (labels, out, stats, chosen, np.zeros((N,), bool)) if detail else (labels, out, stats)
    u = neigh[np.where(has, inverse, 0)].astype(np.int64)     # (N, 27), rule 2
    ok = has[:, None] & (u >= 0) & (u < M)
    uc = np.where(ok, u, 0)
    if valid_labels is not None:
        ok &= np.asarray(valid_labels)[uc] >= 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        q = voxel_data[uc][:, :, :3]
        dx = (data[:, None, 0] - q[:, :, 0]).astype(F)
        dy = (data[:, None, 1] - q[:, :, 1]).astype(F)
        dz = (data[:, None, 2] - q[:, :, 2]).astype(F)
        d2 = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
        ok &= np.isfinite(d2)
        d2 = np.where(ok, d2, F(np.inf))
        um = np.where(ok, u, np.int64(1) << 40)
        order = np.lexsort((um, d2), axis=1)                  # rule 3: the total order (d2, u), the dropped ones last
        d2s, us = np.take_along_axis(d2, order, 1), np.take_along_axis(um, order, 1)
        cnt = np.minimum(ok.sum(axis=1), k)
        ties = (ok.sum(axis=1) > k) & (d2s[:, k - 1] == d2s[:, min(k, 26)])
        stats[2] = int((has & (cnt == 0)).sum())              # rule 4
        stats[0] = int((cnt > 0).sum())
        rows = np.nonzero(cnt > 0)[0]                         # rule 5
        w0 = (F(1.0) / np.maximum(d2s[rows, 0], FLOOR)).astype(F)
        W = w0.copy()
        acc = (w0[:, None] * sc[us[rows, 0]]).astype(F)
        chosen[rows, 0] = us[rows, 0]
        for j in range(1, k):
            sel = np.nonzero(cnt[rows] > j)[0]
            r = rows[sel]
            wj = (F(1.0) / np.maximum(d2s[r, j], FLOOR)).astype(F)
            W[sel] = (W[sel] + wj).astype(F)
            acc[sel] = (acc[sel] + (wj[:, None] * sc[us[r, j]]).astype(F)).astype(F)
            chosen[r, j] = us[r, j]
        res = (acc / W[:, None]).astype(F)
        out[rows] = res
        best = np.zeros(rows.size, np.int64)                  # class 0 unless a later class is strictly greater
        top = res[:, 0].copy()
        for c in range(1, C):
            gt = res[:, c] > top
            best[gt] = c
            top[gt] = res[gt, c]
        labels[rows] = best
    if detail:
        return labels, out, stats, chosen, ties
    return labels, out, stats


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError("%s differs at %d of %d, first flat index %d: got %r, want %r" % (
            what, bad.size, g.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))
