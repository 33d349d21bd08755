"""numpy restatement of the k-nearest-voxel search and of its two consumers (include/conv3p_knn.h: conv3p_grid_knn_f32 rules
K1-K8, conv3p_grid_interpolate_knn_f32 / _i64, conv3p_grid_normals_knn_f32 rule R2').  A brute force over all (query, voxel)
pairs, O(Q M): d2 is rule 2's float32 chain, one numpy operation a step; K5 and K6 are float64, one operation a step; so the
device is compared bit for bit.  Rule 5 is tests/grid_interp_ref.py's and R3 / R4 are tests/grid_normals_ref.py's, by
import: the table is handed to them in the place of the 27 cells."""
import numpy as np

from tests import grid_interp_ref as iref
from tests import grid_normals_ref as nref

F = np.float32
BIG = np.int64(1) << 40


class Search:
    """What every question about one (cloud, queries, parameters) needs: the d2 of every pair, the Chebyshev distance of
    every pair, the candidates of K3 without the bound R, the live queries and K5's S per query."""

    def __init__(self, query, query_voxel, voxel_data, voxel_cell, num_voxels, voxel, exclude_self=False, valid=None,
                 voxel_room=None, voxel_start=None):
        q = np.ascontiguousarray(np.asarray(query, F)[:, :3])
        p = np.ascontiguousarray(np.asarray(voxel_data, F)[:, :3])
        cell = np.asarray(voxel_cell, np.int64)
        Q, M = q.shape[0], p.shape[0]
        ne = max(0, min(int(num_voxels), M))
        v0 = np.arange(Q, dtype=np.int64) if query_voxel is None else np.asarray(query_voxel, np.int64)
        assert query_voxel is not None or Q <= M
        live = (v0 >= 0) & (v0 < ne) & np.isfinite(q).all(axis=1)                       # K1
        vc = np.where(live, v0, 0)
        lo, hi = np.zeros(Q, np.int64), np.where(live, ne, 0).astype(np.int64)          # K2
        room_q, room_u = np.zeros(Q, np.int64), np.zeros(M, np.int64)
        rooms = 1
        if voxel_room is not None:
            start = np.asarray(voxel_start, np.int64)
            rooms = start.size - 1
            room_u = np.asarray(voxel_room, np.int64)
            room_q = np.where(live, room_u[vc], -1) if M else np.full(Q, -1, np.int64)
            ok = live & (room_q >= 0) & (room_q < rooms)
            g = np.where(ok, room_q, 0)
            lo = np.where(ok, np.maximum(start[g], 0), 0)
            hi = np.where(ok, np.minimum(start[g + 1], ne), 0)
            room_q = np.where(ok, room_q, -1)
        u = np.arange(M, dtype=np.int64)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            dx = (q[:, None, 0] - p[None, :, 0]).astype(F)
            dy = (q[:, None, 1] - p[None, :, 1]).astype(F)
            dz = (q[:, None, 2] - p[None, :, 2]).astype(F)
            d2 = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
        cand = live[:, None] & (u[None, :] >= lo[:, None]) & (u[None, :] < hi[:, None]) & np.isfinite(d2)    # K3 without R
        if valid is not None:
            cand &= (np.asarray(valid)[None, :M] >= 0)
        if exclude_self:
            cand &= u[None, :] != v0[:, None]
        own = cell[vc] if M else np.zeros((Q, 3), np.int64)
        self.cheb = np.abs(cell[None, :, :] - own[:, None, :]).max(axis=2) if M else np.zeros((Q, 0), np.int64)
        self.Q, self.M, self.ne, self.live, self.cand, self.d2, self.u = Q, M, ne, live, cand, d2, u
        self._sorted = {}
        # K5, in float64: one operation a step
        h = np.float64(F(voxel))
        self.h = h
        S = np.full(max(rooms, 1), np.nan)
        fq = q.astype(np.float64) - own.astype(np.float64) * h
        fu = p.astype(np.float64) - cell.astype(np.float64) * h if M else np.zeros((0, 3))
        fin_u = (u < ne) & np.isfinite(p).all(axis=1)
        for g in range(rooms if voxel_room is not None else 1):
            mq = live & (room_q == g)
            mu = fin_u & (room_u == g) if voxel_room is not None else fin_u
            if mq.any() and mu.any():
                pmin, pmax, fmin, fmax = fq[mq].min(axis=0), fq[mq].max(axis=0), fu[mu].min(axis=0), fu[mu].max(axis=0)
                S[g] = max(max(pmax[a] - fmin[a], fmax[a] - pmin[a]) for a in range(3))
        self.S_room = S
        self.S = np.where(room_q >= 0, S[np.maximum(room_q, 0)], np.nan)

    def _top(self, r):
        """The 16 smallest candidates by (d2, u) within Chebyshev distance r (None: all of the room), sorted once."""
        if r not in self._sorted:
            mask = self.cand if r is None else self.cand & (self.cheb <= r)
            d2m = np.where(mask, self.d2, F(np.inf))
            um = np.where(mask, self.u[None, :], BIG)
            order = np.lexsort((um, d2m), axis=1)[:, :16]
            self._sorted[r] = (np.take_along_axis(um, order, 1), np.take_along_axis(d2m, order, 1),
                               np.take_along_axis(self.cheb, order, 1), mask.sum(axis=1))
        return self._sorted[r]

    def kept(self, k, r=None):
        """K4 over the candidates within Chebyshev distance r (None: all of the room) -> index (Q, k), d2 (Q, k), count,
        ring."""
        us, ds, cs, total = self._top(r)
        kk = min(k, self.M)
        index, d2 = np.full((self.Q, k), -1, np.int32), np.full((self.Q, k), np.inf, F)
        ring = np.zeros(self.Q, np.int32)
        count = np.minimum(total, k).astype(np.int32)
        if kk:
            got = np.arange(kk)[None, :] < count[:, None]
            index[:, :kk] = np.where(got, us[:, :kk], -1)
            d2[:, :kk] = np.where(got, ds[:, :kk], F(np.inf))
            ring = np.where(got, cs[:, :kk], 0).max(axis=1).astype(np.int32)
        return index, d2, count, ring

    def stop(self, k, r, count, d2):
        """K6's STOP(r) from K4 over the cube of r."""
        with np.errstate(invalid="ignore", over="ignore"):
            L = np.float64(r + 1) * self.h - self.S
            least = max(0.25 * self.h, 2.0 ** -50)
            return (count >= k) & (L >= least) & (d2[:, k - 1].astype(np.float64) < (L * L) * (1.0 - 2.0 ** -20))


def knn_ref(query, query_voxel, voxel_data, voxel_cell, num_voxels, voxel, k=8, rings=2, exclude_self=False, valid=None,
            voxel_room=None, voxel_start=None, search=None):
    """-> dict of index, d2, count, ring, scanned, certified, stats (int64 (16)) and the Search."""
    s = search or Search(query, query_voxel, voxel_data, voxel_cell, num_voxels, voxel, exclude_self, valid, voxel_room, voxel_start)
    Q = s.Q
    scanned = np.where(s.live, rings, 0).astype(np.int32)
    certified = np.zeros(Q, np.int32)
    open_ = s.live.copy()
    for r in range(1, rings + 1):                              # K6: the smallest r with STOP(r)
        _, d2, count, _ = s.kept(k, r)
        hit = open_ & s.stop(k, r, count, d2)
        scanned[hit], certified[hit] = r, 1
        open_ &= ~hit
    index, d2, count, ring = s.kept(k, rings)                  # K4 over the cube of R (K7: that of scanned gives the same)
    stats = np.zeros(16, np.int64)
    stats[0] = (s.live & (count == k)).sum()
    stats[1] = (s.live & (count > 0) & (count < k)).sum()
    stats[2] = (s.live & (count == 0)).sum()
    stats[3] = (~s.live).sum()
    stats[4] = certified.sum()
    stats[5] = scanned[s.live].sum()
    for r in range(9):
        stats[6 + r] = (s.live & (count > 0) & (ring == r)).sum()
    return {"index": index, "d2": d2, "count": count, "ring": ring, "scanned": scanned, "certified": certified, "stats": stats,
            "search": s}


def check_theorem(ref, k, rings):
    """K7 by brute force: K4 over the cube of scanned equals K4 over the cube of R, and a certified query's kept set equals
    K4 over all candidates of its room.  -> (certified queries, live queries)."""
    s = ref["search"]
    for r in range(1, rings + 1):
        rows = np.nonzero(s.live & (ref["scanned"] == r))[0]
        if rows.size:
            index, d2, count, ring = s.kept(k, r)
            for name, got in (("index", index), ("d2", d2), ("count", count), ("ring", ring)):
                iref.assert_same(got[rows], ref[name][rows], "K7: %s over the cube of scanned = %d" % (name, r))
    index, d2, count, ring = s.kept(k, None)
    rows = np.nonzero(ref["certified"] == 1)[0]
    for name, got in (("index", index), ("d2", d2), ("count", count), ("ring", ring)):
        iref.assert_same(got[rows], ref[name][rows], "K7: %s of a certified query over the whole room" % name)
    return int(rows.size), int(s.live.sum())


def interpolate_knn_ref(query, voxel_data, index, count, voxel_scores, k_use):
    """Rule 5 on the first min(k_use, count) entries of the table, by tests/grid_interp_ref.py: the table takes the place of
    the 27 cells (query i is handed row i), whose selection by (d2, u) keeps the table's order.  -> labels, scores, stats
    int64 (2)."""
    index, count = np.asarray(index, np.int64), np.asarray(count, np.int64)
    Q, width = index.shape
    sc = np.asarray(voxel_scores)
    M, C = sc.shape
    n = np.minimum(np.maximum(count, 0), k_use)
    table = np.full((max(Q, 1), 27), -1, np.int32)
    table[:Q, :width] = np.where(np.arange(width)[None, :] < n[:, None], index, -1)
    pad = np.zeros((max(Q, M), C), sc.dtype)                   # query i reads row i of the table: at least Q rows
    pad[:M] = sc
    labels, scores, st = iref.interpolate_ref(query, np.arange(Q, dtype=np.int32), voxel_data, table, pad, k=min(k_use, 8)) \
        if k_use <= 8 else _interpolate_wide(query, voxel_data, table, pad, k_use)
    return labels, scores, np.array([st[0], Q - st[0]], np.int64)


def _interpolate_wide(query, voxel_data, table, sc, k_use):
    """grid_interp_ref.interpolate_ref takes k <= 8; rule 5 with up to 16 terms is the same chain continued."""
    query, voxel_data = np.asarray(query, F), np.asarray(voxel_data, F)
    Q = query.shape[0]
    if sc.dtype == np.int64:
        sc = (sc.astype(F) * iref.SCALE).astype(F)
    C = sc.shape[1]
    labels, out = np.full((Q,), -1, np.int32), np.zeros((Q, C), F)
    ok = table[:Q] >= 0
    cnt = ok.sum(axis=1)
    uc = np.where(ok, table[:Q], 0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        p = voxel_data[uc][:, :, :3]
        dx, dy, dz = ((query[:, None, a] - p[:, :, a]).astype(F) for a in range(3))
        d2 = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
        rows = np.nonzero(cnt > 0)[0]
        w0 = (F(1.0) / np.maximum(d2[rows, 0], iref.FLOOR)).astype(F)
        W, acc = w0.copy(), (w0[:, None] * sc[uc[rows, 0]]).astype(F)
        for j in range(1, k_use):
            sel = np.nonzero(cnt[rows] > j)[0]
            r = rows[sel]
            wj = (F(1.0) / np.maximum(d2[r, j], iref.FLOOR)).astype(F)
            W[sel] = (W[sel] + wj).astype(F)
            acc[sel] = (acc[sel] + (wj[:, None] * sc[uc[r, j]]).astype(F)).astype(F)
        res = (acc / W[:, None]).astype(F)
    out[rows] = res
    best, top = np.zeros(rows.size, np.int64), res[:, 0].copy()
    for c in range(1, C):
        gt = res[:, c] > top
        best[gt] = c
        top[gt] = res[gt, c]
    labels[rows] = best
    return labels, out, np.array([rows.size, 0, Q - rows.size], np.int64)


def normals_knn_ref(voxel_data, index, count, num_voxels, min_neighbors=6):
    """R1, R2', R3, R4 by tests/grid_normals_ref.py's moments_ref: the table's entries j < count in rank order take the place
    of the 27 cells in ascending t.  -> samples, flags, moments, stats."""
    index, count = np.asarray(index, np.int64), np.asarray(count, np.int64)
    M, width = index.shape
    assert np.asarray(voxel_data).shape[0] == M
    table = np.full((M, 27), -1, np.int32)
    table[:, :width] = np.where(np.arange(width)[None, :] < np.minimum(np.maximum(count, 0), width)[:, None], index, -1)
    return nref.moments_ref(voxel_data, table, num_voxels, min_neighbors)
