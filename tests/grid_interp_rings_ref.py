"""numpy restatement of the ring fallback of the interpolated projection (include/conv3p.h:
conv3p_grid_interpolate_rings_f32 / _i64, rules 6-9), built on tests/grid_interp_ref.py: the plain pass first (rules 1-5,
interpolate_ref on the table of neighbors_ref), then for the rows it left without a candidate the ring loop.  The
candidates of ring r depend on a row's voxel alone, so they are a table per voxel, and rules 2, 3 and 5 are
interpolate_ref's on that table: the device is compared bit for bit.

interpolate_rings_ref builds the table as the device finds the cells: per (dx, dy) column one np.searchsorted on the
packed cells of the room and a walk of 2r + 1 consecutive entries (the whole cube: the cube of ring r - 1 holds no
candidate of a row that reaches ring r, so the shell alone gives the same set).  interpolate_rings_brute takes every
emitted voxel of the room within Chebyshev distance r."""
import numpy as np

from tests import grid_interp_ref as gi

OFF = 8                                                   # a searched coordinate is never negative: rings <= 8
CHUNK = 512                                               # rows of one interpolate_ref call


def _spans(ne, vox, voxel_room, voxel_start):
    """-> [(a, b, the voxels of vox that search [a, b))]: the emitted voxels, or those of the voxel's room."""
    if voxel_room is None:
        return [(0, ne, vox < ne)]
    room = np.where(vox < ne, np.asarray(voxel_room)[np.minimum(vox, len(voxel_room) - 1)], -1)
    return [(max(0, int(voxel_start[p])), min(ne, int(voxel_start[p + 1])), room == p) for p in range(len(voxel_start) - 1)]


def _compact(T):
    """The hits of every row first (their order does not enter: rule 3 is a total order), at least 27 columns."""
    if T.shape[0] == 0:
        return np.full((0, 27), -1, np.int32)
    T = np.take_along_axis(T, np.argsort(T < 0, axis=1, kind="stable"), 1)
    return np.ascontiguousarray(T[:, :max(27, int((T >= 0).sum(axis=1).max()))])


def ring_table_ref(voxel_cell, ne, vox, r, voxel_room=None, voxel_start=None):
    """int32 (len(vox), W): the emitted voxels u < ne of voxel vox[n]'s room whose cell lies within Chebyshev distance r
    of its own, found column by column by binary search in the ascending cells; -1 behind them."""
    cell = np.asarray(voxel_cell, np.int64)
    side = 2 * r + 1
    T = np.full((vox.size, side ** 3), -1, np.int32)
    B = np.int64(1 << 21)
    for a, b, mine in _spans(ne, vox, voxel_room, voxel_start):
        sel = np.nonzero(mine)[0]
        if a >= b or sel.size == 0:
            continue
        c = cell[a:b] + OFF
        keys = (c[:, 0] * B + c[:, 1]) * B + c[:, 2]
        assert (np.diff(keys) > 0).all()
        own = cell[vox[sel]] + OFF
        col = 0
        for dx in range(-r, r + 1):
            for dy in range(-r, r + 1):
                low = ((own[:, 0] + dx) * B + own[:, 1] + dy) * B + own[:, 2] - r      # the cell (a+dx, b+dy, l-r)
                pos = np.searchsorted(keys, low)
                for w in range(side):                    # consecutive entries of the same column, z up to l+r
                    at = pos + w
                    key = keys[np.minimum(at, b - a - 1)]
                    T[sel, col] = np.where((at < b - a) & (key >= low) & (key <= low + 2 * r), a + at, -1)
                    col += 1
    return _compact(T)


def ring_table_brute(voxel_cell, ne, vox, r, voxel_room=None, voxel_start=None):
    """The same set from the Chebyshev distance to all emitted voxels."""
    cell = np.asarray(voxel_cell, np.int64)
    rows = []
    for v in vox:
        if v >= ne:
            rows.append(np.zeros(0, np.int64))
            continue
        near = np.abs(cell[:ne] - cell[v]).max(axis=1) <= r
        if voxel_room is not None:
            near &= np.asarray(voxel_room[:ne]) == voxel_room[v]
        rows.append(np.nonzero(near)[0])
    T = np.full((vox.size, max([27] + [x.size for x in rows])), -1, np.int32)
    for n, x in enumerate(rows):
        T[n, :x.size] = x
    return T


def _rings(table_of, data, inverse, voxel_data, voxel_cell, num_voxels, voxel_scores, k, rings, valid_labels, voxel_room,
           voxel_start):
    assert 1 <= rings <= 8
    data, inverse = np.asarray(data, gi.F), np.asarray(inverse, np.int32)
    M = np.asarray(voxel_scores).shape[0]
    ne = max(0, min(int(num_voxels), M))
    neigh = gi.neighbors_ref(voxel_cell, num_voxels, voxel_room, voxel_start)
    labels, out, stats = gi.interpolate_ref(data, inverse, voxel_data, neigh, voxel_scores, k=k, valid_labels=valid_labels)
    ring = (labels >= 0).astype(np.int32)                 # rule 6
    ring_stats = np.zeros(9, np.int64)
    ring_stats[1] = stats[0]
    left = np.nonzero((inverse >= 0) & (inverse < M) & (labels < 0))[0]
    ring_stats[0] = left.size
    for r in range(2, rings + 1):                         # rule 7
        if left.size == 0:
            break
        vox, place = np.unique(inverse[left], return_inverse=True)
        table = table_of(voxel_cell, ne, vox.astype(np.int64), r, voxel_room, voxel_start)
        found = np.zeros(left.size, bool)
        for c in range(0, left.size, CHUNK):
            rows = left[c:c + CHUNK]
            lab, sc, _ = gi.interpolate_ref(data[rows], place[c:c + CHUNK].astype(np.int32), voxel_data, table, voxel_scores,
                                            k=k, valid_labels=valid_labels)
            hit = lab >= 0                                # the first ring with a candidate ends the search
            labels[rows[hit]], out[rows[hit]], ring[rows[hit]] = lab[hit], sc[hit], r
            found[c:c + CHUNK] = hit
        n = int(found.sum())
        ring_stats[r] = n
        stats[0] += n
        stats[2] -= n                                     # rule 8: what is left at the end
        left = left[~found]
    return labels, out, ring, stats, ring_stats


def interpolate_rings_ref(data, inverse, voxel_data, voxel_cell, num_voxels, voxel_scores, k=3, rings=1, valid_labels=None,
                          voxel_room=None, voxel_start=None):
    """-> labels int32 (N), scores float32 (N, C), ring int32 (N), stats int64 (3), ring_stats int64 (9).  voxel_cell
    (>= M, 3) and num_voxels are the subsampling's, voxel_scores (M, C) float32 or int64 as interpolate_ref takes them."""
    return _rings(ring_table_ref, data, inverse, voxel_data, voxel_cell, num_voxels, voxel_scores, k, rings, valid_labels,
                  voxel_room, voxel_start)


def interpolate_rings_brute(data, inverse, voxel_data, voxel_cell, num_voxels, voxel_scores, k=3, rings=1, valid_labels=None,
                            voxel_room=None, voxel_start=None):
    return _rings(ring_table_brute, data, inverse, voxel_data, voxel_cell, num_voxels, voxel_scores, k, rings, valid_labels,
                  voxel_room, voxel_start)
