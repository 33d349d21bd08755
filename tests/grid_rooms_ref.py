"""numpy restatement of the many-clouds voxel-grid subsampling (include/conv3p.h: conv3p_grid_subsample_rooms_f32, rules
a-e): tests/grid_ref.grid_subsample_ref run on every room's own rows, never cut, and the results stitched -- the voxels
numbered room after room, rows and voxel numbers made global, the cut of max_voxels taken by the global number."""
import numpy as np

from tests import grid_ref as gr

F = np.float32
MAX_ROOMS = 65536
KEYS = gr.KEYS + ("voxel_room", "voxel_start", "room_stats")


def grid_subsample_rooms_ref(data, room_start, labels=None, voxel=0.05, mode="mean", num_class=None, max_voxels=None):
    """-> dict of data (max_voxels, K), labels or None, inverse (N), voxel_row, voxel_count, voxel_cell, voxel_room
    (max_voxels), voxel_start (R + 1), room_stats (R, 8), stats (8): what conv3p_grid_subsample_rooms_f32 writes (and, for
    N, R or max_voxels of 0, what grid.grid_subsample_rooms fills)."""
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    rs = np.asarray(room_start, np.int64)
    R = rs.size - 1
    M = N if max_voxels is None else int(max_voxels)
    r = gr.filler(N, K, M, labels is not None)
    r["voxel_room"] = np.full((M,), -1, np.int32)
    r["voxel_start"] = np.zeros((R + 1,), np.int32)
    r["room_stats"] = np.zeros((R, 8), np.int32)
    if N == 0 or R == 0 or M == 0:
        return r
    st = r["stats"]
    st[2] = R
    if rs[0] < 0 or (np.diff(rs) < 0).any() or rs[R] > N:            # bit 1: nothing is read through room_start
        st[7] = 2
        return r
    rooms = []
    for k in range(R):
        a, b = int(rs[k]), int(rs[k + 1])
        rooms.append(gr.grid_subsample_ref(data[a:b], None if labels is None else labels[a:b], voxel=voxel, mode=mode,
                                           num_class=num_class, max_voxels=None))
    for k, q in enumerate(rooms):
        r["room_stats"][k] = q["stats"]
    err = r["room_stats"][:, 7] != 0
    st[4], st[5] = int(err.sum()), int(r["room_stats"][:, 5].sum())
    st[7] = 1 if err.any() else 0
    cells = sum(int(s[2]) * int(s[3]) * int(s[4]) for s in r["room_stats"][~err])
    if cells > gr.MAX_CELLS:                                          # bit 2: nothing is emitted
        st[7] |= 4
        r["room_stats"][:, [0, 1, 6]] = 0
        return r
    first = 0
    for k, q in enumerate(rooms):
        a, V = int(rs[k]), int(q["stats"][1])
        ne = min(V, max(0, M - first))                                # the room's single call with max_voxels_r
        lo = min(first, M)
        r["voxel_start"][k] = lo
        r["room_stats"][k, 0] = ne
        inv = q["inverse"]
        r["inverse"][a:a + inv.size] = np.where((inv >= 0) & (inv < ne), inv + first, -1)
        r["data"][lo:lo + ne] = q["data"][:ne]
        r["voxel_row"][lo:lo + ne] = q["voxel_row"][:ne] + a
        r["voxel_count"][lo:lo + ne] = q["voxel_count"][:ne]
        r["voxel_cell"][lo:lo + ne] = q["voxel_cell"][:ne]
        r["voxel_room"][lo:lo + ne] = k
        if labels is not None:
            r["labels"][lo:lo + ne] = q["labels"][:ne]
        first += V
    r["voxel_start"][R] = min(first, M)
    st[0], st[1] = min(first, M), first
    st[3] = int((r["room_stats"][:, 0] > 0).sum())
    st[6] = int(r["room_stats"][:, 6].max())
    return r


def loop_ref(run_single, data, room_start, labels, max_voxels, K):
    """The stitched outputs of a single-cloud callable run per room (run_single(rows, labels, max_voxels_r) -> dict of the
    single call's outputs, None where it does nothing): what a caller's loop builds today, for well-formed rooms without
    errors.  Only the words such a loop can know are returned."""
    rs = np.asarray(room_start, np.int64)
    R, N = rs.size - 1, data.shape[0]
    M = N if max_voxels is None else int(max_voxels)
    r = gr.filler(N, K, M, labels is not None)
    r["voxel_start"] = np.zeros((R + 1,), np.int32)
    first = 0                                            # occupied voxels of the rooms before
    for k in range(R):
        a, b = int(rs[k]), int(rs[k + 1])
        lo = min(first, M)
        r["voxel_start"][k] = lo
        if b > a:
            q = run_single(data[a:b], None if labels is None else labels[a:b], b - a)      # never cut: V is needed
            V, ne = int(q["stats"][1]), min(int(q["stats"][1]), M - lo)
            inv = q["inverse"]
            r["inverse"][a:b] = np.where((inv >= 0) & (inv < ne), inv + first, -1)
            r["data"][lo:lo + ne] = q["data"][:ne]
            r["voxel_row"][lo:lo + ne] = q["voxel_row"][:ne] + a
            r["voxel_count"][lo:lo + ne] = q["voxel_count"][:ne]
            r["voxel_cell"][lo:lo + ne] = q["voxel_cell"][:ne]
            if labels is not None:
                r["labels"][lo:lo + ne] = q["labels"][:ne]
            first += V
    r["voxel_start"][R] = min(first, M)
    return r


def assert_equal(got, want, what="", keys=KEYS):
    """Every output bit for bit (tests/grid_ref.assert_equal's comparison over the rooms call's outputs)."""
    for k in keys:
        g, w = got[k], want[k]
        assert (g is None) == (w is None), (what, k)
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        if not np.array_equal(g, w):
            bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
            raise AssertionError("%s: %s differs at %d of %d, first flat index %d: got %r, want %r" % (
                what, k, bad.size, g.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]],
                np.asarray(want[k]).reshape(-1)[bad[0]]))


def rooms_cloud(sizes, K, seed, num_class=13, spread=0.0):
    """Rooms of the given row counts, each uniform in its own box (extents and origins vary with the room; spread
    shifts the rooms apart) -> data (N, K), labels uint8 (N), room_start (R + 1) int32."""
    rng = np.random.default_rng(seed)
    parts, labs = [], []
    for k, n in enumerate(sizes):
        ext = 0.4 + 0.6 * rng.random(3)
        org = rng.random(3) * 2.0 - 1.0 + spread * k
        d, l = gr.cloud(int(n), K, seed * 1000 + k, extent=ext, origin=org, num_class=num_class)
        parts.append(d)
        labs.append(l)
    data = np.concatenate(parts) if parts else np.zeros((0, K), F)
    labels = np.concatenate(labs) if labs else np.zeros((0,), np.uint8)
    return data, labels, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
