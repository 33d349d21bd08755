"""numpy restatement of the voxel-grid subsampling (include/conv3p.h: conv3p_grid_subsample_f32, steps 1-8, and
conv3p_grid_project_labels).  Every float32 step is one numpy float32 operation, so the device is compared bit for bit.
The mean adds a voxel's members with an explicit loop over the list rank -- np.add.reduce / reduceat add pairwise, in
another order."""
import numpy as np

F = np.float32
MAX_AXIS, MAX_CELLS = 1 << 20, 1 << 40


def ieee_min(col):
    """The minimum with -0.0 below +0.0 (IEEE 754-2019 minimum)."""
    m = col.min()
    if m == 0 and np.signbit(col[col == 0]).any():
        return F(-0.0)
    return F(m)


def filler(N, K, max_voxels, with_labels):
    M = int(max_voxels)
    return {"data": np.zeros((M, K), F), "labels": np.full((M,), -1, np.int32) if with_labels else None,
            "inverse": np.full((N,), -1, np.int32), "voxel_row": np.full((M,), -1, np.int32),
            "voxel_count": np.zeros((M,), np.int32), "voxel_cell": np.full((M, 3), -1, np.int32),
            "stats": np.zeros((8,), np.int32)}


def cells_of(data, voxel):
    """Steps 1-4 -> (finite mask, lo (3) float32, s (finite rows, 3) float32, i (finite rows, 3) int64, n (3) Python
    ints); without a finite row s and i are empty and n is (0, 0, 0)."""
    xyz = np.ascontiguousarray(data[:, :3], dtype=F)
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return fin, np.zeros(3, F), np.zeros((0, 3), F), np.zeros((0, 3), np.int64), (0, 0, 0)
    pts = xyz[fin]
    lo = np.array([ieee_min(pts[:, a]) for a in range(3)], F)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (pts - lo[None, :]).astype(F)
        q = np.floor((s / F(voxel)).astype(F))
    q = np.where(q < F(1073741824.0), q, F(1073741824.0))
    i = q.astype(np.int64)
    return fin, lo, s, i, tuple(int(i[:, a].max()) + 1 for a in range(3))


def grid_subsample_ref(data, labels=None, voxel=0.05, mode="mean", num_class=None, max_voxels=None):
    """-> dict of data (max_voxels, K) float32, labels int32 or None, inverse (N), voxel_row, voxel_count, voxel_cell,
    stats: what conv3p_grid_subsample_f32 writes (and, for N == 0 or max_voxels == 0, what grid.grid_subsample fills)."""
    data = np.ascontiguousarray(data, dtype=F)
    N, K = data.shape
    voxel = F(voxel)
    M = N if max_voxels is None else int(max_voxels)
    r = filler(N, K, M, labels is not None)
    if N == 0 or M == 0:
        return r
    fin, lo, s, i, n = cells_of(data, voxel)
    st = r["stats"]
    st[2:5] = n
    st[5] = int((~fin).sum())
    if not fin.any():
        return r
    if max(n) > MAX_AXIS or n[0] * n[1] * n[2] > MAX_CELLS:
        st[7] = 1
        return r
    c = (i[:, 0] * n[1] + i[:, 1]) * n[2] + i[:, 2]
    rows = np.nonzero(fin)[0]
    order = np.argsort(c, kind="stable")                 # ascending cell, within a cell ascending row
    cs = c[order]
    head = np.ones(cs.size, bool)
    head[1:] = cs[1:] != cs[:-1]
    start = np.nonzero(head)[0]
    count = np.diff(np.append(start, cs.size))
    V = start.size
    ne = min(V, M)
    member = rows[order]                                  # the lists, one behind the other
    which = np.cumsum(head) - 1                          # the voxel of every list entry
    st[0], st[1], st[6] = ne, V, int(count.max())
    inv = np.where(which < ne, which, -1).astype(np.int32)
    r["inverse"][member] = inv
    start, count = start[:ne], count[:ne]
    r["voxel_count"][:ne] = count
    r["voxel_cell"][:ne] = i[order][start]
    lab64 = None if labels is None else np.asarray(labels).astype(np.int64)
    if mode == "mean":
        acc = data[member[start]].copy()
        for rank in range(1, int(count.max()) if ne else 0):          # the explicit chain, in list order
            sel = np.nonzero(count > rank)[0]
            acc[sel] = (acc[sel] + data[member[start[sel] + rank]]).astype(F)
        r["data"][:ne] = (acc / count.astype(F)[:, None]).astype(F)
        r["voxel_row"][:ne] = member[start]
        if labels is not None:
            keep = which < ne
            l = lab64[member]
            ok = keep & (l >= 0) & (l < int(num_class))
            votes = np.zeros((ne, int(num_class)), np.int64)
            np.add.at(votes, (which[ok], l[ok]), 1)
            best = votes.argmax(axis=1)                   # the first maximum: the lowest class on a tie
            r["labels"][:ne] = np.where(votes.max(axis=1) > 0, best, -1)
    elif mode == "center":
        so, io = s[order], i[order]
        with np.errstate(over="ignore", invalid="ignore"):
            ctr = ((io.astype(F) + F(0.5)).astype(F) * voxel).astype(F)
            d3 = (so - ctr).astype(F)
            d3 = (d3 * d3).astype(F)
            d = ((d3[:, 0] + d3[:, 1]).astype(F) + d3[:, 2]).astype(F)
        rep = np.empty(ne, np.int64)
        for v in range(ne):                              # the first strict minimum in list order: the lowest row on a tie
            a, b = start[v], start[v] + count[v]
            best = a
            for j in range(a + 1, b):
                if d[j] < d[best]:
                    best = j
            rep[v] = member[best]
        r["data"][:ne] = data[rep]
        r["voxel_row"][:ne] = rep
        if labels is not None:
            r["labels"][:ne] = lab64[rep].astype(np.int32)
    else:
        raise ValueError(mode)
    return r


def project_ref(voxel_labels, inverse):
    voxel_labels, inverse = np.asarray(voxel_labels, np.int32), np.asarray(inverse, np.int32)
    ok = (inverse >= 0) & (inverse < voxel_labels.size)
    out = np.full(inverse.shape, -1, np.int32)
    out[ok] = voxel_labels[inverse[ok]]
    return out


KEYS = ("stats", "inverse", "voxel_count", "voxel_cell", "voxel_row", "labels", "data")


def assert_equal(got, want, what=""):
    for k in KEYS:
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
                what, k, bad.size, g.size, bad[0], got[k].reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]]))


# ------------------------------------------------------------------------------------------------- clouds of the tests
def cloud(N, K, seed, extent=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), num_class=13):
    """N rows uniform in a box, K - 3 feature channels in [-1, 1), labels uint8 in [0, num_class)."""
    rng = np.random.default_rng(seed)
    xyz = rng.random((N, 3)) * np.asarray(extent)[None, :] + np.asarray(origin)[None, :]
    feat = rng.random((N, K - 3)) * 2.0 - 1.0
    return np.concatenate([xyz, feat], axis=1).astype(F), rng.integers(0, num_class, size=N).astype(np.uint8)


def hand_cloud():
    """A dozen rows, voxel 0.5, num_class 4, written out by hand in tests/test_grid_host.py."""
    nan, inf = np.nan, np.inf
    data = np.array([[0.0, 0.0, 0.0, 1.0],       # 0: cell (0, 0, 0)
                     [0.25, 0.25, 0.25, 2.0],    # 1: cell (0, 0, 0), its centre
                     [1.0, 0.0, 0.0, 3.0],       # 2: cell (2, 0, 0)
                     [nan, 0.0, 0.0, 4.0],       # 3: not finite
                     [0.4, 0.1, 0.3, 4.0],       # 4: cell (0, 0, 0)
                     [0.0, 0.5, 0.0, 5.0],       # 5: cell (0, 1, 0)
                     [1.2, 0.2, 0.1, 6.0],       # 6: cell (2, 0, 0)
                     [0.1, 0.1, 0.1, 7.0],       # 7: cell (0, 0, 0)
                     [0.0, 0.9, 1.4, 8.0],       # 8: cell (0, 1, 2)
                     [0.0, 0.0, inf, 9.0],       # 9: not finite
                     [0.2, 0.7, 0.2, 11.0],      # 10: cell (0, 1, 0)
                     [1.4, 0.4, 1.4, 12.0]], F)  # 11: cell (2, 0, 2)
    labels = np.array([2, 1, 5, 0, 1, 3, -1, 2, 0, 0, 0, 3], np.int32)
    return data, labels
