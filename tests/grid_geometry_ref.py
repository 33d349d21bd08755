"""numpy restatement of conv3p_grid_segment_geometry (include/conv3p.h, rules G1-G8).

G1-G5 are defined to the bit and are restated as such: the integer moments are summed as Python integers (object arrays),
so nothing rounds, and reduced modulo 2^64 at the end as G4 says.  G6 is a tolerance quantity: frame() restates the
kernel's solver (six cyclic Jacobi sweeps in float64) for the tests that have no device, and figures() measures a frame --
the device's or this one -- against G6's four bounds with the covariance rebuilt in exact rational arithmetic.  G7, G8 and
the stats are exact rules on a STORED frame, so sign_rule(), extent_ref() and stats_ref() take the frame they are given.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SWEEPS = 6
MASK = (1 << 64) - 1


def key32(x):
    """G3's key of float32 values -> uint32: the total order on the bits."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 == 0, b ^ np.uint32(0x80000000), ~b)


def unkey32(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def key64(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) == 0, b ^ np.uint64(1 << 63), ~b)


def unkey64(k):
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) == 1, k ^ np.uint64(1 << 63), ~k).astype(np.uint64).view(np.float64)


def members(segment, ne, S):
    """G1 -> (the member voxels in ascending number, their segments)."""
    segment = np.asarray(segment).astype(np.int64)
    M = segment.shape[0]
    ne, S = min(max(int(ne), 0), M), min(max(int(S), 0), M)
    v = np.nonzero((np.arange(M) < ne) & (segment >= 0) & (segment < S))[0]
    return v, segment[v], S


def to_int64(x):
    """A Python integer modulo 2^64 -> the int64 with those bits."""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def exact_part(voxel_data, voxel_cell, voxel_count, segment, S, ne, weight):
    """G1-G5 -> dict(cell_box int32 (M, 6), box float32 (M, 6), moments int64 (M, 10), centroid float64 (M, 3)), the
    filler rows included."""
    cell = np.asarray(voxel_cell).astype(np.int64)
    M = cell.shape[0]
    v, s, S = members(segment, ne, S)
    lo = np.full((M, 3), np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full((M, 3), np.iinfo(np.int64).min, dtype=np.int64)
    np.minimum.at(lo, s, cell[v])
    np.maximum.at(hi, s, cell[v])
    kmin = np.full((M, 3), 0xFFFFFFFF, dtype=np.uint32)
    kmax = np.zeros((M, 3), dtype=np.uint32)
    keys = key32(np.asarray(voxel_data)[:, :3])
    np.minimum.at(kmin, s, keys[v])
    np.maximum.at(kmax, s, keys[v])
    d = (cell[v] - lo[s]).astype(object)                                      # Python integers from here on
    w = np.asarray(voxel_count).astype(np.int64)[v].astype(object) if weight else np.ones(v.size, dtype=object)
    terms = [w, w * d[:, 0], w * d[:, 1], w * d[:, 2], w * d[:, 0] * d[:, 0], w * d[:, 0] * d[:, 1], w * d[:, 0] * d[:, 2],
             w * d[:, 1] * d[:, 1], w * d[:, 1] * d[:, 2], w * d[:, 2] * d[:, 2]]
    sums = [[0] * 10 for _ in range(M)]
    order = np.argsort(s, kind="stable")
    starts = np.nonzero(np.diff(s[order], prepend=-1))[0] if v.size else np.zeros(0, np.int64)
    for k, t in enumerate(terms):
        if v.size:
            for seg, total in zip(s[order][starts], np.add.reduceat(t[order], starts)):
                sums[int(seg)][k] = int(total)
    out = dict(cell_box=np.zeros((M, 6), np.int32), box=np.zeros((M, 6), np.float32), moments=np.zeros((M, 10), np.int64),
               centroid=np.zeros((M, 3), np.float64))
    out["cell_box"][:, 3:] = -1
    for q in range(S):
        mo = [to_int64(x) for x in sums[q]]
        if mo[0] == 0:                                                        # no member, or no weight: filler
            continue
        out["cell_box"][q] = np.concatenate([lo[q], hi[q]])
        out["box"][q] = np.concatenate([unkey32(kmin[q]), unkey32(kmax[q])])
        out["moments"][q] = mo
        W = np.float64(mo[0])
        out["centroid"][q] = [np.float64(lo[q, a]) + np.float64(mo[1 + a]) / W for a in range(3)]
    return out


def live_rows(moments, S):
    moments = np.asarray(moments)
    S = min(max(int(S), 0), moments.shape[0])
    return np.nonzero(moments[:S, 0] != 0)[0]


def rotate(a, v, p, q, r):
    """normals_rotate of csrc/conv3p_grid_normals.hpp on a symmetric a (3 x 3 list) and the accumulated vectors v."""
    apq = a[p][q]
    if apq != 0.0:
        den = 2.0 * apq
        theta = (a[q][q] - a[p][p]) / den if den != 0.0 else math.copysign(math.inf, a[q][q] - a[p][p])
        t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0)) if math.isfinite(theta) else 0.0
    else:
        t = 0.0
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for i in range(3):
        vp, vq = v[i][p], v[i][q]
        v[i][p] = c * vp - s * vq
        v[i][q] = s * vp + c * vq


def sign_rule(axis):
    """G7 on one vector: the component of largest magnitude positive, the lowest index of a tie."""
    axis = np.asarray(axis, dtype=np.float64)
    k = int(np.argmax(np.abs(axis)))                                          # the first of equal maxima
    return -axis if axis[k] < 0 else axis


def frame(moments, S):
    """G6, G7 by the kernel's solver -> (eigenvalues (M, 3), axes (M, 3, 3)); filler rows 0."""
    moments = np.asarray(moments)
    M = moments.shape[0]
    lam, axes = np.zeros((M, 3)), np.zeros((M, 3, 3))
    for q in live_rows(moments, S):
        mo = [np.float64(x) for x in moments[q]]
        e = [float(mo[1 + a] / mo[0]) for a in range(3)]
        m2 = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}
        a = [[0.0] * 3 for _ in range(3)]
        for (i, j), k in m2.items():
            a[i][j] = a[j][i] = float(mo[k] / mo[0]) - e[i] * e[j]
        v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        for _ in range(SWEEPS):
            rotate(a, v, 0, 1, 2)
            rotate(a, v, 0, 2, 1)
            rotate(a, v, 1, 2, 0)
        pairs = [(a[k][k], [v[0][k], v[1][k], v[2][k]]) for k in range(3)]
        for i, j in ((0, 1), (1, 2), (0, 1)):                                 # descending; equal ones keep their places
            if pairs[j][0] > pairs[i][0]:
                pairs[i], pairs[j] = pairs[j], pairs[i]
        for k, (l, vec) in enumerate(pairs):
            lam[q, k] = 0.0 if l < 0.0 else l
            x, y, z = vec
            n = math.sqrt((x * x + y * y) + z * z)
            axes[q, k] = sign_rule([x / n, y / n, z / n])
    return lam, axes


def extent_ref(voxel_cell, segment, S, ne, moments, centroid, axes):
    """G8 from a stored frame -> float64 (M, 6); filler rows 0."""
    cell = np.asarray(voxel_cell).astype(np.float64)
    M = cell.shape[0]
    v, s, S = members(segment, ne, S)
    q = cell[v] - np.asarray(centroid)[s]
    ax = np.asarray(axes)[s]
    kmin = np.full((M, 3), np.iinfo(np.uint64).max, dtype=np.uint64)
    kmax = np.zeros((M, 3), dtype=np.uint64)
    for k in range(3):
        p = (q[:, 0] * ax[:, k, 0] + q[:, 1] * ax[:, k, 1]) + q[:, 2] * ax[:, k, 2]
        np.minimum.at(kmin[:, k], s, key64(p))
        np.maximum.at(kmax[:, k], s, key64(p))
    out = np.zeros((M, 6), dtype=np.float64)
    live = live_rows(moments, S)
    out[live] = np.concatenate([unkey64(kmin[live]), unkey64(kmax[live])], axis=1)
    return out


def stats_ref(S, cell_box, moments, eigenvalues):
    live = live_rows(moments, S)
    box = np.asarray(cell_box)[live]
    return np.array([min(max(int(S), 0), np.asarray(moments).shape[0]), int((box[:, :3] == box[:, 3:]).all(axis=1).sum()),
                     int((np.asarray(eigenvalues)[live, 2] == 0).sum()), 0], dtype=np.int32)


def geometry_ref(voxel_data, voxel_cell, voxel_count, segment, S, ne, weight, eigenvalues=None, axes=None):
    """Everything.  Without a frame the solver's own is used; with the device's (eigenvalues, axes), extent and stats are
    what G8 and the stats rule make of THAT frame."""
    out = exact_part(voxel_data, voxel_cell, voxel_count, segment, S, ne, weight)
    if axes is None:
        eigenvalues, axes = frame(out["moments"], S)
    out["eigenvalues"], out["axes"] = np.asarray(eigenvalues), np.asarray(axes)
    out["extent"] = extent_ref(voxel_cell, segment, S, ne, out["moments"], out["centroid"], axes)
    out["stats"] = stats_ref(S, out["cell_box"], out["moments"], eigenvalues)
    return out


def exact_covariance(mo):
    """The covariance of one row of moments in exact rational arithmetic, every entry rounded once to float64."""
    mo = [int(x) for x in mo]
    W = mo[0]
    e = [Fraction(mo[1 + a], W) for a in range(3)]
    m2 = [[mo[4], mo[5], mo[6]], [mo[5], mo[7], mo[8]], [mo[6], mo[8], mo[9]]]
    return np.array([[float(Fraction(m2[i][j], W) - e[i] * e[j]) for j in range(3)] for i in range(3)], dtype=np.float64)


def figures(moments, S, eigenvalues, axes):
    """A frame against G6's bounds -> (worst (i), worst (ii), worst (iv)) in units of u = 2^-53, (ii) and (iv) relative to
    max(trace C, 1); asserts (iii)."""
    worst = [0.0, 0.0, 0.0]
    for q in live_rows(moments, S):
        C = exact_covariance(np.asarray(moments)[q])
        A, lam = np.asarray(axes)[q], np.asarray(eigenvalues)[q]
        assert lam[0] >= lam[1] >= lam[2] >= 0.0, (q, lam)                      # (iii)
        n = max(float(np.trace(C)), 1.0)
        worst[0] = max(worst[0], float(np.abs(A @ A.T - np.eye(3)).max()) / U)
        worst[1] = max(worst[1], float(np.abs(A.T @ np.diag(lam) @ A - C).max()) / (U * n))
        worst[2] = max(worst[2], float(np.abs(lam - np.linalg.eigvalsh(C)[::-1]).max()) / (U * n))
    return tuple(worst)
