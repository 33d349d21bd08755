"""numpy restatement of conv3p_grid_segments_smooth and conv3p_grid_segment_pool_f32 / _i64 (include/conv3p.h, rules J1-J5
and P1-P6).

Like tests/grid_segments_ref.py it walks every tap of the full directed relation of S2, not the half the kernels use,
and counts the pairs of J5 where u < v.  The float32 operations of J2-J4 are numpy float32 operations, one rounding each,
in the association the header gives.  The pool works in uint64, which wraps as the kernels' integers do.
"""
import numpy as np

from tests import grid_segments_ref as gs

F = np.float32


def pair_rule(v, u, normals=None, flags=None, curvature=None, min_cos=0.0, signed=False, max_curvature=0.0, features=None,
              max_difference=0.0):
    """J2-J4 on the pairs (v[i], u[i]) -> int8: 0 joined, 2 refused for a missing normal, 3 by angle, 4 by curvature, 5 by
    features (the index of smooth_stats the pair is counted in, 1 for joined written as 0)."""
    n = v.shape[0]
    verdict = np.zeros(n, dtype=np.int8)
    open_ = np.ones(n, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if normals is not None:
            nrm = np.asarray(normals, dtype=F)
            has = np.isfinite(nrm).all(axis=1)
            if flags is not None:
                has &= np.asarray(flags) == 0
            missing = ~(has[v] & has[u])
            verdict[open_ & missing] = 2
            open_ &= ~missing
            a, b = nrm[v], nrm[u]
            d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]          # float32, three products, two sums
            assert d.dtype == F
            if not signed:
                d = np.abs(d)
            fails = ~(d >= F(min_cos))
            verdict[open_ & fails] = 3
            open_ &= ~fails
        if curvature is not None:
            c = np.asarray(curvature, dtype=F)
            fails = ~((c[v] <= F(max_curvature)) & (c[u] <= F(max_curvature)))
            verdict[open_ & fails] = 4
            open_ &= ~fails
        if features is not None:
            f = np.asarray(features, dtype=F)
            diff = np.abs(f[v] - f[u])
            assert diff.dtype == F
            fails = ~(diff <= F(max_difference)).all(axis=1)
            verdict[open_ & fails] = 5
    return verdict


def smooth_segments_ref(neigh, labels, L, voxel_count, ne, num_class, connectivity, **rule):
    """-> dict(segment, root, size, rows, label: int32 (M); stats: int32 (8); smooth_stats: int64 (8)).  rule: the keywords
    of pair_rule; at least normals or features."""
    assert rule.get("normals") is not None or rule.get("features") is not None
    neigh = np.asarray(neigh)
    M = neigh.shape[0]
    ne = min(max(int(ne), 0), M)
    lab = gs.voxel_labelling(labels, L, ne, 1 if labels is None else num_class, M)
    parent = list(range(M))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    smooth = np.zeros(8, dtype=np.int64)
    for t in gs.taps(connectivity):
        col = neigh[:, t].astype(np.int64)
        ok = (lab >= 0) & (col >= 0) & (col < ne)
        ok[ok] = lab[col[ok]] == lab[ok]
        v = np.nonzero(ok)[0]                            # J1: the candidate pairs of this tap, directed
        u = col[v]
        verdict = pair_rule(v, u, **rule)
        once = u < v                                     # J5: each undirected pair where u < v
        smooth[0] += int(once.sum())
        smooth[1] += int((once & (verdict == 0)).sum())
        for k in (2, 3, 4, 5):
            smooth[k] += int((once & (verdict == k)).sum())
        for a, b in zip(v[verdict == 0], u[verdict == 0]):
            a, b = find(int(a)), find(int(b))
            if a != b:
                parent[max(a, b)] = min(a, b)
    if rule.get("normals") is not None:
        nrm = np.asarray(rule["normals"], dtype=F)
        has = np.isfinite(nrm).all(axis=1)
        if rule.get("flags") is not None:
            has &= np.asarray(rule["flags"]) == 0
        smooth[6] = int(((lab >= 0) & ~has).sum())
    root_of = np.array([find(v) if lab[v] >= 0 else -1 for v in range(M)], dtype=np.int64)
    roots = np.nonzero((root_of == np.arange(M)) & (lab >= 0))[0]                     # S3
    S = roots.size
    rank = np.full(M, -1, dtype=np.int64)
    rank[roots] = np.arange(S)
    segment = np.where(lab >= 0, rank[np.maximum(root_of, 0)], -1).astype(np.int32)
    root = np.full(M, -1, dtype=np.int32)
    size = np.zeros(M, dtype=np.int32)
    rows = np.zeros(M, dtype=np.int32)
    label = np.full(M, -1, dtype=np.int32)
    root[:S] = roots
    label[:S] = lab[roots]
    inside = segment >= 0
    size[:S] = np.bincount(segment[inside], minlength=S)[:S]
    rows[:S] = np.bincount(segment[inside], weights=np.asarray(voxel_count)[inside].astype(np.float64), minlength=S)[:S]
    stats = np.array([S, inside.sum(), ne - inside.sum(), M - ne, size.max(initial=0), rows.max(initial=0), 0, 0],
                     dtype=np.int32)
    return dict(segment=segment, root=root, size=size, rows=rows, label=label, stats=stats, smooth_stats=smooth)


def pool_ref(values, segment, S, voxel_count, ne, weight, with_mean=True):
    """values float32 or int64 (L, C); segment int32 (M); S and ne as the device reads them; weight 0 or 1 -> dict(sums int64
    (M, C), weights int64 (M), mean float64 (M, C) or None, label int32 (M), voxel_label int32 (M), stats int64 (4))."""
    values = np.asarray(values)
    segment = np.asarray(segment)
    M = segment.shape[0]
    L, C = values.shape
    ne, S = min(max(int(ne), 0), M), min(max(int(S), 0), M)
    member = (np.arange(M) < ne) & (segment >= 0) & (segment < S)                          # P1
    good = member & (np.arange(M) < L)                                                     # P2
    if values.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            fits = np.isfinite(values) & (np.abs(values) <= F(256))
        good[:L] &= fits.all(axis=1)
        q = np.zeros((L, C), dtype=np.int64)
        rows_ok = good[:L]
        q[rows_ok] = np.rint(values[rows_ok].astype(np.float64) * 2.0 ** 30).astype(np.int64)
    else:
        assert values.dtype == np.int64 and weight == 0
        q = values
    w = np.asarray(voxel_count).astype(np.int64).astype(np.uint64) if weight else np.ones(M, dtype=np.uint64)
    sums = np.zeros((M, C), dtype=np.uint64)
    weights = np.zeros(M, dtype=np.uint64)
    idx = np.nonzero(good)[0]
    with np.errstate(over="ignore"):
        np.add.at(sums, segment[idx], w[idx, None] * q[idx].astype(np.uint64))              # P3: wraps
        np.add.at(weights, segment[idx], w[idx])
    sums, weights = sums.view(np.int64), weights.view(np.int64)
    live = weights != 0
    mean = None
    if with_mean:
        mean = np.zeros((M, C), dtype=np.float64)                                          # P4
        mean[live] = sums[live].astype(np.float64) / (weights[live].astype(np.float64) * 2.0 ** 30)[:, None]
    label = np.full(M, -1, dtype=np.int32)                                                 # P5
    voted = live & (sums != 0).any(axis=1)
    label[voted] = np.argmax(sums[voted], axis=1)                                          # the first of equal maxima
    voxel_label = np.where(member, label[np.where(member, segment, 0)], -1).astype(np.int32)
    stats = np.array([good.sum(), member.sum() - good.sum(), (label[:S] >= 0).sum(), (label[:S] < 0).sum()], dtype=np.int64)
    return dict(sums=sums, weights=weights, mean=mean, label=label, voxel_label=voxel_label, stats=stats)


def hand_case():
    """The fixed case of the issue: a floor and a wall that meet in a crease, on an (8, 4, 8) lattice -> (occ, normals (60, 3)
    float32): (0, 0, 1) on the floor, (1, 0, 0) on the wall, (h, 0, h) with h = float32(sqrt(0.5)) on the four crease
    voxels."""
    occ = np.zeros((8, 4, 8), dtype=bool)
    occ[:, :, 0] = True
    occ[0, :, :] = True
    cells = np.argwhere(occ)
    h = F(np.sqrt(0.5))
    nrm = np.zeros((cells.shape[0], 3), dtype=F)
    floor = (cells[:, 0] > 0) & (cells[:, 2] == 0)
    wall = (cells[:, 0] == 0) & (cells[:, 2] > 0)
    crease = (cells[:, 0] == 0) & (cells[:, 2] == 0)
    nrm[floor] = (0, 0, 1)
    nrm[wall] = (1, 0, 0)
    nrm[crease] = (h, 0, h)
    return occ, nrm


def min_cos_of(max_angle):
    """The host line of GridSubsample.segments."""
    import math
    return F(math.cos(math.radians(max_angle)))
