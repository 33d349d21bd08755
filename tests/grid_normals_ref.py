"""numpy restatement of the per-voxel normals (include/conv3p.h: conv3p_grid_normals_f32, rules R1-R6).  R1-R4: every
float32 step is one numpy operation on np.float32 values (a column of voxels at a time) and the chains over t are
explicit loops, so samples, flags, moments and the counts are compared bit for bit.  R5: np.linalg.eigh on the float32
moments taken to float64 -- the device is compared with it to a tolerance (compare_r5).  R6: a checker that works on any
stored vector (orientation_ok)."""
import numpy as np

F = np.float32
U = 2.0 ** -24
CURV_MAX = F(1.0) / F(3.0)


def moments_ref(voxel_data, neigh, num_voxels, min_neighbors=6):
    """-> samples int32 (M), flags int32 (M), moments float32 (M, 9), stats int32 (4): rules R1-R4."""
    xyz = np.ascontiguousarray(np.asarray(voxel_data, F)[:, :3])
    neigh = np.asarray(neigh, np.int32)
    M = xyz.shape[0]
    assert neigh.shape == (M, 27) and 3 <= min_neighbors <= 27
    ne = max(0, min(int(num_voxels), M))
    samples, flags, moments = np.zeros((M,), np.int32), np.full((M,), -1, np.int32), np.zeros((M, 9), F)   # R1
    if ne:
        u = neigh[:ne].astype(np.int64)
        fin = np.isfinite(xyz).all(axis=1)
        ok = (u >= 0) & (u < ne)
        uc = np.where(ok, u, 0)
        ok &= fin[uc] & fin[:ne, None]                                     # R2
        n = ok.sum(axis=1).astype(np.int32)
        with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
            q = (xyz[uc] - xyz[:ne, None, :]).astype(F)                    # R3: (ne, 27, 3)
            fn = np.maximum(n, 1).astype(F)                                # n == 0: the sums are 0
            m = np.zeros((ne, 3), F)
            for t in range(27):
                m = np.where(ok[:, t, None], (m + q[:, t]).astype(F), m)
            m = (m / fn[:, None]).astype(F)
            e = (q - m[:, None, :]).astype(F)
            C = np.zeros((ne, 6), F)
            pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            for t in range(27):
                for j, (a, b) in enumerate(pairs):
                    C[:, j] = np.where(ok[:, t], (C[:, j] + (e[:, t, a] * e[:, t, b]).astype(F)).astype(F), C[:, j])
            C = (C / fn[:, None]).astype(F)
            mo = np.concatenate([m, C], axis=1).astype(F)
            tr = ((C[:, 0] + C[:, 3]).astype(F) + C[:, 5]).astype(F)
            bad = ~np.isfinite(mo).all(axis=1) | ~(tr > 0)                 # R4
        samples[:ne], moments[:ne] = n, mo
        flags[:ne] = np.where(n < min_neighbors, 1, np.where(bad, 2, 0))
    stats = np.array([(flags == 0).sum(), (flags == 1).sum(), (flags == 2).sum(), (flags < 0).sum()], np.int32)
    return samples, flags, moments, stats


def covariance(moments):
    """float32 moments (..., 9) -> the symmetric matrices (..., 3, 3) in float64."""
    c = np.asarray(moments, np.float64)[..., 3:]
    return np.stack([c[..., [0, 1, 2]], c[..., [1, 3, 4]], c[..., [2, 4, 5]]], axis=-2)


def eigen_ref(moments):
    """R5 by the float64 eigh of the float32 moments -> eigenvalues (M, 3) ascending, the unit eigenvector of the
    smallest (M, 3), curvature (M) float64 held to [0, 1/3].  Meaningful at flags-0 voxels only."""
    lam, vec = np.linalg.eigh(covariance(moments))
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.clip(lam[:, 0] / lam.sum(axis=1), 0.0, 1.0 / 3.0)
    return lam, vec[:, :, 0], curv


def orientation_s(n, p, w):
    """R6's s in float32 for stored vectors n (M, 3), representatives p (M, 3) and viewpoints w (M, 3)."""
    n, p, w = np.asarray(n, F), np.asarray(p, F), np.asarray(w, F)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = (w - p).astype(F)
        x, y, z = (d[:, 0] * n[:, 0]).astype(F), (d[:, 1] * n[:, 1]).astype(F), (d[:, 2] * n[:, 2]).astype(F)
        return ((x + y).astype(F) + z).astype(F)


def orientation_ok(n, p=None, w=None):
    """R6 re-evaluated on stored vectors -> bool (M).  w (M, 3): the viewpoint of every voxel, rows of NaN where a voxel
    has none; None: no viewpoint at all.  With s finite and not 0 the stored vector has s > 0 (negation is exact: s of the
    vector before a flip was the negative of this); otherwise its component of largest magnitude, the lowest axis of a
    tie, is positive."""
    n = np.asarray(n, F)
    a = np.abs(n)
    top = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), n[:, 0], np.where(a[:, 1] >= a[:, 2], n[:, 1], n[:, 2]))
    by_axis = top > 0
    if w is None:
        return by_axis
    s = orientation_s(n, p, w)
    decided = np.isfinite(s) & (s != 0)
    return np.where(decided, s > 0, by_axis)


def normals_ref(voxel_data, neigh, num_voxels, min_neighbors=6, viewpoint=None, voxel_room=None):
    """The whole call -> dict of normals float32 (M, 3), curvature float32 (M), samples, flags, moments, stats.  normals
    and curvature are the float64 eigh's, rounded to float32 and oriented by R6: the device's agree to compare_r5's
    tolerance, everything else to the bit."""
    xyz = np.ascontiguousarray(np.asarray(voxel_data, F)[:, :3])
    samples, flags, moments, stats = moments_ref(voxel_data, neigh, num_voxels, min_neighbors)
    M = xyz.shape[0]
    normals, curvature = np.zeros((M, 3), F), np.zeros((M,), F)
    good = np.nonzero(flags == 0)[0]
    if good.size:
        lam, vec, curv = eigen_ref(moments[good])
        n = vec.astype(F)
        w = viewpoints_of(viewpoint, voxel_room, M)
        flip = ~orientation_ok(n, xyz[good], None if w is None else w[good])
        # a flipped vector passes unless nothing decides (s == 0 and the largest component 0 cannot happen to a unit vector)
        n[flip] = -n[flip]
        normals[good], curvature[good] = n, np.minimum(np.maximum(curv.astype(F), F(0)), CURV_MAX)
    return {"normals": normals, "curvature": curvature, "samples": samples, "flags": flags, "moments": moments, "stats": stats}


def viewpoints_of(viewpoint, voxel_room, M):
    """viewpoint None / (3,) / (1, 3) / (R, 3) with voxel_room -> None or the viewpoint of every voxel (M, 3) float32, NaN
    rows for voxels whose room is outside [0, R)."""
    if viewpoint is None:
        return None
    vp = np.asarray(viewpoint, F).reshape(-1, 3)
    if vp.shape[0] == 1:
        return np.broadcast_to(vp, (M, 3)).copy()
    room = np.asarray(voxel_room, np.int64)
    ok = (room >= 0) & (room < vp.shape[0])
    return np.where(ok[:, None], vp[np.where(ok, room, 0)], F(np.nan)).astype(F)


def compare_r5(normals, curvature, flags, moments, voxel_data, viewpoint=None, voxel_room=None, max_left_out=None):
    """The device's R5 / R6 outputs against the float64 eigh of its own (bit-exact) moments, with include/conv3p.h's
    bounds -> (compared voxels, flags-0 voxels, worst angle ratio to the bound / 64).  A flags-0 voxel is compared when
    l1 - l0 >= 1e-3 l2; length and R6 are checked at every flags-0 voxel.  max_left_out: the largest admitted share of
    flags-0 voxels the gap condition leaves out."""
    normals, curvature = np.asarray(normals, F), np.asarray(curvature, F)
    xyz = np.asarray(voxel_data, F)[:, :3]
    M = normals.shape[0]
    off = flags != 0
    assert not normals[off].any() and not curvature[off].any(), "a voxel without a normal must hold zeros"
    good = np.nonzero(flags == 0)[0]
    if good.size == 0:
        return 0, 0, 0.0
    n = normals[good].astype(np.float64)
    assert np.isfinite(n).all()
    length = np.sqrt((n * n).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 1e-6, "length off by %.3e" % np.abs(length - 1.0).max()
    w = viewpoints_of(viewpoint, voxel_room, M)
    held = orientation_ok(normals[good], xyz[good], None if w is None else w[good])
    assert held.all(), "R6 fails at %d of %d voxels, first %d" % ((~held).sum(), good.size, good[np.argmin(held)])
    lam, vec, curv = eigen_ref(moments[good])
    assert (curvature[good] >= 0).all() and (curvature[good] <= CURV_MAX).all()
    cerr = np.abs(curvature[good].astype(np.float64) - curv)
    assert cerr.max() <= 64 * U, "curvature off by %.3e = %.1f u" % (cerr.max(), cerr.max() / U)
    gap = lam[:, 1] - lam[:, 0]
    use = gap >= 1e-3 * lam[:, 2]
    if max_left_out is not None:
        assert (~use).sum() <= max_left_out * good.size, "the gap condition leaves out %d of %d" % ((~use).sum(), good.size)
    if not use.any():
        return 0, int(good.size), 0.0
    sin = np.sqrt((np.cross(n[use], vec[use]) ** 2).sum(axis=1))
    ratio = sin / (U * lam[use, 2] / gap[use])
    worst = float(ratio.max())
    assert worst <= 64.0, "angle: %.2f times u l2 / (l1 - l0) at voxel %d (bound 64)" % (worst, good[use][np.argmax(ratio)])
    return int(use.sum()), int(good.size), worst


def sphere(rows=8000, seed=404):
    """Case 4's cloud: seeded normal vectors, normalised -> float32 (rows, 3) on the unit sphere."""
    x = np.random.default_rng(seed).standard_normal((rows, 3))
    return (x / np.sqrt((x * x).sum(axis=1))[:, None]).astype(F)
