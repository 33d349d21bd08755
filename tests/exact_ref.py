"""Exact-arithmetic cases of conv3p (numpy only): clouds whose tap populations are powers of two, integer operands, and
the float64 sums any correct kernel must return bit for bit.

Everything the op computes is a sum of x * w / count.  With count in {1, 2, 4, 8} and integer x, w, dY every term and
every partial sum, in any association, is a multiple of the unit 2^-3; while the sum of the terms' magnitudes stays below
2^24 units every one of them is a float32 number, so the order of the additions, fused or not, cannot matter.  The bf16
mode of the matrix-core path rounds the operands of its filter contractions (round to nearest even); with the rounding
applied at the same places the sums stay exact, so that mode is pinned bit for bit as well."""
import numpy as np

from oracle import oracle

# filter extents (z, y, x) of the odd tap counts the exact tables use
EXT = {27: (3, 3, 3), 33: (1, 3, 11), 45: (3, 3, 5), 57: (1, 3, 19), 63: (3, 3, 7), 65: (1, 5, 13), 125: (5, 5, 5),
       135: (3, 5, 9)}
LIMIT = float(2 ** 24)   # units below which every partial sum is a float32 number


def cluster_cloud(N, seed, grid, voxel=0.1, jitter=0.2, sizes=(1, 2, 4, 8)):
    """(N, 3) float32: the nodes of the integer `grid` (x, y, z), one voxel apart, in shuffled order; each occupied node
    holds a cluster of a size drawn from `sizes` (size 1 once the rest no longer fits, to end exactly at N), every
    point its node plus uniform +-jitter * voxel per axis; rows permuted.  Two points of one node are within 0.4 voxel of
    each other and points of neighbouring nodes between 0.6 and 1.4 voxel apart, so for ODD filter extents (taps centred
    on the point, one voxel wide, dilated or not) a tap holds exactly one node's cluster or nothing.  With even extents
    the tap boundary passes through the centre's own node and the jitter decides: not valid there."""
    rng = np.random.default_rng(seed)
    gx, gy, gz = grid
    nodes = np.stack(np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij"), axis=-1).reshape(-1, 3)
    nodes = nodes[rng.permutation(len(nodes))]
    owner, left = [], N
    for k in range(len(nodes)):
        if left == 0:
            break
        size = int(rng.choice(sizes))
        if size > left:
            size = 1
        owner += [k] * size
        left -= size
    assert left == 0, "grid %r has too few nodes for %d points" % (grid, N)
    P = (nodes[np.asarray(owner)] + rng.uniform(-jitter, jitter, size=(N, 3))) * voxel
    return P[rng.permutation(N)].astype(np.float32)


def int_case(B, N, ci, co, filter_zyx, seed, x_max, w_max, dy_max, dtype=np.float32):
    """Integer-valued X (B, N, ci), W (fz, fy, fx, ci, co) and dY (B, N, co) in `dtype`, uniform in +-x_max, +-w_max,
    +-dy_max; W holds zeros."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-x_max, x_max + 1, size=(B, N, ci)).astype(dtype)
    W = rng.integers(-w_max, w_max + 1, size=tuple(filter_zyx) + (ci, co)).astype(dtype)
    dY = rng.integers(-dy_max, dy_max + 1, size=(B, N, co)).astype(dtype)
    assert (W == 0).any()
    return X, W, dY


def bf16_rne(a):
    """float32 -> the nearest bf16 value (ties to even), returned as float32: on the bit pattern."""
    u = np.array(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def bf16_trunc(a):
    """float32 -> bf16 by dropping the low 16 bits (here only to show that the tests tell it from bf16_rne)."""
    u = np.array(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def _as_f32_exactly(a, what):
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a), what + " is not a float32 number before its rounding"
    return a32


def _segment_means(rows, group, inv):
    """Sums of rows * inv over runs of equal `group` (sorted): (keys, sums), and the same over |rows|."""
    if len(group) == 0:
        z = np.zeros((0, rows.shape[1]))
        return group, z, z
    start = np.flatnonzero(np.r_[True, group[1:] != group[:-1]])
    v = rows * inv[:, None]
    return group[start], np.add.reduceat(v, start, axis=0), np.add.reduceat(np.abs(v), start, axis=0)


def exact_sums(P, X, W, dY, stride, voxel, round_operand=None):
    """y (B, N, co), dX (B, N, ci) and dW (W's shape, summed over the batch) in float64 over the oracle's pair lists
    (oracle.neighbor_lists / backward_pairs: the reference's single-precision decisions), as
    parity_util.exact_from_oracle_lists, and the headroom {name: (largest sum of |terms|, unit)} (under "terms": those sums per element).

    round_operand (float32 array -> float32 array, bf16_rne for the "medium" matmul precision) is applied where DESIGN.md
    section 5b rounds: M_f = sum x / count and W[f] of the forward, G_f' = sum dY / count and W[f']^T of the grad_input
    pass, the X rows and the G_f' rows of the grad_filter product.  M_f and G_f' are formed unrounded and must be float32
    numbers.  The headroom takes the larger magnitude of every operand before and after its rounding, and the per-centre
    sums of |x| / count, |dY| / count, so it bounds the partial sums of the segmented sums and of the contractions."""
    fz, fy, fx, ci, co = W.shape
    F, (B, N) = fz * fy * fx, P.shape[:2]
    rnd = (lambda a, what: a) if round_operand is None else \
        (lambda a, what: round_operand(_as_f32_exactly(a, what)).astype(np.float64))
    big = lambda a, ra: np.maximum(np.abs(a), np.abs(ra))
    W64 = W.reshape(F, ci, co).astype(np.float64)
    rW = rnd(W64, "W")
    aW = big(W64, rW)
    y, dX, dW = np.zeros((B, N, co)), np.zeros((B, N, ci)), np.zeros((F, ci, co))
    ay, adX, adW = np.zeros((B, N, co)), np.zeros((B, N, ci)), np.zeros((F, ci, co))
    most = 1
    for b in range(B):
        cloud = np.ascontiguousarray(P[b], dtype=np.float32)
        X64, dY64 = X[b].astype(np.float64), dY[b].astype(np.float64)
        rX = rnd(X64, "X")
        aX = big(X64, rX)
        # forward: M_f[i] = sum over the neighbours j of i in tap f of x[j] / count(i, f)
        off, idx, tap = oracle.neighbor_lists(cloud, (fz, fy, fx), stride, voxel)
        ctr = np.repeat(np.arange(N, dtype=np.int64), np.diff(off))
        cnt = np.bincount(ctr * F + tap, minlength=N * F)
        order = np.argsort(ctr * F + tap, kind="stable")
        key = (ctr * F + tap)[order]
        most = max(most, int(cnt.max()))
        keys, M, aM = _segment_means(X64[idx[order]], key, 1.0 / cnt[key])
        rM = rnd(M, "M_f")
        aM = np.maximum(aM, np.abs(rM))
        for f in np.unique(keys % F):
            m = keys % F == f
            y[b, keys[m] // F] += rM[m] @ rW[f]
            ay[b, keys[m] // F] += aM[m] @ aW[f]
        # backward: G_f'[j] = sum over the pairs (j, ii, f') of dY[ii] / count(ii, f')
        j, ii, fb, count = oracle.backward_pairs(cloud, (fz, fy, fx), stride, voxel)
        live = count > 0
        j, ii, fb, count = j[live].astype(np.int64), ii[live], fb[live], count[live]
        order = np.argsort(j * F + fb, kind="stable")
        key = (j * F + fb)[order]
        most = max(most, int(count.max()) if count.size else 1)
        keys, G, aG = _segment_means(dY64[ii[order]], key, 1.0 / count[order])
        rG = rnd(G, "G_f'")
        aG = np.maximum(aG, np.abs(rG))
        for f in np.unique(keys % F):
            m = keys % F == f
            rows = keys[m] // F
            dX[b, rows] += rG[m] @ rW[f].T
            adX[b, rows] += aG[m] @ aW[f].T
            dW[f] += rX[rows].T @ rG[m]
            adW[f] += aX[rows].T @ aG[m]
    unit = 1.0 / most
    head = {"y": (float(ay.max()), unit), "dX": (float(adX.max()), unit), "dW": (float(adW.max()), unit),
            "terms": {"y": ay, "dX": adX, "dW": adW.reshape(W.shape)}}   # per element: 0 where no term enters it
    return y, dX, dW.reshape(W.shape), head


def in_units(a, unit):
    """True where every element of `a` is a whole multiple of `unit`."""
    q = np.asarray(a, dtype=np.float64) / unit
    return bool(np.all(q == np.rint(q)))
