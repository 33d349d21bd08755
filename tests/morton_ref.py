"""The Morton order of include/conv3p.h (conv3p_sort_morton_order_f32) in numpy, one statement per operation of the
definition, and a second, deliberately naive statement of it (Python integers, a loop per point, `sorted`) to check the
first against.  Every floating-point operation is an IEEE double operation on both sides, so the device's orders are
compared with these bit for bit.

    codes(cloud)        uint64 (N,): the 48-bit code of every row of one (N, K >= 3) float32 cloud
    order(cloud)        int32 (N,): the rows by ascending code, ties by ascending index
    batch_order(batch)  int32 (B, N)
    naive_order(cloud)  list of int: the same, stated the slow way
"""
import math

import numpy as np

FAR = (1 << 48) - 1


def codes(cloud):
    xyz = np.asarray(cloud)[:, 0:3]
    assert xyz.dtype == np.float32
    n = xyz.shape[0]
    finite = np.isfinite(xyz).all(axis=1)                              # 1. a row is finite if all three are
    code = np.full(n, FAR, dtype=np.uint64)                            # 8. the others: the far corner's code
    if not finite.any():
        return code
    v = xyz[finite].astype(np.float64)
    lo = xyz[finite].min(axis=0).astype(np.float64)                    # 2. the float32 extrema, converted to double
    hi = xyz[finite].max(axis=0).astype(np.float64)
    e = (hi - lo).max()                                                # 3. subtracted in double
    if e == 0.0:
        q = np.zeros(v.shape, dtype=np.uint64)                         # 6.
    else:
        s = np.float64(65536.0) / e                                    # 4. one division
        d = v - lo                                                     # 5. one subtraction ...
        m = d * s                                                      #    ... then one multiplication
        q = np.minimum(np.floor(m), 65535.0).astype(np.uint64)
    c = np.zeros(v.shape[0], dtype=np.uint64)
    for k in range(16):                                                # 7. x most significant in every triple
        bit = np.uint64(1)
        c |= ((q[:, 0] >> np.uint64(k)) & bit) << np.uint64(3 * k + 2)
        c |= ((q[:, 1] >> np.uint64(k)) & bit) << np.uint64(3 * k + 1)
        c |= ((q[:, 2] >> np.uint64(k)) & bit) << np.uint64(3 * k)
    code[finite] = c
    return code


def order(cloud):
    return np.argsort(codes(cloud), kind="stable").astype(np.int32)   # 9. ties by ascending original index


def batch_order(batch):
    batch = np.asarray(batch)
    return np.stack([order(c) for c in batch]) if batch.shape[0] else np.zeros(batch.shape[0:2], dtype=np.int32)


def gather(batch, orders):
    """batch[b][orders[b]] for every cloud (rows, labels or attributes)."""
    return np.stack([np.asarray(batch)[b][orders[b]] for b in range(len(orders))])


def naive_codes(cloud):
    rows = [[float(np.float32(c)) for c in r[0:3]] for r in np.asarray(cloud)]      # float32 -> double is exact
    fin = [r for r in rows if all(math.isfinite(c) for c in r)]
    out = []
    if fin:
        lo = [min(r[a] for r in fin) for a in range(3)]
        hi = [max(r[a] for r in fin) for a in range(3)]
        e = max(hi[a] - lo[a] for a in range(3))
    for r in rows:
        if not all(math.isfinite(c) for c in r):
            out.append(FAR)
            continue
        q = [0, 0, 0]
        if e != 0.0:
            s = 65536.0 / e
            q = [min(65535, int(math.floor((r[a] - lo[a]) * s))) for a in range(3)]
        code = 0
        for k in range(16):
            for a in range(3):
                code |= ((q[a] >> k) & 1) << (3 * k + 2 - a)
        out.append(code)
    return out


def naive_order(cloud):
    return [i for _, i in sorted((c, i) for i, c in enumerate(naive_codes(cloud)))]


def nonfinite_cloud():
    """64 rows with one NaN, one +Inf and one -Inf in different coordinates of different rows (shared by the CPU and the
    GPU tests): the three rows are left out of the box and come last, in index order."""
    p = np.random.default_rng(5).uniform(-1, 1, size=(64, 3)).astype(np.float32)
    p[3, 0] = np.nan
    p[10, 1] = np.inf
    p[20, 2] = -np.inf
    p.setflags(write=False)
    return p
