"""numpy restatement of the batch provider (the CPU side of test_provider*.py; pointwise_amd.provider is the device
side): the draw recipe of pointwise_amd/csrc/conv3p_provider.hpp and the assembly of a batch -- index, slice, rotate,
jitter, sort, the points / input split, the label cast -- with oracle/prestep_numpy.py doing rotate / jitter / sort."""
import numpy as np

from oracle import prestep_numpy
from tests.cls_tail_ref import philox4x32_10


def _blocks(c0, c1, seed, step):
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint32), np.asarray(c1, dtype=np.uint32))
    ctr = np.zeros(c0.shape + (4,), dtype=np.uint32)
    ctr[..., 0], ctr[..., 1] = c0, c1
    ctr[..., 2], ctr[..., 3] = step & 0xFFFFFFFF, step >> 32
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), c0.shape + (2,))
    return ctr, philox4x32_10(ctr, key)


def angle_counters(seed, step, samples):
    return _blocks(samples, 0xFFFFFFFF, seed, step)[0]


def jitter_counters(seed, step, s, N):
    return _blocks(np.arange(N), s + 1, seed, step)[0]


def uniform53(w0, w1):
    """u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, in [0, 1)."""
    w0, w1 = np.asarray(w0, dtype=np.uint32), np.asarray(w1, dtype=np.uint32)
    return ((w0 >> np.uint32(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def box_muller_uniforms(w):
    """words (..., 4) -> u1, u2, u3, u4: u1, u3 in (0, 1], u2, u4 in [0, 1); all exact in double."""
    w = np.asarray(w, dtype=np.uint32).astype(np.float64)
    return (w[..., 0] + 1.0) * 2.0 ** -32, w[..., 1] * 2.0 ** -32, (w[..., 2] + 1.0) * 2.0 ** -32, w[..., 3] * 2.0 ** -32


def normals_from_words(w):
    u1, u2, u3, u4 = box_muller_uniforms(w)
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2 * np.pi * u2
    return np.stack([r * np.cos(a), r * np.sin(a), np.sqrt(-2.0 * np.log(u3)) * np.cos(2 * np.pi * u4)], axis=-1)


def draw_angles(seed, step, samples):
    """angle of every sample index in `samples`: np.random.uniform() * 2 * np.pi with the device's uniform."""
    w = _blocks(samples, 0xFFFFFFFF, seed, step)[1]
    return uniform53(w[..., 0], w[..., 1]) * 2 * np.pi


def draw_noise(seed, step, samples, N):
    """(len(samples), N, 3) standard normals: row i of sample s from the block of counter (i, s + 1, step)."""
    samples = np.asarray(samples, dtype=np.int64)
    w = _blocks(np.arange(N)[None, :], (samples + 1)[:, None], seed, step)[1]
    return normals_from_words(w)


def assemble(data, labels, samples, N, angles=None, noise=None, sigma=0.01, clip=0.05, sort_cloud=False):
    """The providers' batch from explicit randoms: samples = the B sample indices (outside [0, S): a zero cloud with
    labels -1); angles (B) or None; noise (B, N, 3) or None.  -> points (B, N, 3), input (B, N, K), labels int32,
    order (B, N), bad count."""
    data, labels = np.asarray(data), np.asarray(labels)
    S, _, K = data.shape
    samples = np.asarray(samples, dtype=np.int64)
    B = len(samples)
    ok = (samples >= 0) & (samples < S)
    safe = np.where(ok, samples, 0)
    rows = data[safe][:, 0:N, :].astype(np.float32)                               # current_data[:, 0:num_points, :]
    xyz = np.ascontiguousarray(rows[:, :, 0:3])
    if angles is not None:
        xyz = prestep_numpy.rotate_point_cloud_by_angles(xyz, angles)
    if noise is not None:
        xyz = prestep_numpy.jitter_point_cloud(xyz, noise, sigma, clip).astype(np.float32)   # float32 when it is fed
    rows = np.concatenate([xyz, rows[:, :, 3:]], axis=2)
    rows[~ok] = 0.0
    per_point = labels.ndim == 2
    lab = labels[safe][:, 0:N] if per_point else labels[safe]
    lab = lab.astype(np.int64).astype(np.int32)
    lab[~ok] = -1
    order = np.broadcast_to(np.arange(N, dtype=np.int32), (B, N)).copy()
    if sort_cloud:
        for b in range(B):
            pc = rows[b]
            idx = np.arange(N)
            for col in (2, 1, 0):                                                 # util.py:66-68, every pass stable
                idx = idx[np.argsort(pc[idx, col], kind="mergesort")]
            order[b] = idx
        unsorted = rows
        rows = np.stack([rows[b][order[b]] for b in range(B)]) if B else rows
        assert np.array_equal(rows, prestep_numpy.sort_point_cloud_xyz(unsorted), equal_nan=True), "util.py's order"
        if per_point:
            lab = np.stack([lab[b][order[b]] for b in range(B)]) if B else lab
    return np.ascontiguousarray(rows[:, :, 0:3]), rows, lab, order, int((~ok).sum())
