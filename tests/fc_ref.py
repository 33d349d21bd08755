"""The dense head's FC kernels: a Python mirror of the host's launch planner, the case table of tests/test_fc_shapes.py
and the references those tests compare with.

Planner mirror (csrc/conv3p_abi_heads.hpp unless said otherwise; kept line by line, pinned to the library by
tests/test_fc_plan_host.py through conv3p_fc_workspace_bytes and the status codes):
    fc_plan                    :264-276   kc, chunks, mblocks, nblocks; what it refuses
    carve_fc_part / _dz        :278-279   the forward's partial sums, the backward's dz; Carver::take (conv3p_host.hpp:37-42)
                                          rounds each array up to kAlign = 256 bytes
    fc_waves                   :282-287   waves per workgroup of the dx and dW kernels, 512 or 256 slots
    fc_dx_launch               :289-299   the dx kernel's LDS: the dz tile [32][8 psteps + 4], at least nw transpose tiles
    conv3p_fc_forward_f32      :326-327   the forward's LDS: the x chunk [32][2 psteps + 1]
    conv3p_fc_backward_f32     :355-356   STEPS by batch size; the dW tile [2 STEPS][N + 1] must fit kMaxLds = 160 KiB
                                          (conv3p_abi_layout.hpp:180), else UNSUPPORTED; :362-363 its LDS and waves
    conv3p_fc_backward_step_f32 :514-515, :524-525   the same three lines

References: exact ones are int64 matmuls (inputs are small integers held in float32; every partial sum stays below
2^24, so ANY summation order gives the same float32), float ones are float64.  The SELU slope is restated in float32
with the kernel's two roundings (conv3p_kernels.hpp:80-83, built with -ffp-contract=off).
"""
import collections
import functools

import numpy as np

SELU_ALPHA = 1.6732632423543772848170429916717       # conv3p_kernels.hpp:70-73
SELU_SCALE = 1.0507009873554804934193349852946
U32 = 2.0 ** -24                                      # float32's unit roundoff

K_ALIGN = 256                                         # conv3p_host.hpp:11
K_MAX_LDS = 160 * 1024                                # conv3p_abi_layout.hpp:180
K_FC_COLS = 512                                       # conv3p_head.hpp:24
K_FC_DEPTH = 16                                       # conv3p_head.hpp:25
K_DX_DEPTH = 8                                        # fc_dx_kernel's kD, conv3p_head.hpp:170


def up(nbytes):
    return (nbytes + K_ALIGN - 1) // K_ALIGN * K_ALIGN


def fc_plan(M, K, N):
    """-> (kc, chunks, mblocks, nblocks), or None where fc_plan returns false."""
    if M < 1 or K < 1 or N < 1 or N % 8 != 0 or N > 1024 or M > 128:
        return None
    kc = (K + 255) // 256
    kc = (kc + 1) & ~1
    kc = min(max(kc, 32), 480)
    return kc, (K + kc - 1) // kc, (M + 31) // 32, (N + K_FC_COLS - 1) // K_FC_COLS


def fc_waves(K, lds):
    """-> (waves per workgroup, resident slots the host counts with)."""
    tiles = (K + 31) // 32
    slots = 512 if lds <= 80 * 1024 else 256
    nw = (tiles + slots - 1) // slots
    return min(max(nw, 4), 8), slots


def dw_steps(M):
    return 16 if M <= 32 else 32 if M <= 64 else 64


def lds_forward(kc):
    psteps = ((kc + 1) // 2 + K_FC_DEPTH - 1) // K_FC_DEPTH * K_FC_DEPTH
    return 32 * (2 * psteps + 1) * 4


def lds_dx_tile(N):
    psteps = (N // 8 + K_DX_DEPTH - 1) // K_DX_DEPTH * K_DX_DEPTH
    return 32 * (8 * psteps + 4) * 4


def lds_dx(K, N):
    """What fc_dx_launch asks for: the dz tile, or the nw transpose tiles where those are larger."""
    nw, _ = fc_waves(K, lds_dx_tile(N))
    return max(lds_dx_tile(N), nw * 32 * 33 * 4)


def lds_dw(M, N):
    return 2 * dw_steps(M) * (N + 1) * 4


def backward_served(M, K, N):
    """conv3p_fc_backward_f32 and conv3p_fc_backward_step_f32 serve the shape: fc_plan accepts it AND the dW tile fits."""
    return fc_plan(M, K, N) is not None and lds_dw(M, N) <= K_MAX_LDS


def workspace_bytes(M, K, N):
    """conv3p_fc_workspace_bytes: the larger of the two single-array layouts; 0 exactly where fc_plan refuses."""
    p = fc_plan(M, K, N)
    if p is None:
        return 0
    _, chunks, mblocks, _ = p
    return max(up(chunks * mblocks * 32 * N * 4), up(M * N * 4))


PlanRow = collections.namedtuple("PlanRow", "M K N kc chunks last mblocks nblocks steps nw_dx nw_dw slots_dx slots_dw "
                                            "served")


def plan_row(M, K, N):
    kc, chunks, mblocks, nblocks = fc_plan(M, K, N)
    nw_dx, slots_dx = fc_waves(K, lds_dx_tile(N))
    nw_dw, slots_dw = fc_waves(K, lds_dw(M, N))
    return PlanRow(M, K, N, kc, chunks, K - (chunks - 1) * kc, mblocks, nblocks, dw_steps(M), nw_dx, nw_dw, slots_dx,
                   slots_dw, backward_served(M, K, N))


# (M, K, N): every row is served by all three entry points.  tests/test_fc_plan_host.py asserts what this table covers.
CASES = [(1, 1, 8), (2, 3, 8), (31, 33, 16), (32, 32, 24), (33, 65, 40), (63, 97, 72), (64, 64, 504), (64, 40, 632),
         (65, 95, 312), (127, 200, 8), (128, 129, 312), (96, 64, 160), (3, 77, 512), (3, 77, 520), (7, 50, 1016),
         (32, 31, 1024), (5, 1593, 8), (3, 4160, 8), (5, 8193, 8), (33, 123001, 8), (1, 70000, 8), (9, 90000, 8),
         (40, 100000, 8), (65, 40000, 160), (33, 33000, 320), (8, 33000, 640)]
# one step inside each border of the dW tile's LDS limit: (M 32 | 33) x (N 632 | 640 | 1024), (M 64 | 65) x (N 312 | 320)
BORDER_INSIDE = [(32, 40, 640), (32, 40, 1024), (33, 40, 632), (64, 40, 320), (65, 40, 312)]
BORDER_OUTSIDE = [(33, 40, 640), (33, 40, 1024), (64, 40, 640), (65, 40, 320), (128, 40, 320)]


def case_id(c):
    return "%dx%dx%d" % tuple(c)


# ----------------------------------------------------------------------------------------------- references
def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: a sum of n float32 products in any order is within gamma_n sum |a||b| of the
    exact one (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return n * U32 / (1.0 - n * U32)


def selu64(v):
    v = np.asarray(v, dtype=np.float64)
    return SELU_SCALE * np.where(v >= 0.0, v, SELU_ALPHA * np.expm1(np.minimum(v, 0.0)))


def selu_slope32(y):
    """selu_slope<float> bit for bit: y >= 0 ? (float)SCALE : y + (float)(SCALE * ALPHA), the product taken in double."""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(y >= 0, np.float32(SELU_SCALE), y + np.float32(SELU_SCALE * SELU_ALPHA)).astype(np.float32)


def dz32(y, dy, act):
    """fc_dz_kernel's dz = dy * act'(y) in float32 (one rounding for the sum inside the slope, one for the product)."""
    dy = np.asarray(dy, dtype=np.float32)
    if not act:
        return dy
    with np.errstate(invalid="ignore"):
        return (dy * selu_slope32(y)).astype(np.float32)


def ulp32(v):
    """The float32 spacing at |v| (v a float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def imatmul(a, b):
    """a . b in int64 (torch's integer matmul: numpy's is ten times slower on these shapes)."""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)) @
            torch.from_numpy(np.ascontiguousarray(b, dtype=np.int64))).numpy()


IntCase = collections.namedtuple("IntCase", "x W b dy v v_nobias dx dW db")


@functools.lru_cache(maxsize=None)
def int_case(M, K, N):
    """Integer inputs in [-3, 3] as float32 and the exact results of act = 0 as float32 (9 K + 3 < 2^24 for every K of
    the table): v = x W + b, v_nobias = x W, dx = dy W^T, dW = x^T dy, db = sum_m dy.  Read only: shared between tests."""
    assert 9 * K + 3 < 2 ** 24 and 9 * max(M, N) < 2 ** 24
    rng = np.random.default_rng([M, K, N])
    x, W, dy = (rng.integers(-3, 4, size=s) for s in ((M, K), (K, N), (M, N)))
    b = rng.integers(-3, 4, size=N)
    v0 = imatmul(x, W)
    out = IntCase(x, W, b, dy, v0 + b, v0, imatmul(dy, W.T), imatmul(x.T, dy), dy.sum(axis=0))
    out = IntCase(*(a.astype(np.float32) for a in out))
    for a in out:
        a.setflags(write=False)
    return out
