"""The case tables of the exact-arithmetic tests (tests/exact_ref.py): tests/test_exact_host.py checks every row's
premises on the CPU, tests/test_exact_families.py runs every row on the GPU.  A row names the kernel family that serves
each pass (plan_forward / plan_backward in conv3p_abi_routes.hpp; tests/test_dispatch_map.py) and the GPU test asserts it
from the profile, so a row exercises what it names."""
import collections
import functools

import numpy as np

from tests import exact_ref

VOX = 0.1
B = 2
F32, F64 = np.float32, np.float64
R, MC, FB, G = "register", "matrix-core", "f64-blocks", "generic"
S1, S2, S123 = (1, 1, 1), (2, 2, 2), (1, 2, 3)
STATELESS, HIGHEST, MEDIUM = "stateless", "highest", "medium"
DEEP = (STATELESS, HIGHEST, MEDIUM)     # the matrix-core rows: stateless, and one cache in both precisions

# dt, ci, co, taps: the layer.  N points per cloud on `grid` nodes.  hint: None / "sparse" / "dense" (a cache's density
# hint).  fam_b / fam_f: the family of the backward / forward pass.  runs: how the row is called.  ppp: the cache's
# pairs_per_point (0: sized for the layer; 4: the tiles' pair segments overflow and the tiles are handed over).
# x_max / w_max / dy_max: the integer ranges.  wide: the operand a rounding row gives more than 8 significant bits.
# sizes: the cloud's cluster sizes.
Row = collections.namedtuple("Row", "dt ci co taps N grid strides hint fam_b fam_f runs ppp x_max w_max dy_max wide sizes")


def _row(dt, ci, co, taps, fam_b, fam_f, N=300, grid=(5, 5, 4), strides=(S1, S2), hint=None, runs=(STATELESS,), ppp=0,
         x_max=7, w_max=3, dy_max=7, wide=None, sizes=(1, 2, 4, 8)):
    return Row(dt, ci, co, taps, N, grid, strides, hint, fam_b, fam_f, runs, ppp, x_max, w_max, dy_max, wide, sizes)


INTEGER_ROWS = [
    # fp32 register path
    _row(F32, 3, 9, 27, R, R),
    _row(F32, 3, 9, 65, R, R),
    _row(F32, 9, 9, 27, R, R, hint="dense", runs=(HIGHEST,), strides=(S1, S2, S123)),
    _row(F32, 9, 9, 27, R, R, hint="sparse", runs=(HIGHEST,)),
    _row(F32, 9, 9, 45, R, R),
    _row(F32, 9, 9, 125, R, R),
    _row(F32, 12, 9, 27, R, R),
    _row(F32, 36, 13, 27, R, R),                 # the transform + gather forward, the quad backward
    _row(F32, 3, 3, 135, R, R),
    _row(F32, 9, 3, 65, R, R),
    # fp32 generic kernels: float atomics, whose order is free -- and cannot matter here
    _row(F32, 9, 9, 135, G, R),
    _row(F32, 5, 7, 65, G, G),
    _row(F32, 36, 13, 65, G, R),
    # fp32 matrix-core path: every instantiated padded class (CONV3P_DEEP_SHAPES), channel blocks above 256
    _row(F32, 5, 7, 27, MC, MC, runs=DEEP),
    _row(F32, 3, 64, 27, MC, MC, runs=DEEP),
    _row(F32, 37, 2, 27, MC, MC, runs=DEEP),
    _row(F32, 7, 43, 27, MC, MC, runs=DEEP),
    _row(F32, 64, 128, 27, MC, MC, runs=DEEP, strides=(S1, S2, S123)),
    _row(F32, 128, 256, 27, MC, MC, runs=DEEP),
    _row(F32, 129, 250, 27, MC, MC, runs=DEEP),
    _row(F32, 200, 130, 27, MC, MC, runs=DEEP),
    _row(F32, 256, 128, 27, MC, MC, runs=DEEP),
    _row(F32, 256, 256, 27, MC, MC, runs=DEEP),
    _row(F32, 32, 64, 63, MC, MC, runs=DEEP),
    _row(F32, 36, 13, 45, MC, R, runs=DEEP),
    _row(F32, 300, 70, 27, MC, MC, runs=DEEP),
    _row(F32, 40, 260, 27, MC, MC, runs=DEEP),
    _row(F32, 128, 256, 27, MC, MC, runs=DEEP, N=700, grid=(7, 7, 6)),
    _row(F32, 32, 128, 27, MC, MC, runs=DEEP),
    _row(F32, 128, 64, 27, MC, MC, runs=DEEP),
    _row(F32, 100, 20, 27, MC, MC, runs=DEEP, N=65, grid=(3, 3, 3)),
    _row(F32, 50, 60, 27, MC, MC, runs=DEEP, N=130, grid=(4, 4, 3)),
    _row(F32, 128, 128, 27, MC, MC, runs=DEEP, N=256, grid=(5, 5, 4)),
    # fp64: register path (36 -> 13: three column passes), channel blocks, generic
    _row(F64, 3, 9, 27, R, R),
    _row(F64, 9, 9, 33, FB, R),
    _row(F64, 36, 13, 27, R, R),
    _row(F64, 36, 13, 45, FB, FB),
    _row(F64, 5, 7, 27, FB, FB),
    _row(F64, 17, 3, 33, FB, FB),
    _row(F64, 9, 9, 125, G, G),
    # hand-over: a cloud's lists need ten times the pair slots the cache has, so tiles overflow -- register-path tiles
    # search for themselves; the matrix-core kernels flag theirs for the generic kernel's launch behind them (over
    # flagged tiles it counts as forward_kernel / backward_kernel in the profile, so the family stays matrix-core)
    _row(F32, 9, 9, 27, R, R, runs=(HIGHEST,), ppp=4),
    _row(F32, 32, 64, 27, MC, MC, runs=(HIGHEST, MEDIUM), ppp=4),
]

# One operand of more than 8 significant bits (integers up to +-300: the odd ones between 256 and 512 are exact ties of the
# bf16 rounding), the others small enough for the headroom.  X wide: M_f of the forward and the X rows of the
# grad_filter product are rounded; W wide: the forward's W and the grad_input pass's W^T; dY wide: G_f' of the
# grad_input pass and the G rows of the grad_filter product.
ROUNDED_OUTPUTS = {"X": ("y", "dW"), "W": ("y", "dX"), "dY": ("dX", "dW")}
#
# M_f is a mean of x, but G_f'[j] sums the dY of the cluster next to j over the size of j's own: up to 8 times the range
# of dY on the mixed clouds.  At 256 output channels that takes the grad_input sums of a wide W or dY past 2^24 units, so
# those rows run on clouds of 8-point clusters only (populations {0, 8}: G_f' is a mean as well), a wide W next to
# dY in {-1, 0, 1}.
_WIDE = {"X": dict(x_max=300, w_max=1, dy_max=3), "W": dict(x_max=3, w_max=300, dy_max=3),
         "dY": dict(x_max=3, w_max=1, dy_max=300)}
# (Three or four tiles per cloud there, not five: the reference's own loops, which the CPU test runs on every row, take seconds
# per cloud at these widths.)
_SMALL = dict(N=130, grid=(4, 4, 3))
_EIGHTS = dict(N=200, grid=(4, 4, 3), sizes=(8,))
_WIDE_256 = {"X": dict(_WIDE["X"], **_SMALL), "W": dict(x_max=3, w_max=300, dy_max=1, **_EIGHTS),
             "dY": dict(_WIDE["dY"], **_EIGHTS)}
ROUNDING_ROWS = [_row(F32, ci, co, 27, MC, MC, runs=(HIGHEST, MEDIUM), wide=wide, **(_WIDE if co < 256 else _WIDE_256)[wide])
                 for ci, co in ((37, 43), (128, 256), (256, 256)) for wide in ("X", "W", "dY")]

ROWS = INTEGER_ROWS + ROUNDING_ROWS
CASES = [(k, s) for k, row in enumerate(ROWS) for s in row.strides]


def case_id(case):
    k, s = case
    r = ROWS[k]
    return "%s-%dto%d-t%d-n%d%s%s%s-s%d%d%d" % (np.dtype(r.dt).name, r.ci, r.co, r.taps, r.N, "-" + r.hint if r.hint else "",
                                                "-ppp%d" % r.ppp if r.ppp else "", "-wide" + r.wide if r.wide else "", *s)


@functools.lru_cache(maxsize=None)
def cloud(N, grid, sizes):
    """The row's clouds, float32: shared by every row of the same size."""
    P = np.stack([exact_ref.cluster_cloud(N, 7100 + 10 * N + b, grid, voxel=VOX, sizes=sizes) for b in range(B)])
    P.setflags(write=False)
    return P


def inputs(k):
    """(P, X, W, dY) of row k in its dtype."""
    r = ROWS[k]
    X, W, dY = exact_ref.int_case(B, r.N, r.ci, r.co, exact_ref.EXT[r.taps], 5000 + 13 * k, r.x_max, r.w_max, r.dy_max, r.dt)
    return cloud(r.N, r.grid, r.sizes).astype(r.dt), X, W, dY
