"""Which kernel family serves a call (-m gpu): one explicit row per (dtype, channel shape, tap count) cell, each run
undilated (1, 1, 1) and dilated (2, 2, 2).  plan_backward / plan_forward in conv3p_abi_routes.hpp, the one place the table
is stated, choose among the register path (dense G or populated rows; the fp64 36 -> 13 column split), the matrix-core kernels (conv3p_deep.hpp, blocks above
256 channels), the fp64 channel blocks and the generic thread-per-pair kernels (global float atomics).  The choice
depends on dtype, channels, taps, dilation, the density hint and -- it must not -- on how much scratch the buffer has.

Every cell: neighbour counts exact; y, dX, dW against the CPU oracle (tests/parity_util.TOL; fp32 dW: the oracle's own
fp32 error times 4 as a floor); the family the profile shows equals the row's, for each pass and for every run below;
deterministic rows give the same bits in two stateless runs, a cache sized exactly for the layer and a generous one.
The boundaries: fp32 narrow shapes stay on the register path up to 128 taps (3 -> 3 and 9 -> 3
beyond), fp32 36 -> 13 up to 32 taps and on the matrix-core kernels for 33 .. 64, fp32 padded shapes on the matrix-core
kernels up to 64 taps; fp64 on the register path while its dense G fits LDS, channel blocks after that (backward up to
115 taps, forward up to 92), generic beyond."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pointwise_amd import _lib, conv3p_op as op
from tests.parity_util import TOL, _family, _read_profile, make_case, rel_err

pytestmark = pytest.mark.gpu
VOX = 0.1
F32, F64 = np.float32, np.float64
R, MC, FB, G = "register", "matrix-core", "f64-blocks", "generic"
# filter extents (z, y, x) of each tap count: the boundaries of the kernels' LDS fits and tap sets
EXT = {27: (3, 3, 3), 28: (2, 2, 7), 32: (2, 4, 4), 33: (1, 3, 11), 45: (3, 3, 5), 57: (1, 3, 19), 58: (1, 2, 29),
       64: (4, 4, 4), 65: (1, 5, 13), 125: (5, 5, 5), 128: (2, 8, 8), 130: (2, 5, 13)}

# dtype, Cin, Cout, taps, hint (None / "sparse" / "dense": narrow fp32 rows only), backward family, forward family,
# deterministic
TABLE = [
    # fp32 narrow register shapes: dense G while it fits, populated rows (32 / 64 / 128-bit tap sets) up to 128 taps
    (F32, 3, 9, 27, None, R, R, True),
    (F32, 3, 9, 64, None, R, R, True),
    (F32, 3, 9, 65, None, R, R, True),
    (F32, 3, 9, 128, None, R, R, True),
    (F32, 3, 9, 130, None, G, R, False),
    (F32, 6, 9, 58, None, R, R, True),
    (F32, 6, 9, 64, "sparse", R, R, True),
    (F32, 6, 9, 130, None, G, R, False),
    (F32, 9, 9, 27, "dense", R, R, True),
    (F32, 9, 9, 45, "sparse", R, R, True),
    (F32, 9, 9, 45, "dense", R, R, True),
    (F32, 9, 9, 58, None, R, R, True),
    (F32, 9, 9, 64, None, R, R, True),
    (F32, 9, 9, 125, "dense", R, R, True),
    (F32, 9, 9, 130, None, G, R, False),
    (F32, 12, 9, 57, None, R, R, True),
    (F32, 12, 9, 128, None, R, R, True),
    (F32, 12, 9, 130, None, G, R, False),
    (F32, 3, 3, 130, None, R, R, True),          # (dense G of 3 -> 3 fits LDS up to ~190 taps)
    (F32, 9, 3, 65, None, R, R, True),
    (F32, 9, 3, 130, None, R, R, True),
    # fp32 36 -> 13: populated rows up to 32 taps, matrix-core kernels (padded 64 x 32) for 33 .. 64, generic beyond
    (F32, 36, 13, 27, None, R, R, True),
    (F32, 36, 13, 28, None, R, R, True),
    (F32, 36, 13, 32, None, R, R, True),
    (F32, 36, 13, 33, None, MC, R, True),
    (F32, 36, 13, 45, None, MC, R, True),
    (F32, 36, 13, 64, None, MC, R, True),
    (F32, 36, 13, 65, None, G, R, False),
    # fp32 outside the register shapes: matrix-core kernels up to 64 taps
    (F32, 5, 7, 27, None, MC, MC, True),
    (F32, 5, 7, 64, None, MC, MC, True),
    (F32, 5, 7, 65, None, G, G, False),
    (F32, 32, 64, 33, None, MC, MC, True),
    (F32, 32, 64, 64, None, MC, MC, True),
    (F32, 32, 64, 65, None, G, G, False),
    (F32, 300, 70, 27, None, MC, MC, True),      # more than 256 channels: blocks on the matrix-core kernels
    # fp64 register shapes: dense G while it fits, then channel blocks of 16 x 8 / 16 x 4 / 16 x 2
    (F64, 3, 9, 27, None, R, R, True),
    (F64, 3, 9, 32, None, R, R, True),
    (F64, 3, 9, 33, None, FB, R, True),
    (F64, 3, 9, 58, None, FB, R, True),
    (F64, 3, 9, 125, None, G, R, False),
    (F64, 6, 9, 28, None, R, R, True),
    (F64, 6, 9, 32, None, FB, R, True),
    (F64, 9, 9, 28, None, R, R, True),
    (F64, 9, 9, 33, None, FB, R, True),
    (F64, 9, 9, 64, None, FB, R, True),
    (F64, 9, 9, 125, None, G, G, False),
    (F64, 12, 9, 27, None, R, R, True),
    (F64, 12, 9, 28, None, FB, R, True),
    (F64, 12, 9, 57, None, FB, R, True),
    (F64, 36, 13, 27, None, R, R, True),         # (backward: three column passes of the register kernels)
    (F64, 36, 13, 32, None, R, FB, True),
    (F64, 36, 13, 33, None, R, FB, True),
    (F64, 36, 13, 45, None, FB, FB, True),
    (F64, 36, 13, 64, None, FB, FB, True),
    (F64, 36, 13, 65, None, FB, FB, True),
    (F64, 3, 3, 64, None, R, R, True),
    (F64, 3, 3, 125, None, G, R, False),
    (F64, 9, 3, 65, None, R, R, True),
    (F64, 9, 3, 128, None, G, R, False),
    # fp64 outside the register shapes: channel blocks
    (F64, 5, 7, 27, None, FB, FB, True),
    (F64, 5, 7, 28, None, FB, FB, True),
    (F64, 5, 7, 32, None, FB, FB, True),
    (F64, 5, 7, 57, None, FB, FB, True),
    (F64, 5, 7, 58, None, FB, FB, True),
    (F64, 5, 7, 65, None, FB, FB, True),
    (F64, 5, 7, 128, None, G, G, False),
    (F64, 17, 3, 33, None, FB, FB, True),
    (F64, 17, 3, 64, None, FB, FB, True),
]
KINDS = ("modelnet", "room", "lattice")
STRIDES = ((1, 1, 1), (2, 2, 2))


def _id(row):
    dt, ci, co, nt, hint, fb, ff, det = row
    return "%s-%dto%d-t%d%s" % (np.dtype(dt).name, ci, co, nt, "-" + hint if hint else "")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _run(dev, case, s, cache):
    """(y, dX, dW) on the device and the families the profile saw for the forward and the backward call."""
    lib = _lib.load()
    P, X, W, dY = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tx, tw, tdy = t(P), t(X), t(W), t(dY)
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        y = op.conv3p(tp, tx, tw, s, VOX, cache=cache)
        torch.cuda.synchronize()
        fseen = _read_profile(lib)
        dx, dw = op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache)
        torch.cuda.synchronize()
        bseen = _read_profile(lib)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    return (y, dx, dw), (_family(fseen, True), _family(bseen, False)), (fseen, bseen)


@pytest.mark.parametrize("s", STRIDES, ids=lambda s: "s%d" % s[0])
@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_dispatch_map(dev, row, s):
    dt, ci, co, nt, hint, fam_b, fam_f, det = row
    filt = EXT[nt]
    k = TABLE.index(row)
    B, N = (1, 300) if max(ci, co) > 256 else (2, 420 + 40 * (k % 5))
    case = make_case(KINDS[k % 3], B, N, ci, co, filt, seed=2600 + 7 * k, dtype=dt)
    P, X, W, dY = case
    tdt = torch.float32 if dt == F32 else torch.float64

    cnt = op.neighbor_count(torch.from_numpy(P).to(dev), filt, s, VOX).cpu().numpy()
    assert np.array_equal(cnt, oracle.neighbor_count(P, filt, s, VOX)), "neighbour counts differ from the oracle"

    sparse = None if hint is None else hint == "sparse"
    exact = op.NeighborCache(B, N, tdt, dev, slots=1, max_taps=nt, max_cin=ci, max_cout=co, sparse_neighbourhoods=sparse)
    wide = op.NeighborCache(B, N, tdt, dev, slots=1, max_taps=nt, max_cin=max(256, ci), max_cout=max(256, co),
                            sparse_neighbourhoods=sparse)
    for c in (exact, wide):
        assert c.fits(B, N, tdt, dev, nt, ci, co)
    runs = {"stateless": _run(dev, case, s, None), "stateless again": _run(dev, case, s, None),
            "exact cache": _run(dev, case, s, exact), "generous cache": _run(dev, case, s, wide)}

    for name, (_, (ff, fb), (fseen, bseen)) in runs.items():
        assert (fb, ff) == (fam_b, fam_f), (name, "backward / forward family", (fb, ff), "expected", (fam_b, fam_f), bseen, fseen)
        if det:
            assert fseen.get("generic_forward_kernel", 0) == 0 and bseen.get("generic_backward_kernel", 0) == 0, (name, fseen, bseen)

    ry = oracle.forward(P, X, W, s, VOX, nthreads=8)
    rdx, rdw = oracle.backward(dY, P, X, W, s, VOX, nthreads=8)
    tol_y, tol_w = TOL[np.dtype(dt)]
    if dt == F32:
        d = np.float64
        r64 = oracle.backward(dY.astype(d), P.astype(d), X.astype(d), W.astype(d), s, VOX, nthreads=8)[1]
        tol_w = max(tol_w, 4.0 * rel_err(rdw, r64))
    for name, ((y, dx, dw), _, _) in runs.items():
        assert rel_err(y.cpu().numpy(), ry) <= tol_y, (name, "y", rel_err(y.cpu().numpy(), ry))
        assert rel_err(dx.cpu().numpy(), rdx) <= tol_y, (name, "dX", rel_err(dx.cpu().numpy(), rdx))
        assert rel_err(dw.cpu().numpy(), rdw) <= tol_w, (name, "dW", rel_err(dw.cpu().numpy(), rdw))

    if det:
        # (a hint picks the backward kernel, which the stateless calls cannot carry: they are compared with each other)
        groups = [["stateless", "stateless again", "exact cache", "generous cache"]] if hint is None else \
            [["stateless", "stateless again"], ["exact cache", "generous cache"]]
        for g in groups:
            ref = runs[g[0]][0]
            for name in g[1:]:
                for what, u, v in zip(("y", "dX", "dW"), ref, runs[name][0]):
                    assert torch.equal(u, v), (what, g[0], "and", name, "differ in their bits")


@pytest.mark.parametrize("s", STRIDES, ids=lambda s: "s%d" % s[0])
def test_filters_past_the_search_lds_limit_fail_cleanly(dev, s):
    """The per-tap populations of the search live in LDS: a filter of 8 x 9 x 9 = 648 taps does not fit (the limit lies
    near 570 taps), and the call says so instead of running anything; 8 x 8 x 8 = 512 taps still matches the oracle."""
    B, N = 1, 360
    P, X, W, dY = make_case("room", B, N, 3, 3, (8, 9, 9), seed=2900)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with pytest.raises(op.Conv3pRuntimeError, match="unsupported configuration"):
        op.conv3p(t(P), t(X), t(W), s, VOX)
    with pytest.raises(op.Conv3pRuntimeError, match="unsupported configuration"):
        op.conv3p_grad(t(dY), t(P), t(X), t(W), s, VOX)
    torch.cuda.synchronize()

    P, X, W, dY = make_case("room", B, N, 3, 3, (8, 8, 8), seed=2901)
    cnt = op.neighbor_count(t(P), (8, 8, 8), s, VOX).cpu().numpy()
    assert np.array_equal(cnt, oracle.neighbor_count(P, (8, 8, 8), s, VOX))
    (y, dx, dw), _, _ = _run(dev, (P, X, W, dY), s, None)
    ry = oracle.forward(P, X, W, s, VOX, nthreads=8)
    rdx, rdw = oracle.backward(dY, P, X, W, s, VOX, nthreads=8)
    r64 = oracle.backward(dY.astype(np.float64), P.astype(np.float64), X.astype(np.float64), W.astype(np.float64), s, VOX,
                          nthreads=8)[1]
    tol_y, tol_w = TOL[np.dtype(np.float32)]
    assert rel_err(y.cpu().numpy(), ry) <= tol_y
    assert rel_err(dx.cpu().numpy(), rdx) <= tol_y
    assert rel_err(dw.cpu().numpy(), rdw) <= max(tol_w, 4.0 * rel_err(rdw, r64))
