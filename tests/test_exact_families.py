"""Every conv3p kernel family bit for bit (-m gpu) on the exact-arithmetic rows of tests/exact_cases.py.

The clouds' tap populations are powers of two and the operands small integers, so every term and every partial sum of
y, dX and dW is a float32 number in any order (tests/exact_ref.py; tests/test_exact_host.py checks the premises and that
the reference's own loops return these sums).  A correct kernel -- register path, matrix-core path in fp32 and bf16,
fp64 channel blocks, blocks above 256 channels, the generic atomics kernels, tiles handed over -- returns the float64
sums exactly: np.array_equal on every element, no tolerance.  The family each pass ran on is read from the profile and
asserted against the row.

Rounding rows: one operand has more than 8 significant bits.  "highest" still equals the unrounded sums;
"medium" equals the sums with bf16 round-to-nearest-even applied where DESIGN.md section 5b says the mode rounds
(M_f, W; G_f', W^T; the X and G rows of the grad_filter product) -- a dropped k-group, a mishandled last k-step, the
wrong tap's filter block or truncation instead of rounding each change some element."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle
from pointwise_amd import _lib, conv3p_op as op
from tests import exact_cases as ec
from tests import exact_ref as er
from tests.parity_util import _family, _read_profile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _reference(case):
    """(unrounded, rounded or None) exact sums of a case, each (y, dX, dW) in the row's dtype."""
    k, s = case
    row = ec.ROWS[k]
    P, X, W, dY = ec.inputs(k)
    cast = lambda r: tuple(a.astype(row.dt) for a in r[:3])
    plain = er.exact_sums(P, X, W, dY, s, ec.VOX)
    for name in ("y", "dX", "dW"):
        total, unit = plain[3][name]
        assert total / unit < er.LIMIT, (name, total / unit)
    rounded = None
    if row.wide:
        rounded = er.exact_sums(P, X, W, dY, s, ec.VOX, er.bf16_rne)
        for name in ("y", "dX", "dW"):
            total, unit = rounded[3][name]
            assert total / unit < er.LIMIT, (name, total / unit)
    return cast(plain), cast(rounded) if rounded else None


def _run(dev, tensors, s, cache):
    """(y, dX, dW) as numpy arrays and what the profile saw in the forward and in the backward call."""
    lib = _lib.load()
    tp, tx, tw, tdy = tensors
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        y = op.conv3p(tp, tx, tw, s, ec.VOX, cache=cache)
        torch.cuda.synchronize()
        fseen = _read_profile(lib)
        dx, dw = op.conv3p_grad(tdy, tp, tx, tw, s, ec.VOX, cache=cache)
        torch.cuda.synchronize()
        bseen = _read_profile(lib)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    return (y.cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy()), fseen, bseen


def _where(got, ref):
    """Where two arrays differ, for the failure message: how many elements, the largest difference, and along each axis
    which indices (for channels also modulo 8 and 32: k-groups and k-steps of the matrix-core kernels)."""
    bad = np.argwhere(got != ref)
    out = ["%d of %d elements differ, largest difference %g" % (len(bad), ref.size, float(np.abs(got - ref).max()))]
    for ax in range(ref.ndim):
        idx = np.unique(bad[:, ax])
        out.append("axis %d: %d of %d indices %s" % (ax, len(idx), ref.shape[ax], idx[:24].tolist()))
        if ref.shape[ax] > 32:
            out.append("  mod 8: %s  mod 32: %s" % (np.unique(idx % 8).tolist(), np.unique(idx % 32).tolist()))
    return "; ".join(out)


@pytest.mark.parametrize("case", ec.CASES, ids=[ec.case_id(c) for c in ec.CASES])
def test_exact(dev, case):
    k, s = case
    row = ec.ROWS[k]
    P, X, W, dY = ec.inputs(k)
    plain, rounded = _reference(case)
    filt = er.EXT[row.taps]
    tdt = torch.float32 if row.dt == np.float32 else torch.float64
    tensors = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, X, W, dY))

    cnt = op.neighbor_count(tensors[0], filt, s, ec.VOX).cpu().numpy()
    assert np.array_equal(cnt, oracle.neighbor_count(P, filt, s, ec.VOX)), "populations differ from the oracle's"

    cache = None
    if set(row.runs) - {ec.STATELESS}:
        sparse = None if row.hint is None else row.hint == "sparse"
        cache = op.NeighborCache(ec.B, row.N, tdt, dev, slots=1, max_taps=row.taps, pairs_per_point=row.ppp, max_cin=row.ci,
                                 max_cout=row.co, sparse_neighbourhoods=sparse)
    wrong = []
    for run in row.runs:
        if run != ec.STATELESS:
            cache.matmul_precision = run
        got, fseen, bseen = _run(dev, tensors, s, None if run == ec.STATELESS else cache)
        fams = (_family(bseen, False), _family(fseen, True))
        if fams != (row.fam_b, row.fam_f):
            wrong.append((run, "backward / forward family", fams, bseen, fseen))
        # the matrix-core passes ran in the precision asked for
        bf16 = run == ec.MEDIUM
        if row.fam_f == ec.MC and (fseen["deep_gemm_bf16_kernel"] > 0, fseen["deep_gemm_kernel"] > 0) != (bf16, not bf16):
            wrong.append((run, "forward precision", fseen))
        if row.fam_b == ec.MC and ((bseen["deep_gemm_bf16_kernel"] > 0, bseen["deep_gemm_kernel"] > 0) != (bf16, not bf16) or
                                   (bseen["deep_dw_bf16_kernel"] > 0, bseen["deep_dw_kernel"] > 0) != (bf16, not bf16)):
            wrong.append((run, "backward precision", bseen))
        ref = rounded if (bf16 and rounded is not None) else plain
        for name, g, r in zip(("y", "dX", "dW"), got, ref):
            assert g.dtype == r.dtype and g.shape == r.shape, (run, name, g.dtype, g.shape)
            if not np.array_equal(g, r):
                wrong.append((run, name, _where(g, r)))
    assert not wrong, wrong


@pytest.mark.parametrize("s", (ec.S1, ec.S2), ids=lambda s: "s%d%d%d" % s)
def test_hand_over_rows_on_one_cache(dev, s):
    """The two hand-over rows (9 -> 9, 32 -> 64) in turn on ONE cache of four pair slots per point, in both precisions:
    what one layer's overflowed tiles left behind does not reach the next, and the results are still the exact sums."""
    rows = [k for k, r in enumerate(ec.ROWS) if r.ppp]
    assert [(ec.ROWS[k].ci, ec.ROWS[k].co) for k in rows] == [(9, 9), (32, 64)]
    N = ec.ROWS[rows[0]].N
    cache = op.NeighborCache(ec.B, N, torch.float32, dev, slots=1, max_taps=27, pairs_per_point=4, max_cin=32, max_cout=64)
    wrong = []
    for mode in (ec.HIGHEST, ec.MEDIUM, ec.HIGHEST):
        cache.matmul_precision = mode
        for k in rows:
            row = ec.ROWS[k]
            assert cache.fits(ec.B, row.N, torch.float32, dev, row.taps, row.ci, row.co)
            tensors = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ec.inputs(k))
            got, fseen, bseen = _run(dev, tensors, s, cache)
            fams = (_family(bseen, False), _family(fseen, True))
            if fams != (row.fam_b, row.fam_f):
                wrong.append((mode, k, "backward / forward family", fams))
            for name, g, r in zip(("y", "dX", "dW"), got, _reference((k, s))[0]):
                if not np.array_equal(g, r):
                    wrong.append((mode, k, name, _where(g, r)))
    assert not wrong, wrong
