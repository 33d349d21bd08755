"""The premises of the exact-arithmetic rows (tests/exact_cases.py), on the CPU: every population a power of two, the
sums of the terms' magnitudes below 2^24 units -- with and without the bf16 rounding -- and the reference's own float32
and float64 loops (oracle.forward / backward) equal to the float64 sums of tests/exact_ref.py bit for bit.  What
tests/test_exact_families.py then asserts of the kernels is asserted here of the reference."""
import concurrent.futures

import numpy as np
import pytest

from oracle import conv3p_numpy, oracle
from tests import exact_cases as ec
from tests import exact_ref as er

IDS = [ec.case_id(c) for c in ec.CASES]
_DONE = {}


def _loops(case):
    k, s = case
    P, X, W, dY = ec.inputs(k)
    return (oracle.forward(P, X, W, s, ec.VOX),) + oracle.backward(dY, P, X, W, s, ec.VOX)


def _sums(case):
    k, s = case
    row = ec.ROWS[k]
    P, X, W, dY = ec.inputs(k)
    out = {"cnt": oracle.neighbor_count(P.astype(np.float32), er.EXT[row.taps], s, ec.VOX),
           "exact": er.exact_sums(P, X, W, dY, s, ec.VOX)}
    if row.wide:
        out["rne"] = er.exact_sums(P, X, W, dY, s, ec.VOX, er.bf16_rne)
        out["trunc"] = er.exact_sums(P, X, W, dY, s, ec.VOX, er.bf16_trunc)
    return out


@pytest.fixture(scope="module")
def done():
    """Every case's populations, exact sums and oracle results, computed once.  The reference's loops take seconds on a
    wide layer, so cases run several at a time, the longest first (the C loops and numpy's products release the
    interpreter lock).  Where numpy's own threads can be held to one, the exact sums run in the pool as well; where
    not, they would only get in each other's way there and run here, beside the pool."""
    if not _DONE:
        oracle.lib()
        cases = sorted(ec.CASES, key=lambda c: -ec.ROWS[c[0]].N * ec.ROWS[c[0]].ci * ec.ROWS[c[0]].co)
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            threadpool_limits = None
        if threadpool_limits:
            with threadpool_limits(limits=1), concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
                _DONE.update(zip(cases, pool.map(lambda c: dict(_sums(c), oracle=_loops(c)), cases)))
        else:
            with concurrent.futures.ThreadPoolExecutor(max_workers=6) as pool:
                loops = [pool.submit(_loops, c) for c in cases]
                for c, f in zip(cases, loops):
                    _DONE[c] = dict(_sums(c), oracle=f.result())
    return _DONE


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_populations_are_powers_of_two_with_eights_and_inner_holes(done, case):
    cnt = done[case]["cnt"]
    seen = set(np.unique(cnt).tolist())
    assert seen <= {0, 1, 2, 4, 8} and 8 in seen and 0 in seen, seen
    # an empty tap between two populated ones of the same centre
    F = cnt.shape[-1]
    pop = cnt.reshape(-1, F) > 0
    first = np.where(pop.any(1), pop.argmax(1), F)
    last = np.where(pop.any(1), F - 1 - pop[:, ::-1].argmax(1), -1)
    f = np.arange(F)[None]
    assert (~pop & (f > first[:, None]) & (f < last[:, None])).any()


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_headroom_stays_below_two_to_the_24_units_and_results_are_whole_units(done, case):
    for which in ("exact", "rne", "trunc"):
        if which not in done[case]:
            continue
        y, dx, dw, head = done[case][which]
        for name, a in (("y", y), ("dX", dx), ("dW", dw)):
            total, unit = head[name]
            assert unit == 2.0 ** -3, (which, name, unit)
            assert total / unit < er.LIMIT, (which, name, total / unit)
            assert er.in_units(a, unit), (which, name)


@pytest.mark.parametrize("case", ec.CASES, ids=IDS)
def test_the_reference_loops_equal_the_exact_sums_bit_for_bit(done, case):
    dt = ec.ROWS[case[0]].dt
    for name, got, ref in zip(("y", "dX", "dW"), done[case]["oracle"], done[case]["exact"]):
        assert got.dtype == dt
        assert np.array_equal(got, ref.astype(dt)), (name, int((got != ref.astype(dt)).sum()), "elements differ")
        assert np.array_equal(ref.astype(dt).astype(np.float64), ref), name + ": not representable in the row's type"


SMALL = [c for c in ec.CASES if ec.ROWS[c[0]].ci * ec.ROWS[c[0]].co <= 81 and ec.ROWS[c[0]].taps <= 65]


@pytest.mark.parametrize("case", SMALL, ids=[ec.case_id(c) for c in SMALL])
def test_the_brute_force_restatement_agrees_on_the_smallest_rows(done, case):
    k, s = case
    P, X, W, dY = ec.inputs(k)
    y = conv3p_numpy.forward(P, X, W, s, ec.VOX)
    dx, dw = conv3p_numpy.backward(dY, P, X, W, s, ec.VOX)
    for name, got, ref in zip(("y", "dX", "dW"), (y, dx, dw), done[case]["exact"]):
        assert np.array_equal(got, ref.astype(P.dtype)), name


@pytest.mark.parametrize("case", [c for c in ec.CASES if ec.ROWS[c[0]].wide],
                         ids=[ec.case_id(c) for c in ec.CASES if ec.ROWS[c[0]].wide])
def test_rounding_rows_tell_nearest_even_from_no_rounding_and_from_truncation(done, case):
    """More than half of the elements that some term enters, of each output the wide operand enters, differ between the rounded reference and
    the unrounded one, and between it and the truncating one; the outputs it does not enter are the same in all three."""
    wide = ec.ROWS[case[0]].wide
    for k, name in enumerate(("y", "dX", "dW")):
        exact, rne, trunc = (done[case][w][k] for w in ("exact", "rne", "trunc"))
        if name in ec.ROUNDED_OUTPUTS[wide]:
            hit = done[case]["exact"][3]["terms"][name] > 0     # (a tap no pair of the clouds falls into leaves dW[f] zero)
            assert hit.mean() > 0.25, (name, float(hit.mean()))
            assert np.mean(rne[hit] != exact[hit]) > 0.5, (name, float(np.mean(rne[hit] != exact[hit])))
            assert np.mean(rne[hit] != trunc[hit]) > 0.5, (name, float(np.mean(rne[hit] != trunc[hit])))
        else:
            assert np.array_equal(rne, exact) and np.array_equal(trunc, exact), name


def test_every_operand_position_is_rounded_in_some_row():
    wides = {ec.ROWS[k].wide for k, _ in ec.CASES}
    assert {"X", "W", "dY"} <= wides
    # X: M_f and the X rows; W: the forward's W and the grad_input pass's W^T; dY: G_f' there and the G rows
    assert {o for w in ("X", "W", "dY") for o in ec.ROUNDED_OUTPUTS[w]} == {"y", "dX", "dW"}
    for ci, co in ((37, 43), (128, 256), (256, 256)):
        for s in (ec.S1, ec.S2):
            assert {r.wide for r in ec.ROWS if (r.ci, r.co) == (ci, co) and r.wide and s in r.strides} == {"X", "W", "dY"}


def test_the_tables_span_tiles_sizes_densities_and_padded_classes(done):
    rows = ec.ROWS
    assert {65, 130, 256, 300, 700} <= {r.N for r in rows}
    assert all(r.N > 64 for r in rows)                          # more than one 64-point tile per cloud
    assert max(r.N * max(r.ci, r.co) for r in rows) == 700 * 256
    assert all(r.taps % 2 == 1 and all(e % 2 == 1 for e in er.EXT[r.taps]) for r in rows)
    # both sides of the search's rule for squeezing a tile's lists (more than 40 hits per centre)
    mean = {c: done[c]["cnt"].sum() / done[c]["cnt"][..., 0].size for c in ec.CASES}
    assert any(m >= 40 for (k, s), m in mean.items() if s == ec.S1)
    assert any(m <= 30 for (k, s), m in mean.items() if s != ec.S1)
    # every instantiation of the matrix-core kernels: CONV3P_DEEP_SHAPES of conv3p_abi_routes.hpp
    pad = lambda c: next(p for p in (32, 64, 128, 256) if c <= p)
    classes = {(pad(r.ci), pad(r.co)) for r in rows if ec.MC in (r.fam_b, r.fam_f) and max(r.ci, r.co) <= 256}
    assert classes == {(a, b) for a in (32, 64, 128) for b in (32, 64, 128)} | {(128, 256), (256, 256), (256, 128)}
    for size in (32, 64, 128, 256):
        assert any(size in c for c in classes)
    assert any(r.ci > 256 for r in rows) and any(r.co > 256 for r in rows)


def test_hand_over_rows_cannot_hold_their_lists(done):
    """pairs_per_point rows: every cloud's lists are longer than the cache's pair slots for it, so tiles overflow."""
    cases = [c for c in ec.CASES if ec.ROWS[c[0]].ppp]
    assert {(ec.ROWS[k].ci, ec.ROWS[k].co) for k, _ in cases} == {(9, 9), (32, 64)}
    for c in cases:
        row = ec.ROWS[c[0]]
        assert (done[c]["cnt"].sum(axis=(1, 2)) > 4 * row.ppp * row.N).all()


def test_bf16_rounding_on_the_bit_pattern():
    f = lambda v: float(er.bf16_rne(np.float32(v)))
    assert (f(257), f(259), f(-257), f(511)) == (256.0, 260.0, -256.0, 512.0)
    assert er.bf16_rne(np.float32(0.1)).view(np.uint32) >> 16 == 0x3DCD
    assert er.bf16_trunc(np.float32(0.1)).view(np.uint32) >> 16 == 0x3DCC
    for z in (np.float32(0.0), np.float32(-0.0)):
        assert er.bf16_rne(z).view(np.uint32) == z.view(np.uint32)
        assert er.bf16_trunc(z).view(np.uint32) == z.view(np.uint32)
    t = lambda v: float(er.bf16_trunc(np.float32(v)))
    assert (t(257), t(259), t(-257), t(511)) == (256.0, 258.0, -256.0, 510.0)
    a = np.arange(-600, 601, dtype=np.float32)
    assert np.array_equal(er.bf16_rne(a)[np.abs(a) <= 256], a[np.abs(a) <= 256])
