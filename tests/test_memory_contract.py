"""The memory contract of every entry point (-m gpu): each caller-owned region of include/conv3p.h -- `workspace`,
`scratch`, `cache` -- at exactly its declared size, between guards, and dirty.  tests/memory_rig.py is the rig; the calls
are the table of tests/stream_contract_cases.py, at its shapes, plus targeted cases below for the places where a size
function and a kernel could disagree by a row or a tile and which the table's smallest shapes do not reach.

Per case, with `expected` from one plain run (pooled workspaces with their 1 MiB floor, no shim):
  R0  the same call with `X_bytes - 1` is refused with CONV3P_ERR_WORKSPACE (seven grid calls: with the status their own
      paragraph of the header documents, memory_rig.REFUSES_WITH); its outputs, pre-filled with a sentinel, the body of a
      region that keeps state and all guards are unchanged;
  R1  every region sits at exactly its declared size, and after every run every guard of every region the call touched
      is intact;
  R2  (per-call regions) runs with the body pre-filled with 0x00, with 0xFF and with the leftover of the poison half's
      run give bit-identical outputs;
  R3  the exact-size runs' outputs are bit-identical to `expected`, unless the case is listed in ROUTE_BY_SIZE with the
      source line that makes the route depend on the scratch offered; such a case is compared with its family's reference.

First the rig proves on four plants in plain torch that it can see; every test below depends on that fixture.

Out of scope: the bounds of OUTPUT tensors.  Their sizes are the caller's shapes, not a declaration of the library;
`Guarded` in tests/test_fc_shapes.py remains the only such check.  The ad hoc workspace fills of test_fc_shapes.py and
test_wide_sort.py stay as they are.  conv3p_grid_agglomerate_segments is declared in include/conv3p_graph.h, which the
region finder does not read, and has no case in the table.
"""
import numpy as np
import pytest
import torch

from tests import memory_rig as rig, stream_contract_cases as table
from tests.launch_census_cases import F32, F64, VOX
from tests.parity_util import TOL, make_case, rel_err
from tests.stream_rig import Case
from tests.test_dispatch_map import EXT

pytestmark = pytest.mark.gpu

# C entry points with a region that no case of the table reaches, and why.
NOT_REACHED = {}
# Cases whose exact-size run legitimately takes another route than the pooled run: case -> (file of
# pointwise_amd/csrc, the line that decides it).  None: at the table's and the targeted shapes every declared size gives
# the route the floor gives (a stateless conv3p workspace at B x N = 2 x 130 is already above the floor).
ROUTE_BY_SIZE = {}

REGIONS = rig.regions()


@pytest.fixture(scope="module")
def seeing():
    """(device, the verdicts of the four plants on it, the index R0 finds output tensors in); fails unless the rig sees
    exactly what was planted."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from pointwise_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    plants = rig.judge_plants(dev)
    blind = []
    if rig.all_changed(plants["write_past"]) != {(rig.PLANT_BYTES, rig.PLANT_BYTES)}:
        blind.append("a write one byte past the body")
    if rig.all_changed(plants["write_before"]) != {(-1, -1)}:
        blind.append("a write one byte before the body")
    if plants["reads_stale"].dirty["0xFF"] != [0] or plants["reads_stale"].dirty["leftover"] != [0]:
        blind.append("an output that depends on what the body held")
    if rig.all_changed(plants["well_behaved"]) or rig.any_dirty(plants["well_behaved"]):
        blind.append("(the well-behaved op is reported)")
    assert not blind, "the rig does not see %s: nothing below would prove anything" % ", ".join(blind)
    index = rig.TensorIndex(dev)
    yield dev, plants, index
    index.close()


def test_the_rig_sees_a_write_past_the_body(seeing):
    v = seeing[1]["write_past"]
    assert all(list(per.values()) == [(rig.PLANT_BYTES, rig.PLANT_BYTES)] for per in v.changed.values()), v.changed
    assert not rig.any_dirty(v)


def test_the_rig_sees_a_write_before_the_body(seeing):
    v = seeing[1]["write_before"]
    assert all(list(per.values()) == [(-1, -1)] for per in v.changed.values()), v.changed
    assert not rig.any_dirty(v)


def test_the_rig_sees_a_read_of_a_stale_word(seeing):
    v = seeing[1]["reads_stale"]
    assert v.dirty == {"0x00": [], "0xFF": [0], "leftover": [0]} and not rig.all_changed(v), (v.dirty, v.changed)


def test_the_rig_passes_a_well_behaved_op(seeing):
    v = seeing[1]["well_behaved"]
    assert not rig.all_changed(v) and not rig.any_dirty(v) and list(v.sizes.values()) == [rig.PLANT_BYTES]


# ------------------------------------------------------------------------------------------------ the rules
def contract(seeing, monkeypatch, name, build, reaches=None, reference=None, bitwise=True, short=True):
    """R0 - R3 for one case.  build() -> a Case (made with the caches in arenas); reaches: the C functions run() enters, or
    None if not claimed; reference(outputs): asserts host copies of run()'s outputs against the family's reference;
    bitwise=False: the case is not reproducible bit for bit (R2 and R3's bit comparison are replaced by `reference`)."""
    from pointwise_amd import _lib
    dev, _, index = seeing
    rig._CACHE_ARENAS.clear()
    rig.cache_in_arena(monkeypatch)
    case = build()
    case.reset()
    expected = rig._host(case.run())                     # the plain run: pooled workspaces, no shim
    torch.cuda.synchronize(dev)
    rig.patch_workspace_floor(monkeypatch)
    with rig.Shim(_lib.load(), dev, index) as shim:
        v = rig.judge(shim.around(case), shim, dev)
        short_out = shim.short_run(shim.around(case)) if short else None
    for label, nbytes in v.sizes.items():
        print("%s: %s, %d bytes" % (name, label, nbytes))
    entered = {key[0] for key in shim.arenas}
    if reaches is not None:
        want = {f for f in reaches if f in REGIONS}
        assert entered <= want, (sorted(entered), sorted(want))
        missed = {f: table_reason(name, f) for f in want - entered}
        assert all(missed.values()), "%s: no region of %s was seen: the shim is blind to them" % (name, sorted(missed))
    # R1
    assert not shim.not_arenas, "%s: a region that keeps state is not an arena of its declared size: %s" % (name, shim.not_arenas)
    assert not any(v.changed.values()), "%s: %s" % (name, rig.describe(v.changed))
    late = {a.label + " %#x" % p: a.intact() for p, a in rig._CACHE_ARENAS.items() if a.intact() is not None}
    assert not late, "%s: guards of a cache changed: %s" % (name, late)
    # R2
    if bitwise:
        assert not rig.any_dirty(v), "%s: outputs depend on what the regions held: %s differ from the 0x00 run" % (name, dict(v.dirty))
    # R0
    if short:
        bad = [r for r in shim.refusals if r[2]]
        assert not bad, "%s: one byte short: %s" % (name, bad)
        refused = {r[0] for r in shim.refusals}
        assert refused == entered - set(rig.NO_DECLARED_SIZE), (sorted(refused), sorted(entered))
    # R3
    runs = list(v.outputs.items()) + ([("after the refused calls", short_out)] if short else [])
    if bitwise and name not in ROUTE_BY_SIZE:
        for fill, outs in runs:
            assert not rig.differing(expected, outs), "%s: outputs %s of the exact-size run [%s] differ from the plain run's" % (
                name, rig.differing(expected, outs), fill)
        if reference is not None:
            reference(expected)
    else:
        assert reference is not None, "%s needs its family's reference" % name
        for fill, outs in [("plain", expected)] + runs:
            reference(outs)
    return v


# A function a case reaches may take no region in that call; which, and the header sentence that says so.
NO_REGION_THIS_CALL = {
    ("assemble_batch/plain", "conv3p_provider_batch_f32"): "Scratch from conv3p_provider_workspace_bytes (0 without SORT).",
}


def table_reason(case, function):
    return NO_REGION_THIS_CALL.get((case, function), "")


def _layer_reference(name, real):
    """The conv3p family's own reference for the table's `conv3p+conv3p_grad/...` cases: the CPU oracle at
    tests/parity_util.TOL, as tests/test_gpu_parity.py compares."""
    from oracle import oracle
    P, X, W, dY = real
    s = (int(name.split("/s")[1][0]),) * 3
    memo = {}

    def check(outs):
        if not memo:
            memo["y"] = oracle.forward(P, X, W, s, VOX)
            memo["dx"], memo["dw"] = oracle.backward(dY, P, X, W, s, VOX)
        _against_oracle(outs, memo, P.dtype)
    return check


def _against_oracle(outs, ref, dtype, tol_scale=1.0):
    tol_y, tol_w = TOL[np.dtype(dtype)]
    e = rel_err(outs[0].numpy(), ref["y"])
    print("y", e)
    assert e <= tol_y * tol_scale, ("y", e)
    if len(outs) > 1:
        ex, ew = rel_err(outs[1].numpy(), ref["dx"]), rel_err(outs[2].numpy(), ref["dw"])
        print("dX", ex, "dW", ew)
        assert ex <= tol_y * tol_scale, ("dX", ex)
        assert ew <= tol_w * tol_scale, ("dW", ew)


@pytest.mark.parametrize("name", table.NAMES)
def test_memory_contract(seeing, monkeypatch, name):
    dev = seeing[0]
    e = table.ENTRIES[table.NAMES.index(name)]
    real, poison = e.halves()
    reference = _layer_reference(name, real) if name in ROUTE_BY_SIZE and name.startswith("conv3p+conv3p_grad/") else None
    contract(seeing, monkeypatch, name, lambda: e.build(dev, real, poison), reaches=e.reaches, reference=reference)


# ------------------------------------------------------------------------------------------------ targeted cases
_ORACLE = {}


def _oracle(key, real, s, backward):
    """y (and dX, dW) of the CPU oracle, once per key."""
    from oracle import oracle
    if key not in _ORACLE:
        P, X, W, dY = real
        ref = {"y": oracle.forward(P, X, W, s, VOX, nthreads=8)}
        if backward:
            ref["dx"], ref["dw"] = oracle.backward(dY, P, X, W, s, VOX, nthreads=8)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _op_case(dev, real, poison, s, cache_kw=None, backward=True, trust_cache=False):
    """conv3p (+ conv3p_grad) as a Case: stateless, or through a NeighborCache(**cache_kw) made in here.  trust_cache: the
    Python mirror's own fits() is waived, so that a cache sized for no channels at all reaches the library."""
    from pointwise_amd import conv3p_op as op
    tp, tx, tw, tdy = inputs = table.upload(dev, real)
    B, N = tp.shape[0], tp.shape[1]
    cache = None
    if cache_kw is not None:
        cache = op.NeighborCache(B, N, tp.dtype, dev, **cache_kw)
        if trust_cache:
            cache.fits = lambda *a: True
        assert cache.fits(B, N, tp.dtype, dev, tw.shape[0] * tw.shape[1] * tw.shape[2], tw.shape[3], tw.shape[4])

    def run():
        out = [op.conv3p(tp, tx, tw, s, VOX, cache=cache)]
        if backward:
            out += list(op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache))
        return out
    return Case(inputs, table.upload(dev, poison), run, table._cache_reset(cache))


def _two(kind, B, N, ci, co, taps, seed, dt=F32):
    return [make_case(kind, B, N, ci, co, EXT[taps], seed=sd, dtype=dt) for sd in (seed, seed + 5000)]


FWD, BWD = "conv3p_forward_", "conv3p_backward_"


@pytest.mark.parametrize("ci,co", [(9, 9), (32, 64), (36, 13)], ids=["9to9", "32to64", "36to13"])
@pytest.mark.parametrize("channels", ["sized", "zero"])
def test_pair_buffer_overflow_stays_inside_the_cache(seeing, monkeypatch, ci, co, channels):
    """The construction of test_pair_buffer_overflow_falls_back_correctly (B = 2, N = 300, a room, pairs_per_point = 4):
    the pair allocator overshoots its region ("headroom for the allocator's transient overshoot", carve()).  Once with the
    cache sized for the layer, and once with max_cin = max_cout = 0, so that the pair region is the last thing in the
    buffer: forward only there (such a cache has no room for a backward's partials), and a layer the header says needs a
    cache sized for it ("Wide (matrix-core) layers need a cache sized for them") must be refused with
    CONV3P_ERR_WORKSPACE, guards intact.  Which tiles overflow is a race between the tiles of a cloud (see
    tests/test_backward_riders.py), so runs are compared with the oracle at that test's tolerances, not bit for bit."""
    from pointwise_amd import conv3p_op as op
    dev = seeing[0]
    real, poison = [make_case("room", 2, 300, ci, co, seed=sd) for sd in (970, 5970)]
    zero = channels == "zero"
    kw = dict(slots=1, max_taps=27, pairs_per_point=4, max_cin=0 if zero else ci, max_cout=0 if zero else co)
    ref = _oracle(("overflow", ci, co), real, (1, 1, 1), True)
    name = "pair-overflow/%dto%d/%s" % (ci, co, channels)
    sfx = "f32"
    reaches = ["conv3p_forward_cached_" + sfx] + ([] if zero else ["conv3p_backward_cached_" + sfx])
    if zero and (ci, co) == (32, 64):
        rig._CACHE_ARENAS.clear()
        rig.cache_in_arena(monkeypatch)
        case = _op_case(dev, real, poison, (1, 1, 1), kw, backward=False, trust_cache=True)
        with pytest.raises(op.Conv3pRuntimeError, match="status 2"):
            case.run()
        torch.cuda.synchronize(dev)
        assert [a.intact() for a in rig._CACHE_ARENAS.values()] == [None]
        return
    contract(seeing, monkeypatch, name, lambda: _op_case(dev, real, poison, (1, 1, 1), kw, backward=not zero, trust_cache=zero),
             reaches=reaches, reference=lambda outs: _against_oracle(outs, ref, F32), bitwise=False)


@pytest.mark.parametrize("cached", [False, True], ids=["stateless", "cached"])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("taps", [27, 36, 125])
def test_tap_counts_on_both_sides_of_the_qbm_planes(seeing, monkeypatch, taps, dt, cached):
    """`qbm` has one plane of tap bits up to 32 taps, two up to 64, four above (carve()): 27, 36 and 125 taps, 9 -> 9 at
    B = 2, N = 130.  fp64 at 125 taps is the generic kernels' (tests/test_dispatch_map.py: not deterministic): that case
    is compared with the oracle in every run, every other one bit for bit as well."""
    dev = seeing[0]
    ext = {27: (3, 3, 3), 36: (3, 3, 4), 125: (5, 5, 5)}[taps]
    real, poison = [make_case("modelnet", 2, 130, 9, 9, ext, seed=sd, dtype=dt) for sd in (7300 + taps, 12300 + taps)]
    sfx = "f32" if dt == F32 else "f64"
    mid = "cached_" if cached else ""
    kw = dict(slots=1, max_taps=taps, max_cin=9, max_cout=9) if cached else None
    ref = _oracle(("taps", taps, sfx), real, (1, 1, 1), True)
    contract(seeing, monkeypatch, "taps%d/%s/%s" % (taps, sfx, "cached" if cached else "stateless"),
             lambda: _op_case(dev, real, poison, (1, 1, 1), kw), reaches=[FWD + mid + sfx, BWD + mid + sfx],
             reference=lambda outs: _against_oracle(outs, ref, dt), bitwise=not (taps == 125 and dt == F64))


@pytest.mark.parametrize("N", [16384, 16385])
def test_with_and_without_the_fused_search_tables(seeing, monkeypatch, N):
    """`ftab`, the fused search's per-tile window tables, exists only for N <= 16384 (carve()): the last size with them
    and the first without, B = 1, 3 -> 9, 27 taps, stateless forward and backward."""
    dev = seeing[0]
    real, poison = _two("modelnet", 1, N, 3, 9, 27, 7400)
    ref = _oracle(("ftab", N), real, (1, 1, 1), True)
    contract(seeing, monkeypatch, "ftab/N%d" % N, lambda: _op_case(dev, real, poison, (1, 1, 1)),
             reaches=[FWD + "f32", BWD + "f32"], reference=lambda outs: _against_oracle(outs, ref, F32))


@pytest.mark.parametrize("ci,co", [(64, 64), (300, 64)], ids=["matrix-core-64to64", "blocked-300to64"])
def test_forward_and_backward_workspaces_at_their_own_sizes(seeing, monkeypatch, ci, co):
    """A matrix-core shape and a blocked one at B = 2, N = 1024 (rows of tests/test_abi_sizes_host.py): the forward at
    exactly conv3p_workspace_bytes(FORWARD), which leaves out the backward-only scratch (the `forward_part` placement of
    conv3p_abi_blocks.hpp), the backward at conv3p_workspace_bytes(BACKWARD)."""
    dev = seeing[0]
    real, poison = _two("modelnet", 2, 1024, ci, co, 27, 7500 + ci)
    ref = _oracle(("passes", ci, co), real, (1, 1, 1), True)
    contract(seeing, monkeypatch, "passes/%dto%d" % (ci, co), lambda: _op_case(dev, real, poison, (1, 1, 1)),
             reaches=[FWD + "f32", BWD + "f32"], reference=lambda outs: _against_oracle(outs, ref, F32))


@pytest.mark.parametrize("cin,ncls", [(3, None), (9, 13)], ids=["cls4", "seg5"])
def test_stack_scratch_and_caches_in_arenas(seeing, monkeypatch, cin, ncls):
    """A Conv3pStack forward and backward (the stacks of tests/test_backward_riders.py, 2 x 130) with its backward scratch
    and both caches in arenas; fused launches stay off, as in the launch census.  Against the stack's oracle at that
    test's tolerance."""
    from pointwise_amd import stack
    from tests.stack_ref import stack_reference
    from tests.test_backward_riders import STACK_TOL, _case
    dev = seeing[0]
    B, N = 2, 130
    P, X, ups = _case(cin, ncls, B, N, F32)
    P2, X2, ups2 = _case(cin, ncls, B + 1, N, F32)       # (another seed of the same generator)
    P2, X2, ups2 = P2[:B], X2[:B], [u[:B] for u in ups2]

    def build():
        st = stack.Conv3pStack(cin, ncls, device=dev, seed=47, fused_launch=False)
        st.prepare(B, N)
        tp, tx, *tups = inputs = table.upload(dev, [P, X] + ups)

        def reset():
            st._pending.clear()
            st._inflight = st._saved = None
            st.fused_grad.zero_()
            table._cache_reset(*st._caches)()

        def run():
            acts = st.forward(tp, tx)
            dx, grads = st.backward(tups)
            assert st.c_stack
            return list(acts) + [dx, grads]
        build.st = st
        return Case(inputs, table.upload(dev, [P2, X2] + ups2), run, reset)

    def reference(outs):
        st = build.st
        _, ref_dx, ref_dws = stack_reference(P, X, [f.cpu().numpy() for f in st.filters], [(s, s, s) for _, _, s in st.layers],
                                             stack.HIDDEN, grad_head=ups[0] if ncls else None,
                                             grad_concat=None if ncls else np.concatenate(ups, axis=2), nthreads=8,
                                             memo=("memory-contract", cin, ncls))
        dx, fg = outs[-2].numpy(), outs[-1].numpy()
        assert rel_err(dx, ref_dx) <= STACK_TOL[F32], ("dX", rel_err(dx, ref_dx))
        o = 0
        for l, r in enumerate(ref_dws):
            assert rel_err(fg[o:o + r.size], r.ravel()) <= STACK_TOL[F32], ("grad_filter", l)
            o += r.size
        assert o == fg.size

    v = contract(seeing, monkeypatch, "stack/%s" % ("seg5" if ncls else "cls4"), build,
                 reaches=["conv3p_stack_forward_f32", "conv3p_stack_backward_f32"], reference=reference)
    assert any("`scratch`" in label for label in v.sizes) and any("`cache`" in label for label in v.sizes), list(v.sizes)
