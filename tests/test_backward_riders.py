"""Reduction riders of the stack-level backward (-m gpu).

conv3p_stack_backward sums a layer's grad_filter partials inside the NEXT layer's backward launch: workgroups appended
after the tile workgroups (reduce_rider, csrc/conv3p_kernels.hpp) add them in the order of the closing reduction, which
is left with the first layer's partials only.  The op-by-op composition (Conv3pStack(c_stack=False)) keeps one reduction
per op call.  Both must give the same bits.

Shapes: one tile (1 x 64), a ragged last tile with a batch that is no multiple of the 8 XCDs (3 x 130), and 32 tiles per
cloud (2 x 2048: 64 partial slots and more, every stripe of the summation order in use).  Stacks: the classification
model's four layers and the segmentation model's five (13 classes), fp32 and fp64, with the SPARSE hint, the DENSE hint
and neither (the dilated layers then launch both backward kernels and the slot's regime word lets one run: the rider
goes with the first of the two whatever the word says).

Tolerances against the CPU oracle: tests/parity_util.TOL is per op call (fp32 1e-5 for grad_input, 2e-5 for
grad_filter; fp64 1e-12); a stack chains up to five forward and five backward ops, so the figures of
tests/test_stack_descriptors.py hold here: 5e-5 in fp32 (five ops at 1e-5), 1e-11 in fp64 (1e-12 over at most nine
chained ops)."""
import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op, stack, synth
from tests.parity_util import TOL, rel_err
from tests.stack_ref import stack_reference

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
STACK_TOL = {F32: 5 * TOL[np.dtype(F32)][0], F64: 10 * TOL[np.dtype(F64)][0]}
SHAPES = [(1, 64), (3, 130), (2, 2048)]
STACKS = [(3, None), (9, 13)]          # (in_channels, num_class): 4 layers / 5 layers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _case(cin, ncls, B, N, dt):
    seed = 5200 + 7 * B + N
    P = (synth.modelnet_like(B, N, seed) if ncls is None else synth.room_like(B, N, seed)).astype(dt)
    X = synth.features(B, N, cin, seed + 1, points=P, dtype=dt)
    ups = [synth.upstream_grad(B, N, stack.HIDDEN, seed + 2 + i, dtype=dt) for i in range(4)] if ncls is None else \
        [synth.upstream_grad(B, N, ncls, seed + 2, dtype=dt)]
    return P, X, ups


def _reference(st, cin, ncls, B, N, dt, P, X, ups, memo):
    return stack_reference(P, X, [f.cpu().numpy() for f in st.filters], [(s, s, s) for _, _, s in st.layers], stack.HIDDEN,
                           grad_head=ups[0] if ncls else None, grad_concat=None if ncls else np.concatenate(ups, axis=2),
                           nthreads=8, memo=memo)


def _run(st, tp, tx, tups, calls):
    out = []
    for _ in range(calls):
        st.forward(tp, tx)
        dx, fg = st.backward(tups)
        out.append((dx.clone(), fg.clone()))
    return out


@pytest.mark.parametrize("hint", [True, False, None], ids=["sparse", "dense", "nohint"])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("cin,ncls", STACKS, ids=["cls4", "seg5"])
@pytest.mark.parametrize("B,N", SHAPES, ids=["1x64", "3x130", "2x2048"])
def test_stack_backward_with_riders_equals_the_op_by_op_backward(dev, B, N, cin, ncls, dt, hint):
    P, X, ups = _case(cin, ncls, B, N, dt)
    tdt = torch.float32 if dt == F32 else torch.float64
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tx, tups = t(P), t(X), [t(u) for u in ups]
    res = {}
    for c_stack in (True, False):
        st = stack.Conv3pStack(cin, ncls, device=dev, dtype=tdt, seed=47, c_stack=c_stack)
        st.sparse_neighbourhoods = hint
        res[c_stack] = _run(st, tp, tx, tups, 2 if c_stack else 1)
        assert st.c_stack == c_stack, "the stack entry points must serve the models' stacks"
    (dx, fg), (dx2, fg2) = res[True]
    dx_ops, fg_ops = res[False][0]
    # bit for bit the op-by-op composition, whose every op call reduces its own partials
    assert torch.equal(fg, fg_ops), ("fused_grad", rel_err(fg.cpu().numpy(), fg_ops.cpu().numpy()))
    assert torch.equal(dx, dx_ops), ("dX", rel_err(dx.cpu().numpy(), dx_ops.cpu().numpy()))
    # no stale partials: a second call on the same stack object gives the same bits
    assert torch.equal(fg, fg2) and torch.equal(dx, dx2)
    # the oracle (one reference per stack, shape and dtype, shared by the three hints)
    _, ref_dx, ref_dws = _reference(st, cin, ncls, B, N, dt, P, X, ups, ("riders", cin, ncls, B, N, np.dtype(dt).name))
    tol = STACK_TOL[dt]
    e = rel_err(dx.cpu().numpy(), ref_dx)
    print("dX", e)
    assert e <= tol, ("dX", e)
    o = 0
    for l, r in enumerate(ref_dws):
        g = fg[o:o + r.size].view(r.shape).cpu().numpy()
        o += r.size
        e = rel_err(g, r)
        print("grad_filter", l, e)
        assert e <= tol, ("grad_filter", l, e)
    assert o == fg.numel()


def test_riders_beside_tiles_that_search_themselves(dev):
    """Caches too small for the pair lists (pairs_per_point = 6, the construction of
    test_fused_stack_launch_with_overflowed_pair_buffers): most tiles' pair segments overflow and the tile workgroups
    search for themselves, with the riders behind them in the same launches.  WHICH tiles overflow is a race between the
    tiles of a cloud and an overflowed tile sums in another order, so two caches need not agree bit for bit: the stack
    entry point and the op-by-op composition are compared within rounding (2e-6, as that test does) and both runs against
    the oracle."""
    B, N, cin = 5, 900, 3
    P = synth.modelnet_like(B, N, seed=15)
    X = synth.features(B, N, cin, 16, points=P)
    ups = [synth.upstream_grad(B, N, stack.HIDDEN, 170 + i) for i in range(4)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tx, tups = t(P), t(X), [t(u) for u in ups]
    res = {}
    for c_stack in (True, False):
        st = stack.Conv3pStack(cin, None, device=dev, seed=3, c_stack=c_stack, fused_launch=False)
        st.sparse_neighbourhoods = True
        for i in (0, 1):
            st._caches[i] = op.NeighborCache(B, N, torch.float32, dev, slots=len(st.layers), max_taps=27, max_cin=9, max_cout=9,
                                             pairs_per_point=6, sparse_neighbourhoods=True)
        res[c_stack] = _run(st, tp, tx, tups, 2 if c_stack else 1)
        assert st.c_stack == c_stack
    _, ref_dx, ref_dws = _reference(st, cin, None, B, N, F32, P, X, ups, None)
    ref_fg = np.concatenate([r.ravel() for r in ref_dws])
    dx_ops, fg_ops = (a.cpu().numpy() for a in res[False][0])
    for dx, fg in res[True]:
        dx, fg = dx.cpu().numpy(), fg.cpu().numpy()
        assert rel_err(dx, dx_ops) <= 2e-6 and rel_err(fg, fg_ops) <= 2e-6
        assert rel_err(dx, ref_dx) <= STACK_TOL[F32], rel_err(dx, ref_dx)
        o = 0
        for l, r in enumerate(ref_dws):
            assert rel_err(fg[o:o + r.size], r.ravel()) <= STACK_TOL[F32], ("grad_filter", l)
            o += r.size
    assert rel_err(fg_ops, ref_fg) <= STACK_TOL[F32]
