"""Conv3pStack over seeded call schedules (-m gpu): prefetches early, late, mixed, superseded and never consumed, forwards
without a backward, changes of (B, N) with a prefetch outstanding, tune() and prepare() mid-run, batch tensors rewritten in
place or dropped by the caller -- the schedules of tests/stack_schedule.py, whose legality and coverage
tests/test_stack_schedules_host.py asserts on the CPU.  None is filtered or skipped here.

Every forward's activations and every backward's grad_input and fused weight-gradient buffer are cloned as the schedule
runs and compared after ONE synchronise at its end (no per-step sync: the side stream really overlaps; tune() is the one
operation that synchronises by itself) with what a Conv3pStack(use_cache=False) of the same seed gives for that step's
points content, features and upstream gradient.  That stateless stack is itself checked against tests/stack_ref.py once
per pool batch (fp32: 2e-5 activations, 5e-5 gradients, as tests/test_stack_descriptors.py).

The comparison is the one the suite already makes for each route:
  * the stack entry points and the op-by-op composition, with or without the SELU fused into the op (c_stack=False,
    fuse_selu=False, a stack that fell back): torch.equal, as test_stack_with_cache_hints_over_changing_batches -- every
    one of these routes gives the stateless stack's bits on these clouds;
  * the fused forward launch: torch.equal on activations and grad_input, 2e-6 on the weight gradients, as
    test_fused_stack_launch_equals_the_per_layer_launches."""
import numpy as np
import pytest
import torch

from pointwise_amd import _lib, stack, synth
from tests import stack_schedule as S
from tests.parity_util import rel_err
from tests.stack_ref import stack_reference

pytestmark = pytest.mark.gpu
STACK_SEED = 29
SMALL = ((3, 320), (2, 512))        # the sizes of the existing stack tests: several tiles per cloud, a real stride-4 layer
FUSABLE = ((11, 700), (3, 320))     # (11, 700): the smallest size known to take the fused forward launch
EXACT = (0.0, 0.0, 0.0)             # activations, grad_input, fused weight gradient: 0 = torch.equal
FUSED_LAUNCH = (0.0, 0.0, 2e-6)     # test_fused_stack_launch_equals_the_per_layer_launches

# mode -> (in_channels, num_class, cloud kind, shapes, Conv3pStack keywords, batched_prefetch, tune() first, bounds)
MODES = {
    "cls": (3, None, "modelnet", SMALL, {}, False, False, EXACT),
    "seg": (9, 13, "room", SMALL, {}, False, False, EXACT),
    "op-by-op": (3, None, "modelnet", SMALL, {"c_stack": False}, False, False, EXACT),
    "op-by-op-batched-prefetch": (3, None, "modelnet", SMALL, {"c_stack": False}, True, False, EXACT),
    "unfused-selu": (3, None, "modelnet", SMALL, {"fuse_selu": False}, False, False, EXACT),
    "fused-forward": (3, None, "modelnet", FUSABLE, {"fused_launch": "forward"}, False, True, FUSED_LAUNCH),
    # 16 input channels are outside the register-resident list: the first forward (or prefetch) hands over from the stack
    # entry points' bookkeeping to the op-by-op composition, with whatever was prefetched until then
    "fallback-in16": (16, None, "modelnet", SMALL, {}, False, False, EXACT),
}
assert set(MODES) == set(S.MODE_LENGTHS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


class Pool:
    """Five batches over two shapes, their features, two upstream gradients per shape, and the stateless stack's results
    per (content, upstream), computed once."""

    def __init__(self, dev, cin, ncls, kind, shapes):
        self.dev, self.cin, self.ncls, self.shapes = dev, cin, ncls, shapes
        self.P, self.X = [], []
        for j, s in enumerate(S.POOL_SHAPES):
            B, N = shapes[s]
            seed = 7100 + 10 * j + cin
            self.P.append(synth.modelnet_like(B, N, seed) if kind == "modelnet" else synth.room_like(B, N, seed))
            self.X.append(synth.features(B, N, cin, seed + 1, points=self.P[j]))
        self.up = []                      # up[shape][k]: the arrays of one upstream gradient
        for s, (B, N) in enumerate(shapes):
            self.up.append([[synth.upstream_grad(B, N, ncls, 7300 + 10 * s + k)] if ncls else
                            [synth.upstream_grad(B, N, stack.HIDDEN, 7300 + 10 * s + 4 * k + i) for i in range(4)]
                            for k in range(S.N_UPSTREAM)])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.tP = [t(p) for p in self.P]  # masters: never handed to a stack under test, never written
        self.tX = [t(x) for x in self.X]
        self.tup = [[[t(u) for u in us] for us in ks] for ks in self.up]
        self.plain = stack.Conv3pStack(cin, ncls, device=dev, seed=STACK_SEED, use_cache=False)
        self._expected = {}

    def expected(self, j):
        """(activations, [(grad_input, fused weight gradient) per upstream]) of the stateless stack on content j."""
        if j not in self._expected:
            acts = [a.clone() for a in self.plain.forward(self.tP[j], self.tX[j])]
            grads = []
            for k in range(S.N_UPSTREAM):
                dx, fg = self.plain.backward(self.tup[S.POOL_SHAPES[j]][k])
                grads.append((dx.clone(), fg.clone()))
            self._expected[j] = (acts, grads)
        return self._expected[j]


_POOLS = {}


def _pool(dev, mode):
    cin, ncls, kind, shapes = MODES[mode][:4]
    key = (cin, ncls, kind, shapes)
    if key not in _POOLS:
        _POOLS[key] = Pool(dev, cin, ncls, kind, shapes)
    return _POOLS[key]


def _stack(dev, mode):
    cin, ncls, _, _, kw, batched, _, _ = MODES[mode]
    st = stack.Conv3pStack(cin, ncls, device=dev, seed=STACK_SEED, **kw)
    st.batched_prefetch = batched
    return st


def run_schedule(st, pool, sched, tune_first=False):
    """Execute `sched` on `st`; returns the log of (kind, content, upstream, cloned results), synchronised once."""
    n = len(S.POOL_SHAPES)
    tensors = [p.clone() for p in pool.tP]
    content = list(range(n))

    def tensor(i):
        if tensors[i] is None:            # dropped earlier: a new object with the content the old one had
            tensors[i] = pool.tP[content[i]].clone()
        return tensors[i]

    if tune_first:
        st.tune(tensor(0))
    log, last = [], None
    for op in sched:
        kind = op[0]
        if kind == "forward":
            last = content[op[1]]
            acts = st.forward(tensor(op[1]), pool.tX[last])
            log.append(("forward", last, None, [a.clone() for a in acts]))
        elif kind == "backward":
            dx, fg = st.backward(pool.tup[S.POOL_SHAPES[last]][op[1]])
            log.append(("backward", last, op[1], [dx.clone(), fg.clone()]))
        elif kind == "prefetch":
            st.prefetch(tensor(op[1]))
        elif kind == "tune":
            st.tune(tensor(op[1]))
        elif kind == "prepare":
            st.prepare(*pool.shapes[op[1]])
        elif kind == "rewrite":
            tensor(op[1]).copy_(pool.tP[op[2]])
            content[op[1]] = op[2]
        elif kind == "drop":
            tensors[op[1]] = None
        else:
            raise AssertionError(op)
    torch.cuda.synchronize()
    return log


def compare(log, pool):
    """(step, what, identical, rel_err) of every logged tensor against the stateless stack's."""
    out = []
    for n, (kind, j, k, got) in enumerate(log):
        acts, grads = pool.expected(j)
        if kind == "forward":
            want = [("activation %d" % l, a) for l, a in enumerate(acts)]
        else:
            want = [("grad_input", grads[k][0]), ("fused_grad", grads[k][1])]
        for g, (what, w) in zip(got, want):
            out.append((n, kind, what, torch.equal(g, w), rel_err(g.cpu().numpy(), w.cpu().numpy())))
    return out


def check(log, pool, bounds, where):
    tol_a, tol_x, tol_w = bounds
    for n, kind, what, same, err in compare(log, pool):
        tol = tol_w if what == "fused_grad" else tol_x if what == "grad_input" else tol_a
        if tol == 0.0:
            assert same, (where, "step", n, kind, what, "differs from the stateless stack, rel_err", err)
        else:
            assert err <= tol, (where, "step", n, kind, what, err)


def _run_mode(dev, mode, sched, where):
    tune_first, bounds = MODES[mode][6], MODES[mode][7]
    pool = _pool(dev, mode)
    st = _stack(dev, mode)
    if mode == "fused-forward":
        # (the counters live in the caches, and a change of shape replaces a cache: one more forward of the fusable shape,
        # so that the launch count read below is never that of two freshly allocated caches)
        sched = list(sched) + [("forward", 0)]
    log = run_schedule(st, pool, sched, tune_first)
    check(log, pool, bounds, where)
    if mode == "fused-forward":
        f, b, e = st.fused_status()
        assert f > 0 and e == 0, (where, "fused launches", (f, b), "error bits", e)
    if mode == "fallback-in16":
        assert not st.c_stack, "16 input channels must fall back to the op-by-op composition"
    return st


@pytest.mark.parametrize("mode", sorted(MODES))
def test_stack_over_seeded_schedules(dev, mode):
    for seed in S.SEEDS:
        sched, _ = S.generate(seed, S.MODE_LENGTHS[mode])
        _run_mode(dev, mode, sched, (mode, "seed", seed))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(S.NAMED))
def test_named_schedule(dev, name, mode):
    """The hand-written regression schedules of tests/stack_schedule.py, in every mode.  (The first two are races between
    the side stream's searches and the backward of the batch in flight; repeated, so that one lucky interleaving is not a
    pass.)"""
    for rep in range(4):
        _run_mode(dev, mode, S.NAMED[name], (mode, name, rep))


@pytest.mark.parametrize("mode", ["cls", "seg", "fused-forward", "fallback-in16"])
def test_stateless_stack_of_the_pool_matches_the_oracle_stack(dev, mode):
    """What the schedules are compared with, against the CPU oracle, once per pool batch."""
    pool = _pool(dev, mode)
    st = pool.plain
    filters = [f.cpu().numpy() for f in st.filters]
    strides = [(s, s, s) for _, _, s in st.layers]
    for j in range(len(S.POOL_SHAPES)):
        acts, grads = pool.expected(j)
        up = pool.up[S.POOL_SHAPES[j]][0]
        ref_acts, ref_dx, ref_dws = stack_reference(pool.P[j], pool.X[j], filters, strides, stack.HIDDEN,
                                                    grad_head=up[0] if pool.ncls else None,
                                                    grad_concat=None if pool.ncls else np.concatenate(up, axis=2), nthreads=4)
        for l, (a, r) in enumerate(zip(acts, ref_acts)):
            assert rel_err(a.cpu().numpy(), r) <= 2e-5, (j, "activation", l, rel_err(a.cpu().numpy(), r))
        dx, fg = grads[0]
        assert rel_err(dx.cpu().numpy(), ref_dx) <= 5e-5, (j, "grad_input", rel_err(dx.cpu().numpy(), ref_dx))
        got, o = fg.cpu().numpy(), 0
        for l, r in enumerate(ref_dws):          # per layer: each has its own scale
            assert rel_err(got[o:o + r.size], r.reshape(-1)) <= 5e-5, (j, "grad_filter", l)
            o += r.size
