"""The stack-level C entry points (conv3p_stack_prefetch / _forward / _backward of include/conv3p.h) over their
description space (-m gpu): one explicit row per conv3p_stack_desc, driven through ctypes, against the general stack
reference of tests/stack_ref.py.  Conv3pStack only ever builds the two models' descriptions (n_hidden 4, hidden 9,
3 x 3 x 3, strides 1..4); these rows also take fp64, other widths, depths, extents and strides, a head stride of 2 and
grad_concat without a head.

Every supported row: activations, head, grad_input and each layer's grad_filter against the reference (fp32: 2e-5 for
activations, 5e-5 for grad_input and grad_filter, each layer on its own scale; fp64: 1e-11, i.e. tests/parity_util.TOL's
1e-12 per op over at most nine chained ops); the profile shows no generic (global-atomics) kernel on deterministic rows;
fused rows show their launch counts with no error bits.  Deterministic rows give the same bits with the geometry built
inline, on the side stream and by conv3p_stack_prefetch; fused rows give the bits of the per-layer launches (grad_filter:
within 2e-6, its partials are summed in another order).  Rows outside the register-resident list return
CONV3P_ERR_UNSUPPORTED before anything is launched."""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle
from pointwise_amd import _lib, conv3p_op as op, stack, synth
from tests.parity_util import rel_err
from tests.stack_ref import stack_reference

pytestmark = pytest.mark.gpu
VOX = 0.1
F32, F64 = np.float32, np.float64
LAYERS, FUSED, NOFUSE, UNSUP, UNSUP_BWD = "per-layer", "fused", "fusion-refused", "unsupported", "unsupported-backward"
TOL = {F32: (2e-5, 5e-5, 5e-5), F64: (1e-11, 1e-11, 1e-11)}   # activations, grad_input, grad_filter

Row = collections.namedtuple("Row", "name dt cin hidden nh ncls ext strides head_stride outcome fused_bwd kind B N")


def S(*v):
    return [(s, s, s) for s in v]


# grad_concat is given exactly when there is no head (the backward needs an external gradient; with a head it is refused).
# outcome: LAYERS (per-layer launches), FUSED (fused forward; fused_bwd: also the fused backward, which needs every hidden
# layer past the first dilated), NOFUSE (the fused bits are set and must be ignored), UNSUP (the forward refuses),
# UNSUP_BWD (the forward runs, the backward refuses).  Every supported row must stay on deterministic kernels.
ROWS = [
    # the two models' descriptions in fp64
    Row("modelnet-f64", F64, 3, 9, 4, 0, (3, 3, 3), S(1, 2, 3, 4), None, LAYERS, False, "modelnet", 2, 900),
    Row("s3dis-f64", F64, 9, 9, 4, 13, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), LAYERS, False, "room", 2, 900),
    # SceneNN (41 classes, 12 input channels): the 36 -> 41 head is no register shape
    Row("scenenn-f32", F32, 12, 9, 4, 41, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), LAYERS, False, "room", 2, 1200),
    Row("scenenn-f64", F64, 12, 9, 4, 41, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), LAYERS, False, "room", 2, 700),
    # hidden = 3: 3 -> 3 and 9 -> 3 rows, with a 12 -> 9 and a 9 -> 3 head, and without a head
    Row("h3-head12to9", F32, 3, 3, 4, 9, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), LAYERS, False, "modelnet", 2, 800),
    Row("h3-head9to3", F32, 9, 3, 3, 3, (3, 3, 3), S(1, 2, 3), (1, 1, 1), LAYERS, False, "room", 2, 800),
    Row("h3-head9to3-f64", F64, 9, 3, 3, 3, (3, 3, 3), S(1, 2, 3), (1, 1, 1), LAYERS, False, "room", 2, 700),
    Row("h3-nohead", F32, 9, 3, 3, 0, (3, 3, 3), S(2, 1, 3), None, LAYERS, False, "modelnet", 2, 800),
    # depths 1, 2, 3, 5, 8 (5 and 8 repeat strides: layers share cache slots)
    Row("nh1", F32, 3, 9, 1, 0, (3, 3, 3), S(2), None, LAYERS, False, "modelnet", 2, 700),
    Row("nh1-head9to13-f64", F64, 6, 9, 1, 13, (3, 3, 3), S(1), (1, 1, 1), LAYERS, False, "room", 2, 600),
    Row("nh2-fused", F32, 9, 9, 2, 0, (3, 3, 3), S(2, 3), None, FUSED, True, "modelnet", 3, 1000),
    Row("nh3-in6-f64", F64, 6, 9, 3, 0, (3, 3, 3), S(1, 2, 3), None, LAYERS, False, "modelnet", 2, 800),
    Row("nh5-fused", F32, 3, 9, 5, 0, (3, 3, 3), S(1, 2, 3, 4, 2), None, FUSED, True, "modelnet", 3, 1000),
    Row("nh8-fused", F32, 3, 9, 8, 0, (3, 3, 3), S(1, 2, 3, 4, 2, 3, 4, 2), None, FUSED, True, "modelnet", 2, 1000),
    Row("nh8-head72to13-f64", F64, 9, 9, 8, 13, (3, 3, 3), S(1, 2, 3, 4, 1, 2, 3, 4), (1, 1, 1), LAYERS, False, "room", 2, 500),
    # in_channels 6 and 12
    Row("in6-f32", F32, 6, 9, 4, 0, (3, 3, 3), S(1, 2, 3, 4), None, LAYERS, False, "room", 2, 900),
    Row("in12-f32", F32, 12, 9, 4, 0, (3, 3, 3), S(1, 2, 3, 4), None, LAYERS, False, "room", 2, 900),
    Row("in12-28taps-f64", F64, 12, 9, 3, 0, (2, 2, 7), S(1, 2, 3), None, LAYERS, False, "room", 2, 700),
    # extents other than 3 x 3 x 3: fused-eligible (<= 32 taps, odd dilated extents), and an even dilated extent
    Row("ext2x4x4-fused", F32, 3, 9, 4, 0, (2, 4, 4), S(2, 4, 2, 4), None, FUSED, True, "modelnet", 2, 1000),
    Row("ext1x3x9-fused", F32, 9, 9, 3, 0, (1, 3, 9), S(1, 2, 3), None, FUSED, True, "modelnet", 2, 1000),
    Row("ext2x2x2-s3-nofuse", F32, 3, 9, 3, 0, (2, 2, 2), S(3, 3, 1), None, NOFUSE, False, "modelnet", 2, 1000),
    # anisotropic and repeated strides, a head stride of 2
    Row("aniso-head-s2", F32, 9, 9, 4, 13, (3, 3, 3), [(1, 1, 1), (2, 1, 3), (3, 2, 2), (1, 4, 2)], (2, 2, 2), LAYERS, False,
        "room", 2, 900),
    Row("aniso-f64", F64, 3, 9, 4, 0, (3, 3, 3), [(1, 2, 1), (2, 2, 3), (3, 1, 2), (2, 2, 2)], None, LAYERS, False, "modelnet",
        2, 800),
    Row("aniso-repeat-fused", F32, 3, 9, 4, 0, (3, 3, 3), [(1, 1, 1), (2, 3, 2), (2, 3, 2), (4, 2, 3)], None, FUSED, True,
        "modelnet", 2, 1000),
    # outside the register-resident list
    Row("in16", F32, 16, 9, 4, 41, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), UNSUP, False, "room", 2, 500),
    Row("hidden64", F32, 3, 64, 4, 0, (3, 3, 3), S(1, 2, 3, 4), None, UNSUP, False, "modelnet", 2, 500),
    # fp64 9 -> 9 with 32 taps: its forward fits the register kernels, its backward's dense G does not
    Row("f64-2x4x4-bwd", F64, 3, 9, 4, 0, (2, 4, 4), S(1, 2, 3, 4), None, UNSUP_BWD, False, "modelnet", 2, 500),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _layers(row):
    """(Cin, Cout, stride) per layer, the head last."""
    out = [(row.cin if l == 0 else row.hidden, row.hidden, row.strides[l]) for l in range(row.nh)]
    if row.ncls:
        out.append((row.nh * row.hidden, row.ncls, row.head_stride))
    return out


def _desc(row):
    d = _lib.StackDesc()
    d.n_hidden, d.in_channels, d.hidden, d.num_class = row.nh, row.cin, row.hidden, row.ncls
    d.fz, d.fy, d.fx = row.ext
    for l, (_, _, s) in enumerate(_layers(row)):
        for a in range(3):
            d.strides[l][a] = s[a]
    return d


def _case(row):
    seed = 3100 + zlib.crc32(row.name.encode()) % 1000
    B, N = row.B, row.N
    P = synth.modelnet_like(B, N, seed) if row.kind == "modelnet" else synth.room_like(B, N, seed)
    P = P.astype(row.dt)
    X = synth.features(B, N, row.cin, seed + 1, points=P if row.cin >= 3 else None, dtype=row.dt)
    Ws = [synth.filter_weights(*row.ext, ci, co, seed + 2 + l, dtype=row.dt) for l, (ci, co, _) in enumerate(_layers(row))]
    up = synth.upstream_grad(B, N, row.ncls if row.ncls else row.nh * row.hidden, seed + 20, dtype=row.dt)
    return P, X, Ws, up


def _reference(row, case):
    P, X, Ws, up = case
    return stack_reference(P, X, Ws, [s for _, _, s in _layers(row)], row.hidden, grad_head=up if row.ncls else None,
                           grad_concat=None if row.ncls else up, nthreads=2, memo=("stack-descriptor", row.name))


def _read_profile(lib):
    seen = {}
    for k in range(lib.conv3p_profile_kinds()):
        n = ctypes.c_uint64(0)
        lib.conv3p_profile_read(k, ctypes.byref(n), None)
        if n.value:
            seen[lib.conv3p_profile_name(k).decode()] = n.value
    lib.conv3p_profile_reset()
    return seen


class StackRun:
    """One description on one neighbour cache: device tensors, pointer tables and the C calls."""

    def __init__(self, dev, row, case, fused=False, sparse=None):
        self.row, self.lib = row, _lib.load()
        self.sfx, self.real = ("f32", ctypes.c_float) if row.dt == F32 else ("f64", ctypes.c_double)
        tdt = torch.float32 if row.dt == F32 else torch.float64
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        P, X, Ws, up = case
        self.P, self.X, self.up = t(P), t(X), t(up)
        self.W = [t(w) for w in Ws]
        self.desc = _desc(row)
        B, N, CW = row.B, row.N, row.nh * row.hidden
        cmax = max(max(ci, co) for ci, co, _ in _layers(row))
        ntap = row.ext[0] * row.ext[1] * row.ext[2]
        self.cache = op.NeighborCache(B, N, tdt, dev, slots=len(_layers(row)), max_taps=ntap, max_cin=cmax, max_cout=cmax,
                                      sparse_neighbourhoods=sparse, fused_stack=fused)
        self.concat = torch.empty((B, N, CW), dtype=tdt, device=dev)
        self.head = torch.empty((B, N, row.ncls), dtype=tdt, device=dev) if row.ncls else None
        self.dx = torch.empty_like(self.X)
        sizes = [w.numel() for w in self.W]
        self.grad = torch.empty(sum(sizes), dtype=tdt, device=dev)
        self.gviews, o = [], 0
        for w, n in zip(self.W, sizes):
            self.gviews.append(self.grad[o:o + n].view(w.shape))
            o += n
        nl = len(self.W)
        self.fptrs = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in self.W])
        self.gptrs = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in self.gviews])
        self.need = self.lib.conv3p_stack_scratch_bytes(ctypes.byref(self.desc), 8 if row.dt == F64 else 4, B, N)
        self.scratch = torch.empty(self.need + 256, dtype=torch.uint8, device=dev)
        self.side = torch.cuda.Stream(device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.P.device).cuda_stream

    def prefetch(self):
        return getattr(self.lib, "conv3p_stack_prefetch_" + self.sfx)(
            ctypes.byref(self.desc), self.P.data_ptr(), self.real(VOX), self.row.B, self.row.N, self.cache.buf.data_ptr(),
            self.cache.nbytes, self.cache.cfg_ptr(False), self.side.cuda_stream, self._stream())

    def forward(self, side=False):
        return getattr(self.lib, "conv3p_stack_forward_" + self.sfx)(
            ctypes.byref(self.desc), self.P.data_ptr(), self.X.data_ptr(), ctypes.cast(self.fptrs, ctypes.c_void_p),
            self.real(VOX), self.row.B, self.row.N, self.concat.data_ptr(),
            self.head.data_ptr() if self.head is not None else None, self.cache.buf.data_ptr(), self.cache.nbytes,
            self.cache.cfg_ptr(False), self._stream(), self.side.cuda_stream if side else None)

    def backward(self, scratch_bytes=None, grad_concat=None):
        has_head = self.row.ncls > 0
        gconcat = grad_concat if grad_concat is not None else (None if has_head else self.up)
        return getattr(self.lib, "conv3p_stack_backward_" + self.sfx)(
            ctypes.byref(self.desc), self.P.data_ptr(), self.X.data_ptr(), ctypes.cast(self.fptrs, ctypes.c_void_p),
            self.real(VOX), self.row.B, self.row.N, self.concat.data_ptr(),
            self.head.data_ptr() if has_head else None, gconcat.data_ptr() if gconcat is not None else None,
            self.up.data_ptr() if has_head else None, self.dx.data_ptr(), ctypes.cast(self.gptrs, ctypes.c_void_p),
            self.scratch.data_ptr(), self.need if scratch_bytes is None else scratch_bytes, self.cache.buf.data_ptr(),
            self.cache.nbytes, self.cache.cfg_ptr(True), self._stream())

    def acts(self):
        H = self.row.hidden
        out = [self.concat[:, :, H * l:H * (l + 1)].clone() for l in range(self.row.nh)]
        return out + ([self.head.clone()] if self.head is not None else [])

    def results(self):
        return self.acts(), self.dx.clone(), [g.clone() for g in self.gviews]

    def fill(self, value):
        self.dx.fill_(value)
        self.grad.fill_(value)

    def untouched(self, value):
        return bool((self.dx == value).all()) and bool((self.grad == value).all())


def _run(dev, row, case, geometry, fused=False, sparse=None):
    """Forward + backward on a fresh cache with the geometry built `inline`, on the `side` stream, or by `prefetch`;
    returns (results, forward profile, backward profile, fused status)."""
    lib = _lib.load()
    r = StackRun(dev, row, case, fused=fused, sparse=sparse)
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        if geometry == "prefetch":
            assert r.prefetch() == _lib.OK
        rc = r.forward(side=geometry == "side")
        assert rc == _lib.OK, (row.name, "forward", _lib.status_string(rc))
        torch.cuda.synchronize()
        fseen = _read_profile(lib)
        if row.dt == F64:
            # conv3p_stack_scratch_bytes is what the backward accepts: one byte less is refused before any launch
            r.fill(7.0)
            assert r.backward(scratch_bytes=r.need - 1) == _lib.ERR_WORKSPACE
            torch.cuda.synchronize()
            assert r.untouched(7.0) and _read_profile(lib) == {}
        rc = r.backward()
        assert rc == _lib.OK, (row.name, "backward", _lib.status_string(rc))
        torch.cuda.synchronize()
        bseen = _read_profile(lib)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    f, b, e = r.cache.fused_status()
    return r.results(), fseen, bseen, (f, b, e)


def _same_bits(a, b, what, grad_filter=True):
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        assert torch.equal(u, v), (what, "activation", i)
    assert torch.equal(a[1], b[1]), (what, "grad_input")
    if grad_filter:
        for i, (u, v) in enumerate(zip(a[2], b[2])):
            assert torch.equal(u, v), (what, "grad_filter", i)


@pytest.mark.parametrize("row", [r for r in ROWS if r.outcome not in (UNSUP, UNSUP_BWD)], ids=lambda r: r.name)
def test_stack_description(dev, row):
    case = _case(row)
    fused = row.outcome in (FUSED, NOFUSE)
    sparse = True if fused else None      # (the fused backward needs the SPARSE hint; the per-layer run then takes it too)
    runs = {g: _run(dev, row, case, g, fused=fused, sparse=sparse) for g in ("inline", "side", "prefetch")}

    for g, (_, fseen, bseen, (f, b, e)) in runs.items():
        assert "generic_forward_kernel" not in fseen and "generic_backward_kernel" not in bseen, (g, fseen, bseen)
        assert e == 0, (g, "fused launch error bits", e)
        want = (1, 1 if row.fused_bwd else 0) if row.outcome == FUSED else (0, 0)
        assert (f, b) == want, (g, "fused launches", (f, b), "expected", want)

    acts, dx, dws = (x for x in runs["inline"][0])
    ref_acts, ref_dx, ref_dws = _reference(row, case)
    tol_a, tol_x, tol_w = TOL[row.dt]
    for l, (a, r) in enumerate(zip(acts, ref_acts)):
        assert rel_err(a.cpu().numpy(), r) <= tol_a, ("activation", l, rel_err(a.cpu().numpy(), r))
    assert rel_err(dx.cpu().numpy(), ref_dx) <= tol_x, ("grad_input", rel_err(dx.cpu().numpy(), ref_dx))
    for l, (w, r) in enumerate(zip(dws, ref_dws)):           # per layer: each has its own scale
        assert rel_err(w.cpu().numpy(), r) <= tol_w, ("grad_filter", l, rel_err(w.cpu().numpy(), r))

    # geometry built inline, on the side stream or by the prefetch: the same lists, hence the same bits
    _same_bits(runs["inline"][0], runs["side"][0], "side-stream geometry")
    _same_bits(runs["inline"][0], runs["prefetch"][0], "prefetched geometry")
    if row.outcome == FUSED:
        per_layer = _run(dev, row, case, "inline", fused=False, sparse=sparse)
        assert per_layer[3][:2] == (0, 0)
        _same_bits(runs["inline"][0], per_layer[0], "fused against per-layer launches", grad_filter=False)
        for l, (u, v) in enumerate(zip(runs["inline"][0][2], per_layer[0][2])):
            assert rel_err(u.cpu().numpy(), v.cpu().numpy()) <= 2e-6, ("grad_filter", l)


@pytest.mark.parametrize("row", [r for r in ROWS if r.outcome == UNSUP], ids=lambda r: r.name)
def test_stack_outside_the_register_list_is_refused(dev, row):
    """The forward returns CONV3P_ERR_UNSUPPORTED (Conv3pStack then composes the op calls) and launches nothing."""
    lib = _lib.load()
    r = StackRun(dev, row, _case(row))
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        assert r.forward() == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _read_profile(lib) == {}
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()


@pytest.mark.parametrize("row", [r for r in ROWS if r.outcome == UNSUP_BWD], ids=lambda r: r.name)
def test_stack_backward_it_cannot_serve_is_refused_before_any_launch(dev, row):
    """A description whose forward runs but whose backward does not fit the register kernels: the backward returns
    CONV3P_ERR_UNSUPPORTED with grad_input and every grad_filter untouched and nothing launched; the forward is right."""
    lib = _lib.load()
    case = _case(row)
    r = StackRun(dev, row, case)
    assert r.forward() == _lib.OK
    r.fill(-3.0)
    torch.cuda.synchronize()
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        assert r.backward() == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _read_profile(lib) == {}
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    assert r.untouched(-3.0)
    P, X, Ws, _ = case
    x = X
    for l, (a, (_, _, s)) in enumerate(zip(r.acts(), _layers(row))):
        x = stack.selu_numpy(oracle.forward(P, x, Ws[l], s, VOX, nthreads=2))
        assert rel_err(a.cpu().numpy(), x) <= TOL[row.dt][0], ("activation", l)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_stack_backward_with_head_and_grad_concat_is_refused_before_any_launch(dev, dt):
    row = Row("s3dis", dt, 9, 9, 4, 13, (3, 3, 3), S(1, 2, 3, 4), (1, 1, 1), LAYERS, False, "room", 2, 500)
    lib = _lib.load()
    r = StackRun(dev, row, _case(row))
    assert r.forward() == _lib.OK
    r.fill(5.0)
    gconcat = torch.zeros_like(r.concat)
    torch.cuda.synchronize()
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        assert r.backward(grad_concat=gconcat) == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _read_profile(lib) == {}
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    assert r.untouched(5.0)


# ------------------------------------------------------------------ the models through Conv3pStack
@pytest.mark.parametrize("cin,ncls,dt,B,N", [(3, None, F64, 2, 1024), (9, 13, F64, 2, 1024), (12, 41, F32, 2, 8192)],
                         ids=["modelnet-f64", "s3dis-f64", "scenenn-f32"])
def test_model_stack_on_the_stack_entry_points(dev, cin, ncls, dt, B, N):
    """The models' stacks as bench.py drives them (tune(), the next batch prefetched while another is between its forward
    and its backward) in fp64 and at SceneNN size: the stack entry points serve them, on deterministic kernels only."""
    tdt = torch.float32 if dt == F32 else torch.float64
    seed = 3500 + cin + (ncls or 0)
    P = (synth.modelnet_like(B, N, seed) if ncls is None else synth.room_like(B, N, seed)).astype(dt)
    X = synth.features(B, N, cin, seed + 1, points=P, dtype=dt)
    ups = [synth.upstream_grad(B, N, stack.HIDDEN, seed + 2 + i, dtype=dt) for i in range(4)] if ncls is None else \
        [synth.upstream_grad(B, N, ncls, seed + 2, dtype=dt)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tx = t(P), t(X)
    st = stack.Conv3pStack(cin, ncls, device=dev, dtype=tdt, seed=41)
    st.tune(tp)
    other = t((synth.modelnet_like(B, N, seed + 9) if ncls is None else synth.room_like(B, N, seed + 9)).astype(dt))
    st.forward(other, t(synth.features(B, N, cin, seed + 10, points=P, dtype=dt)))
    st.prefetch(tp)
    st.backward([t(u) for u in ups])
    lib = _lib.load()
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        acts = st.forward(tp, tx)
        dx, fused = st.backward([t(u) for u in ups])
        torch.cuda.synchronize()
        seen = _read_profile(lib)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    assert st.c_stack, "the stack entry points must serve the model"
    assert "generic_forward_kernel" not in seen and "generic_backward_kernel" not in seen, seen
    strides = [(s, s, s) for _, _, s in st.layers]
    filters = [f.cpu().numpy() for f in st.filters]
    ref_acts, ref_dx, ref_dws = stack_reference(P, X, filters, strides, stack.HIDDEN,
                                                grad_head=ups[0] if ncls else None,
                                                grad_concat=None if ncls else np.concatenate(ups, axis=2), nthreads=8,
                                                memo=("model", cin, ncls, np.dtype(dt).name, B, N))
    tol_a, tol_x, tol_w = TOL[dt]
    for l, (a, r) in enumerate(zip(acts, ref_acts)):
        assert rel_err(a.cpu().numpy(), r) <= tol_a, ("activation", l, rel_err(a.cpu().numpy(), r))
    assert rel_err(dx.cpu().numpy(), ref_dx) <= tol_x, ("grad_input", rel_err(dx.cpu().numpy(), ref_dx))
    for l, (g, r) in enumerate(zip(st.grad_views, ref_dws)):
        assert rel_err(g.cpu().numpy(), r) <= tol_w, ("grad_filter", l, rel_err(g.cpu().numpy(), r))


def test_model_stack_outside_the_register_list_composes_the_op_calls(dev):
    """Conv3pStack(16, 41): the stack entry points refuse 16 -> 9, the stack falls back to the op-by-op composition for
    good, and that composition is the reference's stack."""
    B, N, cin, ncls = 2, 1024, 16, 41
    P = synth.room_like(B, N, 3600)
    X = synth.features(B, N, cin, 3601, points=P)
    up = synth.upstream_grad(B, N, ncls, 3602)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = stack.Conv3pStack(cin, ncls, device=dev, seed=43)
    acts = st.forward(t(P), t(X))
    assert not st.c_stack
    dx, _ = st.backward([t(up)])
    ref_acts, ref_dx, ref_dws = stack_reference(P, X, [f.cpu().numpy() for f in st.filters],
                                                [(s, s, s) for _, _, s in st.layers], stack.HIDDEN, grad_head=up,
                                                nthreads=2)
    tol_a, tol_x, tol_w = TOL[F32]
    for l, (a, r) in enumerate(zip(acts, ref_acts)):
        assert rel_err(a.cpu().numpy(), r) <= tol_a, ("activation", l)
    assert rel_err(dx.cpu().numpy(), ref_dx) <= tol_x
    for l, (g, r) in enumerate(zip(st.grad_views, ref_dws)):
        assert rel_err(g.cpu().numpy(), r) <= tol_w, ("grad_filter", l)
