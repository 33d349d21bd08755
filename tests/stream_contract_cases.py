"""The case table of the stream contract: every public entry point of pointwise_amd, in each dtype it has and in each
argument form that changes what the host does, as a case of tests/stream_rig.py.

    python -m tests.stream_contract_cases      prints, per case, the host enqueue time, the delay used and the two
                                               verdicts (profiles/stream_contract.txt is that output)

tests/test_stream_contract.py (-m gpu) judges every entry and checks that it entered exactly the C functions it claims;
tests/test_stream_contract_host.py (CPU) checks that the table covers every streamed function of include/conv3p.h and
every public name of the package.  Importing this module does not touch the device.

An entry is Entry(name, halves, build, reaches):
  halves()                 -> (real, poison): two lists of numpy arrays from two seeds of one generator -- the inputs the
                              host makes.  The CPU suite checks that they agree in shape and dtype;
  build(dev, real, poison) -> a stream_rig.Case from those arrays uploaded to `dev`.  Inputs that only the device can
                              make (a GridSubsample's tensors, a segmentation) are made here, from both halves alike, and
                              join the case's inputs with their poison; the rig checks their shapes as well;
  reaches                  -> the streamed C entry points the case's run() enters.

Sizes are the smallest the project's own tests use: B = 2 clouds of N = 130 points and the EXT filters of the launch census,
a room of 3000 rows for scene and grid, (7, 1000, 24) for FC, (33, 1024, 13) for the classification tail, three small
tensors at mixed offsets of one buffer for the optimizer.  Only deterministic routes are taken, because the rig compares
bits: every family of launch_census_cases.LAYERS but the two generic-* ones (float atomics; they enter through the same C
functions), and the fused-launch flags stay off as in the launch census (whether a fused launch is taken depends on the
device census).  Objects whose accessors read the device by design -- num_voxels(), trim(), num_segments(),
overflowed(), summary(), last_grad_norm(), room(r) -- are used in build() only.
"""
import collections
import ctypes
import math
import os
import re

import numpy as np
import torch

from pointwise_amd import synth
from tests.launch_census_cases import B, F32, F64, HINTS, LAYERS, N, STRIDES, VOX
from tests.parity_util import make_case
from tests.stream_rig import Case
from tests.test_dispatch_map import EXT

Entry = collections.namedtuple("Entry", "name halves build reaches")
ENTRIES = []
ROOM_ROWS, NCLS = 3000, 13
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conv3p.h")

# Calls that may block the host because their interface takes host data or returns a host value, with the docstring
# sentence that says so.  They still run through the rig and must be ordered; only `asynchronous` is waived.
HOST_BY_CONTRACT = {
    "Conv3pStack.tune": "returns a host bool measured on the device -- \"Optional set-up, once per dataset (it synchronises)\"",
    "BatchProvider.next_epoch+get_batch_point_cloud":
        "the epoch's permutation is drawn by numpy on the host -- \"np.random.default_rng([seed, epoch]).permutation(S), "
        "uploaded once per epoch\"",
}
# C entry points with a stream parameter that no case reaches.
NOT_STREAMED = {}
# Names of pointwise_amd.__all__ without a case of their own, and why.
NO_CASE = {
    "Conv3pInvalidArgument": "an exception", "Conv3pRuntimeError": "an exception",
    "default_max_blocks": "host arithmetic on shapes", "default_max_blocks_rooms": "host arithmetic on shapes",
    "exponential_decay": "host arithmetic", "class_weights_from_counts": "host arithmetic on host counts",
    "Conv3pFunction": "the autograd Function behind conv3p_autograd, which has cases",
    "SceneBlocks": "the output class of scene_blocks, which has cases; its accessors read the device by design",
    "SceneRoomBlocks": "the output class of scene_blocks_rooms, which has cases",
    "GridRoomSubsample": "the output class of grid_subsample_rooms, which has cases; its methods are GridSubsample's",
    "BatchBuffers": "the output buffers of assemble_batch, which has cases",
    "SegmentPool": "the output class of GridSegments.pool, which has cases",
    "SegmentGeometry": "the output class of GridSegments.geometry, which has cases",
    "GridNormals": "the output class of GridSubsample.normals, which has cases",
}


def streamed_functions(header=HEADER):
    """Every function include/conv3p.h declares with a `void *stream` or `void *side_stream` parameter."""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    found = set()
    for name, params in re.findall(r"\b(conv3p_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"void\s*\*\s*(side_)?stream\b", params):
            found.add(name)
    return found


def entry(name, halves, reaches):
    def deco(build):
        assert name not in [e.name for e in ENTRIES], name
        ENTRIES.append(Entry(name, halves, build, frozenset("conv3p_" + r for r in reaches)))
        return build
    return deco


def upload(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def two(make, seed):
    """halves() from one generator at two seeds."""
    return lambda: (list(make(seed)), list(make(seed + 5000)))


def tensors(obj, names):
    return [getattr(obj, n) for n in names if getattr(obj, n, None) is not None]


def _tdt(dt):
    return torch.float32 if dt == F32 else torch.float64


def _sfx(dt):
    return "f32" if dt == F32 else "f64"


def _cache_reset(*caches):
    """A neighbour cache made a valid empty one again (conv3p_cache_init: the host bookkeeping dropped, the buffer
    zero-filled on the current stream), so that every run searches anew."""
    from pointwise_amd import _lib

    def reset():
        for c in caches:
            if c is not None:
                c.forget_points()
                assert _lib.load().conv3p_cache_init(c.buf.data_ptr(), c.nbytes,
                                                     torch.cuda.current_stream(c.buf.device).cuda_stream) == _lib.OK
    return reset


# ================================================================================================ the conv3p op
def _layer_halves(layer, seed):
    return two(lambda s: make_case("modelnet", B, N, layer.cin, layer.cout, EXT[layer.taps], seed=s, dtype=layer.dt), seed)


def _add_layer(layer, s, route, hint, matmul, seed):
    sfx = _sfx(layer.dt)
    cached = route != "stateless"
    name = "conv3p+conv3p_grad/%s/s%d/%s" % (layer.name, s[0], route if not cached else "cache-%s-%s" % (hint, matmul))
    names = ("forward_cached_", "backward_cached_") if cached else ("forward_", "backward_")

    @entry(name, _layer_halves(layer, seed), [n + sfx for n in names])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        tp, tx, tw, tdy = inputs = upload(dev, real)
        cache = None
        if cached:
            cache = op.NeighborCache(B, N, _tdt(layer.dt), dev, slots=1, max_taps=layer.taps, max_cin=layer.cin,
                                     max_cout=layer.cout, sparse_neighbourhoods=HINTS[hint], matmul_precision=matmul)
            assert cache.fits(B, N, _tdt(layer.dt), dev, layer.taps, layer.cin, layer.cout)

        def run():
            y = op.conv3p(tp, tx, tw, s, VOX, cache=cache)
            dx, dw = op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache)
            return [y, dx, dw]
        return Case(inputs, upload(dev, poison), run, _cache_reset(cache))


for _i, _layer in enumerate(LAYERS):
    if _layer.name.startswith("generic-"):
        continue
    for _s in STRIDES:
        _add_layer(_layer, _s, "stateless", None, None, 6100 + 11 * _i)
        for _hint in _layer.hints:
            for _matmul in _layer.matmul:
                _add_layer(_layer, _s, "cache", _hint, _matmul, 6100 + 11 * _i)


def _add_prepare(dt, kind):
    sfx = _sfx(dt)
    cin, cout = (32, 64) if kind == "deep_orders" else (9, 9)
    reaches = {"single": ["cache_prepare_", "forward_cached_"], "multi": ["cache_prepare_multi_", "forward_cached_"],
               "deep_orders": ["cache_prepare_", "forward_cached_", "backward_cached_"]}[kind]

    @entry("cache_prepare%s/%s" % ({"single": "", "multi": "_multi", "deep_orders": "/deep_orders"}[kind], sfx),
           two(lambda s: make_case("modelnet", B, N, cin, cout, EXT[27], seed=s, dtype=dt), 6500), [r + sfx for r in reaches])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        tp, tx, tw, tdy = inputs = upload(dev, real)
        cache = op.NeighborCache(B, N, _tdt(dt), dev, slots=2, max_taps=27, max_cin=cin, max_cout=cout)
        s1, s2 = STRIDES

        def run():
            # the op calls trust the prepared geometry (points_unchanged): a prepare that strayed from the stream shows
            if kind == "multi":
                op.cache_prepare_multi(tp, EXT[27], [s1, s2], VOX, cache)
                return [op.conv3p(tp, tx, tw, s, VOX, cache=cache, points_unchanged=True) for s in (s2, s1)]
            op.cache_prepare(tp, EXT[27], s2, VOX, cache, deep_orders=kind == "deep_orders")
            out = [op.conv3p(tp, tx, tw, s2, VOX, cache=cache, points_unchanged=True)]
            if kind == "deep_orders":
                out += list(op.conv3p_grad(tdy, tp, tx, tw, s2, VOX, cache=cache, points_unchanged=True))
            return out
        return Case(inputs, upload(dev, poison), run, _cache_reset(cache))


for _dt in (F32, F64):
    _add_prepare(_dt, "single")
    _add_prepare(_dt, "multi")
_add_prepare(F32, "deep_orders")


def _add_cache_init():
    @entry("cache_init(C)/f32", two(lambda s: make_case("modelnet", B, N, 9, 9, EXT[27], seed=s), 6550),
           ["cache_init", "forward_cached_f32"])
    def build(dev, real, poison):
        from pointwise_amd import _lib, conv3p_op as op
        tp, tx, tw, tdy = inputs = upload(dev, real)
        cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=9, max_cout=9)

        def run():
            # no Python path calls conv3p_cache_init (the TensorFlow shim does): through ctypes, then a forward on it
            assert _lib.load().conv3p_cache_init(cache.buf.data_ptr(), cache.nbytes,
                                                 torch.cuda.current_stream(dev).cuda_stream) == _lib.OK
            return [op.conv3p(tp, tx, tw, STRIDES[0], VOX, cache=cache)]
        return Case(inputs, upload(dev, poison), run)


_add_cache_init()


def _add_neighbor_count(dt, s):
    @entry("neighbor_count/%s/s%d" % (_sfx(dt), s[0]), two(lambda sd: [synth.modelnet_like(B, N, sd).astype(dt)], 6600),
           ["neighbor_count_" + _sfx(dt)])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        inputs = upload(dev, real)
        return Case(inputs, upload(dev, poison), lambda: [op.neighbor_count(inputs[0], EXT[27], s, VOX)])


def _add_layer_pair(dt, addend):
    sfx = _sfx(dt)

    def make(seed):
        P, X, W, dY = make_case("modelnet", B, N, 9, 9, EXT[27], seed=seed, dtype=dt)
        return [P, X, W, dY, synth.upstream_grad(B, N, 9, seed + 7, dtype=dt)]

    @entry("conv3p_layer+conv3p_layer_grad/%s/%s" % (sfx, "grad_addend" if addend else "no-addend"), two(make, 6700),
           ["layer_forward_cached_" + sfx, "layer_backward_cached_" + sfx])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        tp, tx, tw, tdy, tadd = inputs = upload(dev, real)
        cache = op.NeighborCache(B, N, _tdt(dt), dev, slots=1, max_taps=27, max_cin=9, max_cout=9)
        s = STRIDES[1]

        def run():
            y = op.conv3p_layer(tp, tx, tw, s, VOX, cache)
            dx, dw = op.conv3p_layer_grad(tdy, tp, tx, tw, s, VOX, cache, grad_addend=tadd if addend else None)
            return [y, dx, dw]
        return Case(inputs, upload(dev, poison), run, _cache_reset(cache))


def _add_selu(dt, which):
    sfx = _sfx(dt)
    reach = {"selu": "selu_", "selu_grad": "selu_grad_", "selu_grad/dy_b": "selu_grad_add_"}[which]

    @entry("%s/%s" % (which, sfx), two(lambda s: [synth.upstream_grad(B, N, 9, s + i, dtype=dt) for i in range(3)], 6800),
           [reach + sfx])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        y, dy, dyb = inputs = upload(dev, real)
        run = {"selu": lambda: [op.selu(y)], "selu_grad": lambda: [op.selu_grad(y, dy)],
               "selu_grad/dy_b": lambda: [op.selu_grad(y, dy, dyb)]}[which]
        return Case(inputs, upload(dev, poison), run)


def _add_autograd(dt):
    sfx = _sfx(dt)

    @entry("conv3p_autograd/forward+backward/" + sfx, two(lambda s: make_case("modelnet", B, N, 9, 9, EXT[27], seed=s, dtype=dt), 6900),
           ["forward_" + sfx, "backward_" + sfx])
    def build(dev, real, poison):
        from pointwise_amd import conv3p_op as op
        tp, tx, tw, tdy = inputs = upload(dev, real)

        def run():
            x, w = tx.detach().requires_grad_(), tw.detach().requires_grad_()     # leaves over the inputs' storage
            y = op.conv3p_autograd(tp, x, w, STRIDES[0], VOX)
            y.backward(tdy)
            return [y.detach(), x.grad, w.grad]
        return Case(inputs, upload(dev, poison), run)


for _dt in (F32, F64):
    for _s in STRIDES:
        _add_neighbor_count(_dt, _s)
    _add_layer_pair(_dt, False)
    _add_layer_pair(_dt, True)
    for _which in ("selu", "selu_grad", "selu_grad/dy_b"):
        _add_selu(_dt, _which)
    _add_autograd(_dt)


# ================================================================================================ Conv3pStack
def _add_stack(dt, num_class, geometry, c_stack=True, tune=False):
    sfx = _sfx(dt)
    cout = num_class if num_class else 36

    def make(seed):
        P = synth.modelnet_like(B, N, seed).astype(dt)
        return [P, synth.features(B, N, 3, seed + 1, points=P, dtype=dt), synth.upstream_grad(B, N, cout, seed + 2, dtype=dt)]

    if tune:
        name, reaches = "Conv3pStack.tune", ["neighbor_count_f32", "stack_forward_f32"]
    elif c_stack:
        name = "Conv3pStack/%s/%s/%s" % ("head%d" % num_class if num_class else "nohead", sfx,
                                        "prepare+forward+backward" if geometry == "inline" else "prefetch+forward+backward")
        reaches = ["stack_forward_" + sfx, "stack_backward_" + sfx] + (["stack_prefetch_" + sfx] if geometry == "prefetch" else [])
    else:
        name = "Conv3pStack/op-by-op/%s/%s" % (sfx, "forward+backward" if geometry == "inline" else "prefetch+forward+backward")
        reaches = [r + sfx for r in ("cache_prepare_", "layer_forward_cached_", "layer_backward_cached_", "backward_cached_",
                                     "selu_grad_")]

    @entry(name, two(make, 7000), reaches)
    def build(dev, real, poison):
        from pointwise_amd import stack
        tp, tx, tup = inputs = upload(dev, real)
        st = stack.Conv3pStack(3, num_class, dev, _tdt(dt), c_stack=c_stack, fused_launch=False)
        st.prepare(B, N)
        weights = [(f, f.clone()) for f in st.filters]
        poison_w = [torch.from_numpy(synth.filter_weights(3, 3, 3, ci, co, 7100 + i, dtype=dt)).to(dev)
                    for i, (ci, co, _) in enumerate(st.layers)]

        def reset():
            st._pending.clear()
            st._inflight = None
            st._saved = None
            st.fused_grad.zero_()
            if tune:
                st.sparse_neighbourhoods = None
                for c in st._caches:
                    c.sparse_neighbourhoods = None
            _cache_reset(*st._caches)()

        def run():
            out = []
            st.prepare(B, N)
            if tune:
                st.tune(tp)
            if geometry == "prefetch":
                st.prefetch(tp)
            acts = st.forward(tp, tx)
            if not tune:
                dx, grads = st.backward([tup] if num_class else tup)
                out = [dx, grads]
            assert st.c_stack == c_stack
            return list(acts) + out
        return Case(inputs + [f for f, _ in weights], upload(dev, poison) + poison_w, run, reset)


for _dt in (F32, F64):
    for _geometry in ("inline", "prefetch"):
        _add_stack(_dt, None, _geometry)
for _geometry in ("inline", "prefetch"):
    _add_stack(F32, NCLS, _geometry)
    _add_stack(F32, None, _geometry, c_stack=False)
_add_stack(F32, None, "inline", tune=True)


# ================================================================================================ the dense head
FC_M, FC_K, FC_N = 7, 1000, 24
TAIL_M, TAIL_H, TAIL_C = 33, 1024, 13


def _fc_arrays(seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((FC_M, FC_K)).astype(F32)
    W = (rng.standard_normal((FC_K, FC_N)) / math.sqrt(FC_K)).astype(F32)
    b = (0.1 * rng.standard_normal(FC_N)).astype(F32)
    y = rng.standard_normal((FC_M, FC_N)).astype(F32)
    dy = rng.standard_normal((FC_M, FC_N)).astype(F32)
    return [x, W, b, y, dy]


@entry("fully_connected", two(_fc_arrays, 7200), ["fc_forward_f32"])
def _build_fc(dev, real, poison):
    from pointwise_amd import head
    x, W, b, y, dy = inputs = upload(dev, real)
    return Case(inputs, upload(dev, poison), lambda: [head.fully_connected(x, W, b, selu=True), head.fully_connected(x, W, None, selu=False)])


@entry("fully_connected_grad", two(_fc_arrays, 7210), ["fc_backward_f32"])
def _build_fc_grad(dev, real, poison):
    from pointwise_amd import head
    x, W, b, y, dy = inputs = upload(dev, real)

    def run():
        dx, dW, db = head.fully_connected_grad(x, W, y, dy, selu=True)
        _, dW2, db2 = head.fully_connected_grad(x, W, y, dy, selu=False, need_dx=False)
        return [dx, dW, db, dW2, db2]
    return Case(inputs, upload(dev, poison), run)


def _tail_arrays(seed, label_dtype=np.int32):
    rng = np.random.default_rng(seed)
    fc1 = rng.standard_normal((TAIL_M, TAIL_H)).astype(F32)
    W2 = (rng.standard_normal((TAIL_H, TAIL_C)) / math.sqrt(TAIL_H)).astype(F32)
    b2 = (0.1 * rng.standard_normal(TAIL_C)).astype(F32)
    labels = rng.integers(0, TAIL_C, TAIL_M).astype(label_dtype)
    return [fc1, W2, b2, labels]


def _add_tail(training, label_dtype):
    @entry("classification_tail/%s/labels-%s" % ("train" if training else "eval", np.dtype(label_dtype).name),
           two(lambda s: _tail_arrays(s, label_dtype), 7300), ["cls_tail_f32"])
    def build(dev, real, poison):
        from pointwise_amd import head
        fc1, W2, b2, labels = inputs = upload(dev, real)

        def run():
            out = head.classification_tail(fc1, W2, b2, labels, rate=0.5, training=training, seed=3, step=5,
                                           need_grad=training, need_keep=training)
            return [v for v in out.values() if v is not None]
        return Case(inputs, upload(dev, poison), run)


_add_tail(True, np.int32)
_add_tail(True, np.int64)
_add_tail(False, np.int32)

HEAD_B, HEAD_POINTS, HEAD_FEAT, HEAD_HIDDEN, HEAD_CLASSES = 7, 28, 36, 512, 40


def _head_arrays(seed):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((HEAD_B, HEAD_POINTS, HEAD_FEAT)).astype(F32)
    labels = rng.integers(0, HEAD_CLASSES, HEAD_B).astype(np.int32)
    keep = (rng.random((HEAD_B, HEAD_HIDDEN)) < 0.5).astype(F32)
    return [feat, labels, keep]


def _add_head(which):
    reaches = {"forward_backward": ["fc_forward_f32", "cls_tail_f32", "fc_backward_f32"],
               "forward_backward/optimizer": ["fc_forward_f32", "cls_tail_step_f32", "fc_backward_step_f32"],
               "evaluate": ["fc_forward_f32", "cls_tail_f32"],
               "forward+loss+backward": ["fc_forward_f32", "fc_backward_f32"]}[which]

    @entry("ClassificationHead." + which, two(_head_arrays, 7400), reaches)
    def build(dev, real, poison):
        from pointwise_amd import head, optim
        feat, labels, keep = inputs = upload(dev, real)
        h = head.ClassificationHead(HEAD_POINTS, HEAD_CLASSES, HEAD_FEAT, HEAD_HIDDEN, dev, seed=1)
        other = head.ClassificationHead(HEAD_POINTS, HEAD_CLASSES, HEAD_FEAT, HEAD_HIDDEN, dev, seed=2)
        opt = optim.MomentumOptimizer(h.parameters(), 0.01) if which.endswith("optimizer") else None
        saved = [p.clone() for p in h.parameters()]

        def reset():
            h._calls = 0
            for p, s in zip(h.parameters(), saved):
                p.copy_(s)
            if opt is not None:
                for a in opt.accums:
                    a.zero_()

        def run():
            if which == "evaluate":
                pred, counts = h.evaluate(feat, labels)
                return [pred, counts["all"], h.last_loss(), h.logits]
            if which == "forward+loss+backward":
                logits = h.forward(feat, training=True, keep_mask=keep)
                loss, dlogits = h.loss(logits, labels)
                return [logits, loss, h.backward(dlogits)] + h.gradients()
            loss, dfeat = h.forward_backward(feat, labels, optimizer=opt)
            grads = [g for g in h.gradients() if g is not None]
            return [loss, dfeat, h.logits, h.pred, h.counts()["all"]] + grads + h.parameters() + (opt.accums if opt else [])
        return Case(inputs + h.parameters(), upload(dev, poison) + other.parameters(), run, reset)


for _which in ("forward_backward", "forward_backward/optimizer", "evaluate", "forward+loss+backward"):
    _add_head(_which)


# ================================================================================================ the segmentation head
def _seg_arrays(dt, label_dtype):
    def make(seed):
        rng = np.random.default_rng(seed)
        act = rng.standard_normal((B, N, NCLS)).astype(dt)
        labels = rng.integers(-1, NCLS, (B, N)).astype(label_dtype)          # -1: an ignored point, as the head defines it
        pw = (rng.random((B, N)) * (rng.random((B, N)) < 0.8)).astype(dt)
        den = np.array([float(B * N) + rng.integers(1, 9)], dtype=np.float64)
        return [act, labels, pw, den]
    return make


SEG_CLASS_WEIGHTS = [0.5 + 0.125 * c for c in range(NCLS)]


def _add_seg(dt, which, label_dtype=np.int32):
    sfx = _sfx(dt)
    weighted, total, confusion = "seg_head_weighted_" + sfx, "seg_weight_total_" + sfx, "seg_confusion"
    form = {"loss/plain": ("points", False, [weighted]),
            "loss/points/class+point-weights/need_pred": ("points", True, [weighted]),
            "loss/nonzero_weights/class+point-weights": ("nonzero_weights", True, [total, weighted]),
            "loss/sum_weights/class+point-weights": ("sum_weights", True, [total, weighted]),
            "loss/sum_weights/denominator": ("sum_weights", True, [weighted]),
            "weight_total": ("nonzero_weights", True, [total]),
            "evaluate/class+point-weights": ("nonzero_weights", True, [total, weighted]),
            "evaluate/confusion": ("points", False, [weighted, confusion])}[which]
    reduction, weights, reaches = form

    @entry("SegmentationHead.%s/%s/labels-%s" % (which, sfx, np.dtype(label_dtype).name), two(_seg_arrays(dt, label_dtype), 7500),
           reaches)
    def build(dev, real, poison):
        from pointwise_amd import seg_head
        act, labels, pw, den = inputs = upload(dev, real)
        h = seg_head.SegmentationHead(NCLS, dev, class_weights=SEG_CLASS_WEIGHTS if weights else None,
                                      label_smoothing=0.1 if weights else 0.0, reduction=reduction)
        w = pw if weights else None

        def run():
            if which == "weight_total":
                return [h.weight_total(labels, w)]
            if which.startswith("evaluate"):
                pred, counts = h.evaluate(act, labels, point_weights=w, confusion=which.endswith("confusion"))
                return [pred, counts["all"], h.last_loss()] + ([counts["confusion"]] if "confusion" in counts else [])
            out = h.loss(act, labels, need_pred=which.endswith("need_pred"), point_weights=w,
                         denominator=den if which.endswith("denominator") else None)
            return list(out) + [h.counts()["all"]]
        return Case(inputs, upload(dev, poison), run)


for _which in ("loss/plain", "loss/points/class+point-weights/need_pred", "loss/nonzero_weights/class+point-weights",
               "loss/sum_weights/class+point-weights", "loss/sum_weights/denominator", "weight_total",
               "evaluate/class+point-weights", "evaluate/confusion"):
    _add_seg(F32, _which)
for _which in ("loss/plain", "loss/nonzero_weights/class+point-weights", "evaluate/confusion"):
    _add_seg(F64, _which)
_add_seg(F32, "loss/sum_weights/class+point-weights", np.int64)


def _add_seg_plain_c(dt):
    """conv3p_seg_head_f32 / _f64, the head without weights: SegmentationHead goes through the weighted entry whatever its
    settings, so no Python path reaches these; through ctypes."""
    sfx = _sfx(dt)

    @entry("seg_head(C)/" + sfx, two(_seg_arrays(dt, np.int32), 7600), ["seg_head_" + sfx])
    def build(dev, real, poison):
        from pointwise_amd import _lib
        act, labels, pw, den = inputs = upload(dev, real)
        lib = _lib.load()
        rows = B * N
        need = lib.conv3p_seg_head_workspace_bytes(rows, NCLS)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        real_t = ctypes.c_float if dt == F32 else ctypes.c_double

        def run():
            dact = torch.empty_like(act)
            pred = torch.empty((rows,), dtype=torch.int32, device=dev)
            loss = torch.empty((), dtype=torch.float64, device=dev)
            counts = torch.empty(2 + 3 * NCLS, dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                rc = getattr(lib, "conv3p_seg_head_" + sfx)(act.data_ptr(), labels.data_ptr(), rows, NCLS, real_t(1.0 / rows),
                                                            dact.data_ptr(), pred.data_ptr(), loss.data_ptr(), counts.data_ptr(),
                                                            ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream)
            assert rc == _lib.OK
            return [dact, pred, loss, counts]
        return Case(inputs, upload(dev, poison), run)


_add_seg_plain_c(F32)
_add_seg_plain_c(F64)


# ================================================================================================ the optimizer
OPT_SIZES, OPT_OFFSETS = (37, 130, 1000), (1, 41, 173)          # three small tensors at mixed offsets of one buffer
OPT_TOTAL = 1200


def _opt_arrays(dt):
    def make(seed):
        rng = np.random.default_rng(seed)
        return [rng.standard_normal(OPT_TOTAL).astype(dt), (0.1 * rng.standard_normal(OPT_TOTAL)).astype(dt),
                (0.01 * rng.standard_normal(OPT_TOTAL)).astype(dt)]
    return make


def _slices(flat):
    return [flat[o:o + n] for n, o in zip(OPT_SIZES, OPT_OFFSETS)]


def _add_opt(dt, which):
    sfx = _sfx(dt)
    reaches = {"momentum_step": ["momentum_step_" + sfx],
               "momentum_step/nesterov+clip_norm+skip_nonfinite": ["grad_norm_" + sfx, "momentum_step_guarded_" + sfx],
               "grad_sumsq": ["grad_norm_" + sfx],
               "MomentumOptimizer.step/clip_norm+skip_nonfinite": ["grad_norm_" + sfx, "momentum_step_guarded_" + sfx],
               "MomentumOptimizer.step": ["momentum_step_" + sfx]}[which]

    @entry("%s/%s" % (which, sfx), two(_opt_arrays(dt), 7700), reaches)
    def build(dev, real, poison):
        from pointwise_amd import optim
        params, grads, accums = inputs = upload(dev, real)
        saved = [params.clone(), accums.clone()]
        p, g, a = _slices(params), _slices(grads), _slices(accums)
        guarded = "clip_norm" in which
        opt = None
        if which.startswith("MomentumOptimizer"):
            opt = optim.MomentumOptimizer(p, lambda s: 0.01 * 0.5 ** s, momentum=0.9, clip_norm=0.5 if guarded else None,
                                          skip_nonfinite=guarded)
            a = opt.accums

        def reset():
            params.copy_(saved[0])
            accums.copy_(saved[1])
            if opt is not None:
                opt.global_step = 0
                opt.skipped_steps.zero_()
                for t in opt.accums:
                    t.zero_()

        def run():
            if which == "grad_sumsq":
                first = optim.grad_sumsq(g)
                return [first, optim.grad_sumsq(g[:1], out=first.clone(), accumulate=True)]
            if opt is not None:
                opt.step(g)
                return [params] + list(a) + ([opt.grad_stats, opt.skipped_steps] if guarded else [])
            stats = optim.momentum_step(p, g, a, 0.01, 0.9, use_nesterov=guarded, clip_norm=0.5 if guarded else None,
                                        skip_nonfinite=guarded)
            return [params, accums] + ([stats] if stats is not None else [])
        return Case(inputs, upload(dev, poison), run, reset)


for _dt in (F32, F64):
    for _which in ("momentum_step", "momentum_step/nesterov+clip_norm+skip_nonfinite", "grad_sumsq",
                   "MomentumOptimizer.step/clip_norm+skip_nonfinite"):
        _add_opt(_dt, _which)
_add_opt(F32, "MomentumOptimizer.step")


@entry("MomentumOptimizer.fused_fc_step", two(_fc_arrays, 7800), ["fc_backward_step_f32"])
def _build_fused_fc_step(dev, real, poison):
    from pointwise_amd import optim
    x, W, b, y, dy = inputs = upload(dev, real)
    opt = optim.MomentumOptimizer([W, b], 0.01)
    saved = [W.clone(), b.clone()]

    def reset():
        W.copy_(saved[0])
        b.copy_(saved[1])
        for a in opt.accums:
            a.zero_()
    return Case(inputs, upload(dev, poison), lambda: [opt.fused_fc_step(x, W, b, y, dy), W, b] + opt.accums, reset)


# ================================================================================================ the pre-step
def _prestep_arrays(seed):
    rng = np.random.default_rng(seed)
    P = synth.modelnet_like(B, N, seed)
    return [P, rng.standard_normal((B, N, 3)), rng.integers(0, NCLS, (B, N)).astype(np.int32),
            synth.features(B, N, 6, seed + 1, points=P)]


PRESTEP = collections.OrderedDict([
    ("rotate_point_cloud/angles", (["augment_f32"], lambda ps, t: [ps.rotate_point_cloud(t[0], [0.3, 1.7])])),
    ("rotate_point_cloud_by_angle", (["augment_f32"], lambda ps, t: [ps.rotate_point_cloud_by_angle(t[0], 0.9)])),
    ("jitter_point_cloud/noise", (["augment_f32"], lambda ps, t: [ps.jitter_point_cloud(t[0], noise=t[1])])),
    ("rotate_and_jitter/angles+noise", (["augment_f32"], lambda ps, t: [ps.rotate_and_jitter(t[0], [0.3, 1.7], noise=t[1])])),
    ("sort_order_xyz", (["sort_xyz_order_f32"], lambda ps, t: [ps.sort_order_xyz(t[3])])),
    ("sort_order_morton", (["sort_morton_order_f32"], lambda ps, t: [ps.sort_order_morton(t[3])])),
    ("sort_point_cloud_xyz", (["sort_xyz_order_f32", "gather_rows"], lambda ps, t: [ps.sort_point_cloud_xyz(t[3])])),
    ("sort_point_cloud_xyz2", (["sort_xyz_order_f32", "gather_rows"], lambda ps, t: list(ps.sort_point_cloud_xyz2(t[0], t[2])))),
    ("sort_point_cloud_morton", (["sort_morton_order_f32", "gather_rows"], lambda ps, t: [ps.sort_point_cloud_morton(t[3])])),
    ("sort_point_cloud_morton2", (["sort_morton_order_f32", "gather_rows"],
                                  lambda ps, t: list(ps.sort_point_cloud_morton2(t[0], t[2])))),
    ("sort_order/wide/xyz", (["sort_order_f32"], lambda ps, t: [ps.sort_order(t[3], "xyz")])),
    ("sort_order/wide/morton", (["sort_order_f32"], lambda ps, t: [ps.sort_order(t[3], "morton")])),
    ("sort_point_cloud/morton", (["sort_order_f32", "gather_rows"], lambda ps, t: [ps.sort_point_cloud(t[3], "morton")])),
    ("sort_point_cloud2/xyz", (["sort_order_f32", "gather_rows"], lambda ps, t: list(ps.sort_point_cloud2(t[0], t[2], "xyz")))),
])


def _add_prestep(name, reaches, call):
    @entry("prestep." + name, two(_prestep_arrays, 7900), reaches)
    def build(dev, real, poison):
        from pointwise_amd import prestep
        inputs = upload(dev, real)
        return Case(inputs, upload(dev, poison), lambda: call(prestep, inputs))


for _name, (_reaches, _call) in PRESTEP.items():
    _add_prestep(_name, _reaches, _call)


# ================================================================================================ the batch provider
PROV_S = 6


def _provider_arrays(per_point):
    def make(seed):
        rng = np.random.default_rng(seed)
        data = np.stack([synth.modelnet_like(1, N, seed + i)[0] for i in range(PROV_S)])
        labels = rng.integers(0, NCLS, (PROV_S, N) if per_point else (PROV_S,)).astype(np.int32)
        return [data, labels, rng.permutation(PROV_S).astype(np.int32)]
    return make


def _add_assemble(which):
    wide = which == "wide_sort"

    @entry("assemble_batch/" + which, two(_provider_arrays(which != "plain"), 8000),
           ["provider_batch_wide_f32" if wide else "provider_batch_f32"])
    def build(dev, real, poison):
        from pointwise_amd import provider
        data, labels, perm = inputs = upload(dev, real)

        def run():
            res = provider.assemble_batch(data, labels, B, perm=perm, start=1, rotate=True, jitter=True, sort_cloud=which != "plain",
                                          seed=5, step=9, return_randoms=which == "return_randoms", wide_sort=wide,
                                          sort_method="morton" if wide else "xyz")
            return list(res[:4]) + (list(res[4].values()) if len(res) > 4 else [])
        return Case(inputs, upload(dev, poison), run)


for _which in ("plain", "sort_cloud", "return_randoms", "wide_sort"):
    _add_assemble(_which)


def _add_batch_provider(which):
    name = {"steady": "BatchProvider.get_batch_point_cloud", "epoch": "BatchProvider.next_epoch+get_batch_point_cloud"}[which]

    @entry(name, two(_provider_arrays(False), 8100), ["provider_batch_f32"])
    def build(dev, real, poison):
        from pointwise_amd import provider
        bp = provider.BatchProvider(real[0], real[1], B, device=dev, sort_cloud=True, seed=4)
        other = provider.BatchProvider(poison[0], poison[1], B, device=dev, sort_cloud=True, seed=5)
        inputs, bad = [bp.data, bp.labels], [other.data, other.labels]
        if which == "steady":                      # the epoch's permutation is an input like the data: another one is valid
            inputs, bad = inputs + [bp.permutation], bad + [other.permutation]

        def reset():
            bp._turn = 0
            if which == "epoch":
                bp.load_state_dict({"seed": 4, "epoch": 0, "cur_batch": 0})
            else:
                bp.cur_batch = 0

        def run():
            if which == "epoch":
                bp.next_epoch()
            return list(bp.get_batch_point_cloud()) + [bp.bad_index]
        return Case(inputs, bad, run, reset)


_add_batch_provider("steady")
_add_batch_provider("epoch")


# ================================================================================================ scene
ROOM_START = [0, 1400, ROOM_ROWS]
SCENE_KW = dict(num_point=256, block=1.0, stride=0.5, min_points=20, max_blocks=96, seed=3, step=1)
SCENE_OUT = ("data", "labels", "index", "block_cell", "block_count", "stats", "block_room", "room_blocks", "room_stats")


def _room_arrays(seed):
    rng = np.random.default_rng(seed)
    xyz = synth.room_like(1, ROOM_ROWS, seed, extent=(2.5, 2.0, 3.0))[0]
    data = np.concatenate([xyz, rng.random((ROOM_ROWS, 3)).astype(F32)], axis=1)
    return [data, rng.integers(0, NCLS, ROOM_ROWS).astype(np.int32)]


def _add_scene_blocks(which):
    rooms = which.startswith("rooms")
    reach = "scene_blocks_rooms_f32" if rooms else "scene_blocks_cover_f32" if which == "cover" else "scene_blocks_f32"

    def make(seed):
        return _room_arrays(seed) + [np.array([0, 1400 + (seed % 7) * 10, ROOM_ROWS], dtype=np.int32)]

    @entry(("scene_blocks_rooms/" + which[6:]) if rooms else "scene_blocks/" + which, two(make, 8200), [reach])
    def build(dev, real, poison):
        from pointwise_amd import scene
        data, labels, room_start = inputs = upload(dev, real)
        bad = upload(dev, poison)
        if which == "rooms/host-list":             # the list is the host's: not an input on the device
            inputs, bad = inputs[:2], bad[:2]

        def run():
            if rooms:
                sb = scene.scene_blocks_rooms(data, room_start if which == "rooms/device" else ROOM_START, labels,
                                              cover=which == "rooms/cover", **SCENE_KW)
            else:
                sb = scene.scene_blocks(data, labels, cover=which == "cover", **SCENE_KW)
            return tensors(sb, SCENE_OUT)
        return Case(inputs, bad, run)


for _which in ("plain", "cover", "rooms/device", "rooms/cover", "rooms/host-list"):
    _add_scene_blocks(_which)


def _vote_arrays(seed):
    rng = np.random.default_rng(seed)
    rows = 4 * 256
    return [rng.integers(0, NCLS, rows).astype(np.int32), rng.integers(-1, ROOM_ROWS, rows).astype(np.int32),
            rng.standard_normal((rows, NCLS)).astype(F32)]


@entry("SceneVotes.add+labels+counts", two(_vote_arrays, 8300), ["scene_vote", "scene_vote_labels"])
def _build_votes(dev, real, poison):
    from pointwise_amd import scene
    pred, index, logits = inputs = upload(dev, real)
    votes = scene.SceneVotes(ROOM_ROWS, NCLS, dev)

    def run():
        votes.add(pred, index)
        return [votes.labels().clone(), votes.counts().clone(), votes.votes]
    return Case(inputs, upload(dev, poison), run, votes.reset)


@entry("SceneScores.add+labels+counts", two(_vote_arrays, 8310), ["scene_vote_scores_f32", "scene_score_labels"])
def _build_scores(dev, real, poison):
    from pointwise_amd import scene
    pred, index, logits = inputs = upload(dev, real)
    scores = scene.SceneScores(ROOM_ROWS, NCLS, dev)

    def run():
        scores.add(logits, index)
        return [scores.labels().clone(), scores.counts().clone(), scores.scores, scores.vote_stats]
    return Case(inputs, upload(dev, poison), run, scores.reset)


# ================================================================================================ grid
GRID_VOXEL = 0.08
GRID_STATE = ("data", "labels", "inverse", "voxel_row", "voxel_count", "voxel_cell", "stats", "voxel_room", "voxel_start",
              "room_stats")
SEG_STATE = ("segment", "root", "size", "rows", "label", "stats")


def _grid_pair(dev, real, poison, rooms=False):
    """The subsampling of both halves, neighbour tables built: (raw data, g) twice.  Both have max_voxels = the rows, so
    every tensor of one is a valid stand-in for the other's: voxel and row numbers stay in range."""
    from pointwise_amd import grid
    out = []
    for arrays in (real, poison):
        data, labels = upload(dev, arrays[:2])
        if rooms:
            g = grid.grid_subsample_rooms(data, torch.tensor(ROOM_START, dtype=torch.int32).to(dev), labels, voxel=GRID_VOXEL,
                                          num_class=NCLS)
        else:
            g = grid.grid_subsample(data, labels, voxel=GRID_VOXEL, num_class=NCLS)
        g.neighbors()
        out.append((data, labels, g))
    return out


def _grid_state(g):
    return tensors(g, GRID_STATE) + [g._neigh]


def _voxel_labels(g):
    """A label per voxel in slabs, so that segments have some size: from the voxels' own coordinates, on the device."""
    lab = (torch.floor(g.data[:, 0] / 0.6) + 3 * torch.floor(g.data[:, 2] / 0.8)).to(torch.int32) % NCLS
    return lab.clamp_(0, NCLS - 1).contiguous()


def _add_subsample(which):
    rooms = which == "rooms"
    reach = "grid_subsample_rooms_f32" if rooms else "grid_subsample_f32"

    def make(seed):
        return _room_arrays(seed) + [np.array([0, 1400 + (seed % 7) * 10, ROOM_ROWS], dtype=np.int32)]

    @entry("grid_subsample_rooms" if rooms else "grid_subsample/" + which, two(make, 8400), [reach])
    def build(dev, real, poison):
        from pointwise_amd import grid
        data, labels, room_start = inputs = upload(dev, real)
        bad = upload(dev, poison)
        if not rooms:
            inputs, bad = inputs[:2], bad[:2]

        def run():
            if rooms:
                g = grid.grid_subsample_rooms(data, room_start, labels, voxel=GRID_VOXEL, num_class=NCLS)
            else:
                g = grid.grid_subsample(data, labels, voxel=GRID_VOXEL, mode=which, num_class=NCLS if which == "mean" else None)
            return tensors(g, GRID_STATE)
        return Case(inputs, bad, run)


for _which in ("mean", "center", "rooms"):
    _add_subsample(_which)


def _add_grid(name, reaches, make_run, rooms=False, seed=8500):
    """A method of GridSubsample on a subsampling made in build(): make_run(dev, a, b) -> (run, reset or None, further
    (input, poison) pairs), a and b the (raw data, raw labels, g) of the two halves."""
    @entry(name, two(_room_arrays, seed), reaches)
    def build(dev, real, poison):
        a, b = _grid_pair(dev, real, poison, rooms)
        run, reset, more = make_run(dev, a, b)
        inputs = [a[0]] + _grid_state(a[2]) + [x for x, _ in more]
        bad = [b[0]] + _grid_state(b[2]) + [p for _, p in more]
        return Case(inputs, bad, run, reset or (lambda: None))


def _run_project(dev, a, b):
    la, lb = _voxel_labels(a[2]), _voxel_labels(b[2])
    return (lambda: [a[2].project(la)]), None, [(la, lb)]


def _run_neighbors(dev, a, b):
    g = a[2]

    def reset():
        g._neigh = None
    return (lambda: [g.neighbors()]), reset, []     # (the table of build() stays among the inputs; the call makes a new one)


def _scores_pair(dev, a, b):
    rng = np.random.default_rng(8600)
    M = a[2].data.shape[0]
    return [torch.from_numpy(rng.standard_normal((M, NCLS)).astype(F32)).to(dev) for _ in range(2)]


def _run_interpolate(scores_kind, rings):
    def make(dev, a, b):
        from pointwise_amd import scene
        g = a[2]
        M = g.data.shape[0]
        sa, sb = _scores_pair(dev, a, b)
        if scores_kind == "f32":
            arg, more, reset = sa, [(sa, sb)], None
        else:
            tables = []
            for logits, seed in ((sa, 1), (sb, 2)):
                t = scene.SceneScores(M, NCLS, dev)
                idx = torch.from_numpy(np.random.default_rng(seed).integers(-1, M, M).astype(np.int32)).to(dev)
                t.add(logits, idx)
                tables.append(t)
            arg, more = tables[0], [(tables[0].scores, tables[1].scores)]

            def reset():
                arg._fresh = False                 # labels() of the sums is part of the call

        def run():
            out = g.interpolate(a[0], arg, k=3, return_scores=True, rings=rings, return_ring=rings > 1)
            return list(out) + [g.interp_stats] + ([g.ring_stats] if rings > 1 else [])
        return run, reset, more
    return make


def _run_normals(viewpoint):
    def make(dev, a, b):
        g = a[2]
        vp, more = viewpoint, []
        if viewpoint == "tensor":
            vp = torch.tensor([[1.0, 0.5, 1.5]], dtype=torch.float32).to(dev)
            more = [(vp, torch.tensor([[-1.0, 2.5, 0.5]], dtype=torch.float32).to(dev))]
        elif viewpoint == "per-room":
            vp = torch.tensor([[1.0, 0.5, 1.5], [0.2, 0.1, 3.5]], dtype=torch.float32).to(dev)
            more = [(vp, torch.tensor([[-1.0, 2.5, 0.5], [2.0, 2.0, 2.0]], dtype=torch.float32).to(dev))]

        def run():
            nrm = g.normals(viewpoint=vp, return_moments=True)
            return tensors(nrm, ("normals", "curvature", "samples", "flags", "moments", "stats"))
        return run, None, more
    return make


def _run_segments(smooth):
    def make(dev, a, b):
        la, lb = _voxel_labels(a[2]), _voxel_labels(b[2])
        more = [(la, lb)]
        kw = {}
        if smooth:
            na, nb = a[2].normals(), b[2].normals()
            kw = dict(normals=na, max_angle=30.0, max_curvature=0.2, features=a[2].data[:, 3:6], max_difference=0.5)
            more += list(zip(tensors(na, ("normals", "curvature", "flags")), tensors(nb, ("normals", "curvature", "flags"))))

        def run():
            seg = a[2].segments(la, NCLS, 26, **kw)
            return tensors(seg, SEG_STATE + ("smooth_stats",))
        return run, None, more
    return make


def _segmentations(a, b):
    la, lb = _voxel_labels(a[2]), _voxel_labels(b[2])
    sa, sb = a[2].segments(la, NCLS, 26), b[2].segments(lb, NCLS, 26)
    return sa, sb, [(la, lb)] + list(zip(tensors(sa, SEG_STATE), tensors(sb, SEG_STATE)))


def _run_absorb(dev, a, b):
    sa, sb, more = _segmentations(a, b)
    return (lambda: [sa.absorb(6), sa.absorbed_label, sa.absorb_stats]), None, more


def _run_geometry(weight):
    def make(dev, a, b):
        sa, sb, more = _segmentations(a, b)
        names = ("cell_box", "box", "moments", "centroid", "eigenvalues", "axes", "extent", "stats")
        return (lambda: tensors(sa.geometry(weight), names)), None, more
    return make


ADJ_OUT = ("start", "src", "dst", "contacts", "voxels", "offset", "twin", "border", "stats")


def _run_adjacency(dev, a, b):
    sa, sb, more = _segmentations(a, b)
    return (lambda: tensors(sa.adjacency(max_edges=8 * sa.shape[0]), ADJ_OUT)), None, more


def _run_merge(select):
    def make(dev, a, b):
        sa, sb, more = _segmentations(a, b)
        adj = [s.adjacency(max_edges=8 * s.shape[0]) for s in (sa, sb)]
        assert not adj[0].overflowed() and not adj[1].overflowed()
        more = more + list(zip(tensors(adj[0], ("src", "dst", "contacts")), tensors(adj[1], ("src", "dst", "contacts"))))

        def run():
            if select == "bool":                   # a policy as a torch expression, as adjacency()'s docstring writes it
                merged = adj[0].merge(adj[0].contacts > 4)
            else:
                merged = sa.merge(adj[0].src, adj[0].dst)
            return tensors(merged, SEG_STATE + ("seg_map", "merge_stats"))
        return run, None, more
    return make


def _run_pool(kind):
    def make(dev, a, b):
        from pointwise_amd import scene
        sa, sb, more = _segmentations(a, b)
        if kind == "f32":
            values, weight = a[2].data[:, 3:6], "rows"      # a column slice: strided rows; g.data is an input already
        else:
            M = a[2].data.shape[0]
            tables = []
            for seed in (1, 2):
                rng = np.random.default_rng(8700 + seed)
                t = scene.SceneScores(M, NCLS, dev)
                t.add(torch.from_numpy(rng.standard_normal((M, NCLS)).astype(F32)).to(dev),
                      torch.from_numpy(rng.integers(-1, M, M).astype(np.int32)).to(dev))
                tables.append(t)
            values, weight = tables[0].scores, "voxels"
            more = more + [(tables[0].scores, tables[1].scores)]
        names = ("sums", "weights", "mean", "label", "voxel_label", "stats")
        return (lambda: tensors(sa.pool(values, weight), names)), None, more
    return make


_add_grid("GridSubsample.project", ["grid_project_labels"], _run_project)
_add_grid("GridSubsample.neighbors", ["grid_neighbors"], _run_neighbors)
_add_grid("GridSubsample.neighbors/rooms", ["grid_neighbors"], _run_neighbors, rooms=True)
_add_grid("GridSubsample.interpolate/f32/rings1", ["grid_interpolate_f32"], _run_interpolate("f32", 1))
_add_grid("GridSubsample.interpolate/f32/rings3", ["grid_interpolate_rings_f32"], _run_interpolate("f32", 3))
_add_grid("GridSubsample.interpolate/SceneScores-i64/rings1", ["scene_score_labels", "grid_interpolate_i64"],
          _run_interpolate("i64", 1))
_add_grid("GridSubsample.interpolate/SceneScores-i64/rings3", ["scene_score_labels", "grid_interpolate_rings_i64"],
          _run_interpolate("i64", 3))
_add_grid("GridSubsample.interpolate/f32/rings3/rooms", ["grid_interpolate_rings_f32"], _run_interpolate("f32", 3), rooms=True)
_add_grid("GridSubsample.normals/viewpoint-none", ["grid_normals_f32"], _run_normals(None))
_add_grid("GridSubsample.normals/viewpoint-tensor", ["grid_normals_f32"], _run_normals("tensor"))
_add_grid("GridSubsample.normals/viewpoint-tuple", ["grid_normals_f32"], _run_normals((1.0, 0.5, 1.5)))
_add_grid("GridSubsample.normals/viewpoint-per-room", ["grid_normals_f32"], _run_normals("per-room"), rooms=True)
_add_grid("GridSubsample.segments/plain", ["grid_segments"], _run_segments(False))
_add_grid("GridSubsample.segments/smooth", ["grid_segments_smooth"], _run_segments(True))
_add_grid("GridSegments.absorb", ["grid_absorb_segments"], _run_absorb)
_add_grid("GridSegments.geometry/voxels", ["grid_segment_geometry"], _run_geometry("voxels"))
_add_grid("GridSegments.geometry/rows", ["grid_segment_geometry"], _run_geometry("rows"))
_add_grid("GridSegments.adjacency", ["grid_segment_adjacency"], _run_adjacency)
_add_grid("GridSegments.merge", ["grid_merge_segments"], _run_merge(None))
_add_grid("SegmentAdjacency.merge/select-bool", ["grid_merge_segments"], _run_merge("bool"))
_add_grid("GridSegments.pool/f32", ["grid_segment_pool_f32"], _run_pool("f32"))
_add_grid("GridSegments.pool/i64", ["grid_segment_pool_i64"], _run_pool("i64"))

NAMES = [e.name for e in ENTRIES]


# ================================================================================================ the table, run
def report(dev, out):
    from tests import stream_rig
    stream, tries, plants = stream_rig.find_stream(dev)
    out("stream contract on %s: torch stream try %d of 4 %s" % (
        torch.cuda.get_device_name(dev), tries, "sees the wrong-stream plant" if stream is not None else "DOES NOT SEE the plant"))
    out("%-72s %10s %9s %8s %12s" % ("case", "t_host ms", "delay ms", "ordered", "asynchronous"))
    rows = [("plant: " + k, v) for k, v in plants.items()]
    if stream is not None:
        for e in ENTRIES:
            real, poison = e.halves()
            rows.append((e.name, stream_rig.judge(e.build(dev, real, poison), stream)))
    bad = 0
    for name, v in rows:
        waived = " (host by contract)" if name in HOST_BY_CONTRACT else ""
        out("%-72s %10.3f %9.1f %8s %12s%s%s" % (name, v.t_host_ms, v.delay_ms, v.ordered, v.asynchronous, waived,
                                                 "" if v.deterministic else "  NOT DETERMINISTIC"))
        if not name.startswith("plant: "):
            bad += (v.ordered is not True) or (v.asynchronous is not True and not waived)
    out("%d cases, %d outside the contract" % (len(rows) - len(plants), bad))
    return bad


if __name__ == "__main__":
    assert torch.cuda.is_available(), "the stream contract needs a HIP device"
    raise SystemExit(1 if report(torch.device("cuda:0"), print) else 0)
