"""The case list that pins the host's launch decisions: which launchers run and how often, which zero-fills are issued,
when a search is skipped and which companion stencils ride along.  The profile calls (conv3p_profile_*) count host-side
launch scopes per kind; the counts depend on the host's decisions alone, never on the data or the device.

    python -m tests.launch_census_cases      records tests/golden/launch_census.json from the library as it stands

tests/test_launch_census.py replays the list and compares with that file by equality.  The file was written once, from
the library before its core host glue was split by concern, and is not edited: a change of the host glue that moves a
count has changed behaviour.

Every case is small: B = 2 clouds of N = 130 points (three tiles, the last ragged), voxel 0.1, inputs from
tests/parity_util.make_case, filter extents from EXT of tests/test_dispatch_map.py.  A single-layer case runs at strides
(1, 1, 1) and (2, 2, 2), stateless and through a cache sized for it; a hint or a matmul precision needs the cache.
"""
import collections
import ctypes
import json
import os

import numpy as np
import torch

from pointwise_amd import _lib, conv3p_op as op
from tests.parity_util import make_case
from tests.test_dispatch_map import EXT
from tests.test_stack_descriptors import Row, S, StackRun, _case as stack_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_census.json")
VOX = 0.1
B, N = 2, 130
F32, F64 = np.float32, np.float64
STRIDES = ((1, 1, 1), (2, 2, 2))
HINTS = {"none": None, "sparse": True, "dense": False}

# name, dtype, Cin, Cout, taps, hints run through the cache, matmul precisions run through the cache
Layer = collections.namedtuple("Layer", "name dt cin cout taps hints matmul")
LAYERS = [
    # register path, fp32: dense G / populated rows by hint and dilation; transform + gather forward; 64 .. 128-bit tap sets
    Layer("register-f32-9to9-t27", F32, 9, 9, 27, ("none", "sparse", "dense"), ("highest",)),
    Layer("register-f32-36to13-t27", F32, 36, 13, 27, ("none",), ("highest",)),
    Layer("register-f32-3to9-t65", F32, 3, 9, 65, ("none",), ("highest",)),
    # register path, fp64; 36 -> 13: the backward's column split
    Layer("register-f64-9to9-t27", F64, 9, 9, 27, ("none",), ("highest",)),
    Layer("register-f64-36to13-t27", F64, 36, 13, 27, ("none",), ("highest",)),
    # matrix-core kernels
    Layer("matrix-core-5to7-t27", F32, 5, 7, 27, ("none",), ("highest",)),
    Layer("matrix-core-36to13-t33", F32, 36, 13, 33, ("none",), ("highest",)),
    Layer("matrix-core-32to64-t27", F32, 32, 64, 27, ("none",), ("highest", "medium")),
    # more than 256 channels: blocks on the matrix-core kernels
    Layer("wide-260to260-t27", F32, 260, 260, 27, ("none",), ("highest",)),
    Layer("wide-300to70-t27", F32, 300, 70, 27, ("none",), ("highest",)),
    Layer("wide-40to260-t27", F32, 40, 260, 27, ("none",), ("highest",)),
    # fp64 channel blocks: backward blocks of 8, 4 and 2 output channels
    Layer("f64-blocks-17to9-t27", F64, 17, 9, 27, ("none",), ("highest",)),
    Layer("f64-blocks-17to9-t45", F64, 17, 9, 45, ("none",), ("highest",)),
    Layer("f64-blocks-17to9-t65", F64, 17, 9, 65, ("none",), ("highest",)),
    Layer("f64-blocks-5to7-t27", F64, 5, 7, 27, ("none",), ("highest",)),
    # the generic thread-per-pair kernels
    Layer("generic-f32-5to7-t65", F32, 5, 7, 65, ("none",), ("highest",)),
    Layer("generic-f64-9to9-t125", F64, 9, 9, 125, ("none",), ("highest",)),
]
# three hidden layers of width 9 from 3 inputs, without and with a 13-class head; the fused-launch flags stay off (whether a
# fused launch is taken depends on the device census)
STACKS = [
    Row("census-stack", F32, 3, 9, 3, 0, (3, 3, 3), S(1, 2, 3), None, None, False, "modelnet", B, N),
    Row("census-stack-head13", F32, 3, 9, 3, 13, (3, 3, 3), S(1, 2, 3), (1, 1, 1), None, False, "modelnet", B, N),
]


def _tdt(dt):
    return torch.float32 if dt == F32 else torch.float64


def _to(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def read_census(lib):
    """{kind name: launches} of everything recorded since the last reset, kinds without a launch left out."""
    seen = {}
    for k in range(lib.conv3p_profile_kinds()):
        n = ctypes.c_uint64(0)
        assert lib.conv3p_profile_read(k, ctypes.byref(n), None) == _lib.OK
        if n.value:
            seen[lib.conv3p_profile_name(k).decode()] = n.value
    lib.conv3p_profile_reset()
    return seen


class Census:
    """The profile switched on around a sequence of calls; call(thunk) returns the thunk's result and notes its census."""

    def __init__(self):
        self.lib = _lib.load()
        self.calls = []

    def __enter__(self):
        self.lib.conv3p_profile_reset()
        self.lib.conv3p_profile_enable(1)
        return self

    def __exit__(self, *exc):
        self.lib.conv3p_profile_enable(0)
        self.lib.conv3p_profile_reset()

    def call(self, thunk):
        res = thunk()
        torch.cuda.synchronize()
        self.calls.append(read_census(self.lib))
        return res


def _pair(dev, tensors, s, cache, unchanged=False):
    """One forward and one backward call: ({"forward": census, "backward": census}, (y, dX, dW))."""
    tp, tx, tw, tdy = tensors
    with Census() as c:
        y = c.call(lambda: op.conv3p(tp, tx, tw, s, VOX, cache=cache, points_unchanged=unchanged))
        dx, dw = c.call(lambda: op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache, points_unchanged=unchanged))
    return {"forward": c.calls[0], "backward": c.calls[1]}, (y, dx, dw)


def run_layer(dev, case):
    """Every variant of a single-layer case: {variant: {"forward": census, "backward": census}} and {variant: (y, dX, dW)}."""
    filt = EXT[case.taps]
    tensors = _to(dev, *make_case("modelnet", B, N, case.cin, case.cout, filt, seed=4100 + 11 * LAYERS.index(case), dtype=case.dt))
    census, outputs = {}, {}
    for s in STRIDES:
        tag = "s%d" % s[0]
        census[tag + "/stateless"], outputs[tag + "/stateless"] = _pair(dev, tensors, s, None)
        for hint in case.hints:
            for matmul in case.matmul:
                cache = op.NeighborCache(B, N, _tdt(case.dt), dev, slots=1, max_taps=case.taps, max_cin=case.cin,
                                         max_cout=case.cout, sparse_neighbourhoods=HINTS[hint], matmul_precision=matmul)
                assert cache.fits(B, N, _tdt(case.dt), dev, case.taps, case.cin, case.cout)
                key = "%s/cache/%s/%s" % (tag, hint, matmul)
                census[key], outputs[key] = _pair(dev, tensors, s, cache)
    return census, outputs


def run_two_slots(dev):
    """9 -> 9 on ONE cache of two slots: forward stride 1, forward stride 2, backward stride 2, backward stride 1 on fresh
    points, then the same four calls under the points-unchanged hint: the companions and the skip flags."""
    tp, tx, tw, tdy = _to(dev, *make_case("modelnet", B, N, 9, 9, EXT[27], seed=4500))
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=2, max_taps=27, max_cin=9, max_cout=9)
    s1, s2 = STRIDES
    out = {}
    with Census() as c:
        for unchanged in (False, True):
            tag = "hinted" if unchanged else "fresh"
            out[tag + "/forward-s1"] = c.call(lambda: op.conv3p(tp, tx, tw, s1, VOX, cache=cache, points_unchanged=unchanged))
            out[tag + "/forward-s2"] = c.call(lambda: op.conv3p(tp, tx, tw, s2, VOX, cache=cache, points_unchanged=unchanged))
            out[tag + "/backward-s2"] = c.call(lambda: op.conv3p_grad(tdy, tp, tx, tw, s2, VOX, cache=cache, points_unchanged=unchanged))
            out[tag + "/backward-s1"] = c.call(lambda: op.conv3p_grad(tdy, tp, tx, tw, s1, VOX, cache=cache, points_unchanged=unchanged))
    return dict(zip(out, c.calls)), out


def run_prepared_orders(dev):
    """32 -> 64: prepare with the matrix-core path's record orders, then a forward and a backward that find them."""
    tp, tx, tw, tdy = _to(dev, *make_case("modelnet", B, N, 32, 64, EXT[27], seed=4600))
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=32, max_cout=64)
    s = STRIDES[0]
    with Census() as c:
        c.call(lambda: op.cache_prepare(tp, EXT[27], s, VOX, cache, deep_orders=True))
        y = c.call(lambda: op.conv3p(tp, tx, tw, s, VOX, cache=cache, points_unchanged=True))
        dx, dw = c.call(lambda: op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache, points_unchanged=True))
    return dict(zip(("prepare", "forward", "backward"), c.calls)), {"forward": y, "backward": (dx, dw)}


def run_stack(dev, row):
    """One forward and one backward of the stack-level entry points, the geometry built inline and by a prefetch."""
    census, outputs = {}, {}
    for geometry in ("inline", "prefetch"):
        r = StackRun(dev, row, stack_case(row))
        with Census() as c:
            if geometry == "prefetch":
                assert c.call(r.prefetch) == _lib.OK
            assert c.call(r.forward) == _lib.OK
            assert c.call(r.backward) == _lib.OK
        census[geometry] = dict(zip(("prefetch", "forward", "backward")[-len(c.calls):], c.calls))
        acts, dx, grads = r.results()
        outputs[geometry] = tuple(acts) + (dx,) + tuple(grads)
    return census, outputs


CASES = collections.OrderedDict((case.name, lambda dev, case=case: run_layer(dev, case)) for case in LAYERS)
CASES["two-slots-9to9"] = run_two_slots
CASES["prepared-orders-32to64"] = run_prepared_orders
for _row in STACKS:
    CASES[_row.name] = lambda dev, row=_row: run_stack(dev, row)


def record(dev):
    return {name: run(dev)[0] for name, run in CASES.items()}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "recording the launch census needs a HIP device"
    table = record(torch.device("cuda:0"))
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(table), GOLDEN))
