"""The stream-contract cases of include/conv3p_knn.h: the table of tests/stream_contract_cases.py continued for the header of
the k-nearest-voxel search, with the same Entry and the same builders, as tests/stream_contract_graph_cases.py continues it
for conv3p_graph.h.  It keeps a list of its own -- the main table, and the CPU test that pins it to conv3p.h and to
pointwise_amd.__all__, stay as they are.  Importing this module does not touch the device."""
import os

import numpy as np
import torch

from tests import stream_contract_cases as main
from tests.stream_rig import Case

ENTRIES = []
HEADER = os.path.join(os.path.dirname(main.HEADER), "conv3p_knn.h")
KNN_OUT = ("index", "d2", "count", "ring", "scanned", "certified", "stats")
NORMALS_OUT = ("normals", "curvature", "samples", "flags", "moments", "stats")


def streamed_functions():
    """Every function include/conv3p_knn.h declares with a `void *stream` parameter."""
    return main.streamed_functions(HEADER)


def _add(name, reaches, make_run, rooms=False, seed=9100):
    """main._add_grid for this table: a call on a subsampling made in build(); make_run(dev, a, b) -> (run, reset or None,
    further (input, poison) pairs), a and b the (raw data, raw labels, g) of the two halves.  The poison is another
    seed's room and its subsampling of the same shapes: every voxel and row number of it is in range."""
    def build(dev, real, poison):
        a, b = main._grid_pair(dev, real, poison, rooms)
        run, reset, more = make_run(dev, a, b)
        inputs = [a[0]] + main._grid_state(a[2]) + [x for x, _ in more]
        bad = [b[0]] + main._grid_state(b[2]) + [p for _, p in more]
        return Case(inputs, bad, run, reset or (lambda: None))
    ENTRIES.append(main.Entry(name, main.two(main._room_arrays, seed), build, frozenset("conv3p_" + r for r in reaches)))


def _run_knn(rows, rings):
    def make(dev, a, b):
        g = a[2]
        va, vb = ((main._voxel_labels(x[2]) % 3) - 1 for x in (a, b))            # a third of the voxels are no neighbours
        va, vb = va.contiguous(), vb.contiguous()

        def run():
            t = g.knn(main.GRID_VOXEL, a[0] if rows else None, k=8, rings=rings, valid_labels=va, exclude_self=not rows)
            return main.tensors(t, KNN_OUT)
        return run, None, [(va, vb)]
    return make


def _tables(a, b, **kw):
    """The voxels' table of both halves, made in build(): the inputs of the consumers and their poison."""
    ta, tb = (x[2].knn(main.GRID_VOXEL, **kw) for x in (a, b))
    return ta, tb, list(zip(main.tensors(ta, KNN_OUT[:3]), main.tensors(tb, KNN_OUT[:3])))


def _run_interpolate(kind):
    def make(dev, a, b):
        from pointwise_amd import scene
        M = a[2].data.shape[0]
        ta, tb, more = _tables(a, b, points=None, k=8, rings=2)
        sa, sb = main._scores_pair(dev, a, b)
        if kind == "i64":
            sums = []
            for logits, seed in ((sa, 1), (sb, 2)):
                t = scene.SceneScores(M, main.NCLS, dev)
                t.add(logits, torch.from_numpy(np.random.default_rng(seed).integers(-1, M, M).astype(np.int32)).to(dev))
                sums.append(t)
            arg, more = sums[0], more + [(sums[0].scores, sums[1].scores)]
        else:
            arg, more = sa, more + [(sa, sb)]

        def run():
            return list(ta.interpolate(arg, k=5, return_scores=True)) + [ta.interp_stats]
        return run, None, more
    return make


def _run_normals(dev, a, b):
    ta, tb, more = _tables(a, b, points=None, k=16, rings=2)
    vp = torch.tensor([[1.0, 0.5, 1.5]], dtype=torch.float32).to(dev)
    more = more + [(vp, torch.tensor([[-1.0, 2.5, 0.5]], dtype=torch.float32).to(dev))]

    def run():
        return main.tensors(ta.normals(viewpoint=vp, return_moments=True), NORMALS_OUT)
    return run, None, more


_add("GridSubsample.knn/voxels", ["grid_knn_f32"], _run_knn(False, 2))
_add("GridSubsample.knn/rows, one ring", ["grid_knn_f32"], _run_knn(True, 1))
_add("GridRoomSubsample.knn/rows, eight rings", ["grid_knn_f32"], _run_knn(True, 8), rooms=True)
_add("GridKnn.interpolate/f32", ["grid_interpolate_knn_f32"], _run_interpolate("f32"))
_add("GridKnn.interpolate/SceneScores", ["grid_interpolate_knn_i64"], _run_interpolate("i64"))
_add("GridKnn.normals", ["grid_normals_knn_f32"], _run_normals)
NAMES = [e.name for e in ENTRIES]
