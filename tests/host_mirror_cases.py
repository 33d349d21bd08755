"""The case table that pins the Python host mirror's behaviour before any device work: which exception and which message
every argument check of scene.py, grid.py, provider.py and prestep.py raises and in which ORDER, what the output classes'
trim() and room() hand out (type, shape, own tensor or view and at which offset), and the host-only block bounds.

    python -m tests.host_mirror_cases        records tests/golden/host_mirror.json from the package as it stands

tests/test_host_mirror_host.py replays the table and compares with that file by equality.  Every check runs before the
device is touched, so CPU tensors (and tensors on the "meta" device, where a check needs a device that is not the CPU or a
row count past a limit) reach all of them.

A ladder: a call whose every argument is wrong, then the same call with the argument the message named repaired, and so
on down to the call whose only fault is that nothing lives on a HIP device.  It is written as the good arguments and a
list of steps {argument: wrong value}, in the order the checks run; rung j applies the steps from j on, the earliest step
that names an argument winning.  An argument with several checks has a step for each.  A key "self.x" (or "grid.x") is
not an argument: it sets attribute x of the object the method is called on (of the subsampling behind the segments).
"""
import json
import os

import numpy as np
import torch

from pointwise_amd import grid, prestep, provider, scene

CPU, META = torch.device("cpu"), torch.device("meta")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_mirror.json")
I32, I64, F32, F64, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8


def describe(x):
    """A result as JSON: tensors by dtype and shape, containers by their items, everything else by repr."""
    if isinstance(x, torch.Tensor):
        return {"tensor": [str(x.dtype), list(x.shape), x.device.type]}
    if isinstance(x, (tuple, list)):
        return [describe(v) for v in x]
    if isinstance(x, dict):
        return {str(k): describe(v) for k, v in x.items()}
    if x is None or isinstance(x, (bool, int, str)):
        return x
    return type(x).__name__


def outcome(thunk):
    try:
        res = thunk()
    except Exception as e:                   # the class and the message are what is pinned
        return {"raises": type(e).__name__, "message": str(e)}
    return {"returns": describe(res)}


def ladder(call, good, steps):
    rungs = []
    for j in range(len(steps) + 1):
        kw = dict(good)
        for step in reversed(steps[j:]):
            kw.update(step)
        rungs.append(outcome(lambda: call(**kw)))
    return rungs


def z(shape, dtype=F32, device=CPU):
    return torch.zeros(shape, dtype=dtype, device=device)


def method(make, name):
    """call(**kw) for a ladder over obj.name(...): a fresh object per rung, "self.x" / "grid.x" keys set attributes."""
    def call(**kw):
        obj = make()
        for key in [k for k in kw if "." in k]:
            owner, attr = key.split(".")
            setattr(obj if owner == "self" else obj._source[0], attr, kw.pop(key))
        return getattr(obj, name)(**kw)
    return call


# ---- scene --------------------------------------------------------------------------------------------------------------------

N, K = 10, 6
BIG24, BIG26 = (1 << 24) + 1, (1 << 26) + 1


def _scene_common(limit_rows):
    """The steps scene_blocks and scene_blocks_rooms share after their data (and room_start) checks."""
    dev = META
    return [{"labels": z(N)}, {"labels": z(N + 1, I32)}, {"labels": z(N, I32, dev)}, {"num_point": 0}, {"num_point": "4"},
            {"block": float("inf")}, {"block": "1"}, {"stride": -1.0}, {"stride": float("nan")}, {"block": 3.0},
            {"data": z((limit_rows, K), F32, dev), "labels": z(limit_rows, U8, dev)},
            {"data": z((1, 65537)), "labels": None}, {"min_points": 2 ** 31}, {"min_points": 1.5}, {"cover": 1},
            {"max_blocks": -1}, {"max_blocks": 2.0}, {"max_blocks": 2 ** 31}, {"seed": -1}, {"step": 2 ** 64}]


def scene_blocks_ladder(cover):
    good = dict(data=z((N, K)), labels=z(N, I32), num_point=4, block=1.0, stride=1.0, min_points=1, max_blocks=None, seed=0,
                step=0, out=None, cover=cover)
    steps = ([{"data": "x"}, {"data": z((N, K), F64)}, {"data": z(N)}, {"data": z((N, 2))}, {"data": z((K, N)).t()}]
             + _scene_common(BIG24)
             + [{"out": "x"}, {"out": scene.SceneBlocks(3, 4, K, True, CPU)}, {"out": scene.SceneBlocks(3, 4, K, True, META),
                                                                               "max_blocks": 3}])
    return ladder(scene.scene_blocks, good, steps)


def scene_rooms_ladder(host):
    dev = CPU if host else META
    good = dict(data=z((N, K), F32, dev), room_start=[0, 4, N] if host else z(3, I32, dev), labels=z(N, I32, dev),
                num_point=4, block=1.0, stride=1.0, min_points=1, max_blocks=None, seed=0, step=0, out=None, cover=True)
    steps = [{"data": "x"}, {"data": z((N, K), F64, dev)}, {"data": z((K, N), F32, dev).t()}]
    if host:
        steps += [{"room_start": z(3)}, {"room_start": [0.0, 1.0]}, {"room_start": "ab"}, {"room_start": [[0], [0, 1]]},
                  {"room_start": []}, {"room_start": [[0, 1]]}, {"room_start": np.zeros(0, np.int64)}, {"room_start": 3},
                  {"room_start": [5, 3]}, {"room_start": [-1, 3]}, {"room_start": [0, N + 1], "data": z((N, K))},
                  {"room_start": z(2, I64) + N + 1, "data": z((N, K))},
                  {"room_start": [0, BIG24], "data": z((BIG24 + 1, K), F32, META)},
                  {"room_start": np.zeros(65538, np.int32)}]
    else:
        steps += [{"room_start": z(3, I64, dev)}, {"room_start": z((3, 1), I32, dev)}, {"room_start": z(0, I32, dev)},
                  {"room_start": z(6, I32, dev)[::2]}, {"room_start": z(65538, I32, dev)}]
    common = _scene_common(BIG26)
    if host:                                  # the labels that are "on another device" are the meta ones there too
        common[10] = {"data": z((BIG26, K), F32, META), "labels": z(BIG26, U8, META), "room_start": [0, 4]}
        common[11] = dict(common[11], room_start=[0, 1])
    else:
        common[0], common[1], common[2] = {"labels": z(N, F32, dev)}, {"labels": z(N + 1, I32, dev)}, {"labels": z(N, I32)}
        common[11] = {"data": z((1, 65537), F32, dev), "labels": None, "room_start": z(2, I32, dev)}
    out_cpu = scene.SceneRoomBlocks(3, 4, K, True, CPU, 0, 2)
    steps += common + [{"out": "x"}, {"out": scene.SceneBlocks(3, 4, K, True, dev)}, {"out": out_cpu, "max_blocks": 5},
                       {"out": scene.SceneRoomBlocks(3, 4, K, True, dev, 0, 3), "max_blocks": 3}]
    return ladder(scene.scene_blocks_rooms, good, steps)


def votes_constructor(cls):
    steps = [{"num_rows": -1}, {"num_rows": 2 ** 31}, {"num_rows": 2.0}, {"num_class": 0}, {"num_class": "3"}]
    return {"ladder": ladder(cls, dict(num_rows=5, num_class=3, device="cpu"), steps),
            "bools": [outcome(lambda: cls(True, 3, "cpu")), outcome(lambda: cls(5, True, "cpu"))],
            "num_class": [outcome(lambda: cls(5, c, "cpu")) for c in (1, 128, 129, 1 << 20)]}


def _accumulator(cls, dev=CPU, rows=5):
    a = object.__new__(cls)
    a.device, a.num_rows, a.num_class, a._fresh = dev, rows, 3, True
    a.scores = z((rows, 3), I64, dev)
    return a


def votes_add():
    def call(**kw):
        a = _accumulator(scene.SceneVotes)
        return [a.add(**kw), a._fresh]
    steps = [{"pred": "x"}, {"pred": z(4, I64)}, {"pred": z(8, I32)[::2]}, {"pred": z(4, I32, META)}, {"index": None},
             {"index": z(4, F32)}, {"index": z((2, 4), I32).t()}, {"index": z(3, I32)}]
    return ladder(call, dict(pred=z(0, I32), index=z((0, 2), I32)), steps)


def scores_add():
    def call(**kw):
        a = _accumulator(scene.SceneScores)
        return [a.add(**kw), a._fresh]
    steps = [{"logits": "x"}, {"logits": z((4, 3), F64)}, {"logits": z((4, 3), F32, META)}, {"logits": z((3, 4)).t()},
             {"logits": z(())}, {"logits": z((4, 2))}, {"index": "x"}, {"index": z(4, I64)}, {"index": z(8, I32)[::2]},
             {"index": z(4, I32, META)}, {"index": z(3, I32), "logits": z((4, 3))}]
    return ladder(call, dict(logits=z((0, 3)), index=z(0, I32)), steps)


# ---- grid ---------------------------------------------------------------------------------------------------------------------

M, R = 4, 2


def _grid_common(num_class_steps):
    return ([{"data": "x"}, {"data": z((N, K), F64)}, {"data": z((N, 2))}, {"data": z((K, N)).t()}, {"labels": z(N)},
             {"labels": z(N + 1, I32)}, {"labels": z(N, I32, META)}, {"labels": z(2 * N, I32)[::2]}, {"voxel": True},
             {"voxel": "1"}, {"voxel": float("inf")}, {"voxel": 1e39}, {"voxel": 1e-50}, {"voxel": -1}, {"mode": "median"},
             {"mode": 0}] + num_class_steps
            + [{"data": z((BIG24, K), F32, META), "labels": z(BIG24, U8, META)}, {"data": z((1, 65537)), "labels": z(1, I64)},
               {"max_voxels": -1}, {"max_voxels": True}, {"max_voxels": 2 ** 31}, {"max_voxels": 2.0}])


def grid_subsample_ladder(mode):
    good = dict(data=z((N, K)), labels=z(N, I32), voxel=0.5, mode=mode, num_class=3 if mode == "mean" else None,
                max_voxels=None, out=None)
    ncs = ([{"num_class": None}, {"num_class": 0}, {"num_class": 129}, {"num_class": True}] if mode == "mean" else
           [{"num_class": "3"}, {"num_class": True}, {"num_class": 2.0}])
    steps = _grid_common(ncs) + [{"out": "x"}, {"out": grid.GridSubsample(N, M, K, True, CPU)},
                                 {"out": grid.GridSubsample(N, M, K, True, META), "max_voxels": M}]
    return ladder(grid.grid_subsample, good, steps)


def grid_rooms_ladder(mode):
    good = dict(data=z((N, K)), room_start=z(R + 1, I32), labels=z(N, I32), voxel=0.5, mode=mode,
                num_class=3 if mode == "mean" else None, max_voxels=None, out=None)
    ncs = ([{"num_class": None}, {"num_class": 0}, {"num_class": 129}, {"num_class": True}] if mode == "mean" else
           [{"num_class": "3"}, {"num_class": True}, {"num_class": 2.0}])
    steps = _grid_common(ncs) + [{"room_start": [0, 4, N]}, {"room_start": z(3, I64)}, {"room_start": z((3, 1), I32)},
                                 {"room_start": z(0, I32)}, {"room_start": z(6, I32)[::2]}, {"room_start": z(3, I32, META)},
                                 {"room_start": z(65538, I32)}, {"out": "x"}, {"out": grid.GridSubsample(N, N, K, True, CPU)},
                                 {"out": grid.GridRoomSubsample(N, R + 1, N, K, True, CPU)},
                                 {"out": grid.GridRoomSubsample(N, R, M, K, True, META), "max_voxels": M}]
    return ladder(grid.grid_subsample_rooms, good, steps)


def make_grid(rooms, dev=CPU):
    def make():
        g = grid.GridRoomSubsample(N, R, M, K, True, dev) if rooms else grid.GridSubsample(N, M, K, True, dev)
        g.stats.zero_()
        return g
    return make


def _table_steps(rooms, first_axis=M):
    """Steps over the tensors of the subsampling that neighbors / the ring path of interpolate read."""
    steps = [{"self.voxel_cell": z((first_axis, 3), I64)}, {"self.voxel_cell": z((first_axis, 2), I32)},
             {"self.voxel_cell": z((3, first_axis), I32).t()}, {"self.stats": "x"}, {"self.stats": z(7, I32)},
             {"self.stats": z(8, I32, META)}]
    if rooms:
        steps += [{"self.voxel_room": z(first_axis, I64)}, {"self.voxel_room": z(first_axis + 1, I32)},
                  {"self.voxel_start": z(R + 1, I64)}, {"self.voxel_start": z(2 * R + 2, I32)[::2]}]
    return steps


def project_ladder(rooms):
    steps = [{"voxel_labels": "x"}, {"voxel_labels": z(M, I64)}, {"voxel_labels": z((M, 1), I32)},
             {"voxel_labels": z(M, I32, META)}, {"voxel_labels": z(2 * M, I32)[::2]}, {"out": "x"}, {"out": z(N, I64)},
             {"out": z(N + 1, I32)}, {"out": z(N, I32, META)}, {"out": z(2 * N, I32)[::2]}]
    return ladder(method(make_grid(rooms), "project"), dict(voxel_labels=z(M, I32), out=None), steps)


def neighbors_ladder(rooms):
    res = {"ladder": ladder(method(make_grid(rooms), "neighbors"), {}, _table_steps(rooms))}
    if rooms:                                 # a voxel_start that is no vector: checked by one caller, not by the other
        res["voxel_start_2d"] = outcome(lambda: method(make_grid(True), "neighbors")(**{"self.voxel_start": z((R + 1, 1), I32)}))
        res["voxel_start_empty"] = outcome(lambda: method(make_grid(True), "neighbors")(**{"self.voxel_start": z(0, I32)}))
    return res


def _scores_object(dev=CPU, rows=M):
    return _accumulator(scene.SceneScores, dev, rows)


def interpolate_ladder(rooms, ringed, with_out, i64=False):
    C = 3
    flags = dict(rings=2, return_ring=True) if ringed else dict(rings=1, return_ring=False)
    parts = 3 if ringed else 2
    out = (z(N, I32), z((N, C)), z(N, I32))[:parts] if with_out else None
    good = dict(data=z((N, K)), voxel_scores=_scores_object() if i64 else z((M, C)), k=3, valid_labels=z(M, I32),
                return_scores=True, out=out, **flags)
    steps = [{"data": "x"}, {"data": z((N, K), F64)}, {"data": z((N, 2))}, {"data": z((K, N)).t()}, {"data": z((N, K), F32, META)},
             {"data": z((N + 1, K))}, {"k": 0}, {"k": 9}, {"k": True}, {"k": 3.0}, {"voxel_scores": "x"},
             {"voxel_scores": _scores_object(META)}, {"voxel_scores": z((M, C), F64)}, {"voxel_scores": z(M)},
             {"voxel_scores": z((C, M)).t()}, {"voxel_scores": z((M, C), F32, META)}, {"voxel_scores": z((M, 0))},
             {"voxel_scores": z((M, 129))}, {"voxel_scores": z((M + 1, C)), "valid_labels": z(M + 1, I32)},
             {"voxel_scores": _scores_object(CPU, M + 1), "valid_labels": None}, {"valid_labels": "x"},
             {"valid_labels": z(M, I64)}, {"valid_labels": z(M - 1, I32)}, {"valid_labels": z(M, I32, META)},
             {"valid_labels": z(2 * M, I32)[::2]}, {"rings": 0}, {"rings": 9}, {"rings": True}, {"return_ring": 1},
             {"out": z(N, I32)}, {"out": (z(N, I32),) * (parts + 1)},
             {"out": [z(N, I64), z((N, C)), z(N, I32)][:parts]}, {"out": [z(N + 1, I32), z((N, C)), z(N, I32)][:parts]},
             {"out": [z(N, I32), z((N, C), F64), z(N, I32)][:parts]}, {"out": [z(N, I32), z((N, C + 1)), z(N, I32)][:parts]},
             {"out": [z(N, I32), "x", z(N, I32)][:parts]}]
    if ringed:
        steps += [{"out": [z(N, I32), z((N, C)), z(N, I64)]}, {"out": [z(N, I32), z((N, C)), z(2 * N, I32)[::2]]}]
        steps += _table_steps(rooms)
        if rooms:
            steps += [{"self.voxel_start": z((R + 1, 1), I32)}, {"self.voxel_start": z(0, I32)}]
    return ladder(method(make_grid(rooms), "interpolate"), good, steps)


def interpolate_out_shapes(rooms):
    """The two messages of a malformed out=, by the flags that choose between them."""
    call = method(make_grid(rooms), "interpolate")
    base = dict(data=z((N, K)), voxel_scores=z((M, 3)))
    return [outcome(lambda: call(out=z(N, I32), return_scores=rs, return_ring=rr, **base))
            for rs in (False, True, 1) for rr in (False, True)]


def normals_ladder(rooms):
    steps = [{"min_neighbors": 2}, {"min_neighbors": 28}, {"min_neighbors": True}, {"return_moments": 1}, {"viewpoint": "abc"},
             {"viewpoint": 3}, {"viewpoint": (1, 2)}, {"viewpoint": (float("inf"), 0, 0)}, {"viewpoint": (1e39, 0, 0)},
             {"viewpoint": z((1, 3), F64)}, {"viewpoint": z(3)}, {"viewpoint": z((1, 4))}, {"viewpoint": z((0, 3))},
             {"viewpoint": z((3, 2)).t()}, {"viewpoint": z((1, 3), F32, META)}, {"viewpoint": z((R + 1, 3))},
             {"self.data": z((M, K), F64)}, {"self.data": z((M, 2))}, {"self.data": z((K, M)).t()}]
    if rooms:
        steps += [{"self.voxel_room": "x"}, {"self.voxel_room": z(M, I64)}, {"self.voxel_room": z(M + 1, I32)},
                  {"self.voxel_room": z(M, I32, META)}]
    steps += [{"out": "x"}, {"out": grid.GridNormals(M, False, CPU)}, {"out": grid.GridNormals(M + 1, True, CPU)},
              {"out": grid.GridNormals(M, True, META)}]
    good = dict(viewpoint=z((R, 3)) if rooms else (0.0, 1, 2), min_neighbors=6, return_moments=True, out=None)
    return ladder(method(make_grid(rooms), "normals"), good, steps)


def with_normals_ladder(rooms):
    steps = [{"nrm": "x"}, {"nrm": grid.GridNormals(M + 1, False, CPU)}, {"nrm": grid.GridNormals(M, False, META)},
             {"curvature": 1}]
    call = method(make_grid(rooms), "with_normals")
    return ladder(call, dict(nrm=grid.GridNormals(M, False, CPU), curvature=True), steps) + [
        outcome(lambda: call(nrm=grid.GridNormals(M, True, CPU)))]


def _segment_steps(labelled):
    if labelled:
        steps = [{"voxel_labels": "x"}, {"voxel_labels": z(M, I64)}, {"voxel_labels": z((M, 1), I32)},
                 {"voxel_labels": z(M, I32, META)}, {"voxel_labels": z(2 * M, I32)[::2]}, {"voxel_labels": z(M + 1, I32)},
                 {"num_class": None}, {"num_class": 0}, {"num_class": 129}, {"num_class": True}]
    else:
        steps = [{"num_class": "3"}, {"num_class": 0}, {"num_class": 129}, {"num_class": True}]
    return steps + [{"connectivity": 7}, {"connectivity": True}, {"connectivity": 26.0}, {"self.voxel_count": z(M, I64)},
                    {"self.voxel_count": z(2 * M, I32)[::2]}, {"self.voxel_cell": z((M, 2), I32)}, {"out": "x"},
                    {"out": grid.GridSegments(M + 1, CPU)}, {"out": grid.GridSegments(M, META)}]


def segments_ladder(rooms, labelled):
    good = dict(voxel_labels=z(M - 1, I32) if labelled else None, num_class=3 if labelled else None, connectivity=18, out=None)
    return ladder(method(make_grid(rooms), "segments"), good, _segment_steps(labelled))


def clean_labels_ladder(rooms):
    good = dict(voxel_labels=z(M, I32), num_class=3, min_size=2, connectivity=6, drop_orphans=True)
    steps = [{"min_size": 0}, {"min_size": True}, {"min_size": 2 ** 31}, {"min_size": 2.0}, {"drop_orphans": 0}]
    return ladder(method(make_grid(rooms), "clean_labels"), good, steps + _segment_steps(True)[:-3])


def make_segments(rooms, labelled=True):
    def make():
        s = grid.GridSegments(M, CPU)
        s.stats.zero_()
        s._source = (make_grid(rooms)(), z(M, I32) if labelled else None, M if labelled else 0, 3 if labelled else 1, 26)
        return s
    return make


def absorb_ladder(rooms):
    steps = [{"min_size": 0}, {"min_size": True}, {"min_size": 2 ** 31}, {"drop_orphans": None}, {"self._source": None},
             {"out": "x"}, {"out": z(M, I64)}, {"out": z(M + 1, I32)}, {"out": z(M, I32, META)}, {"out": z(2 * M, I32)[::2]}]
    good = dict(min_size=2, drop_orphans=False, out=None)
    return {"ladder": ladder(method(make_segments(rooms), "absorb"), good, steps),
            "with_out": outcome(lambda: method(make_segments(rooms), "absorb")(min_size=1, out=z(M, I32))),
            "on_trim": outcome(lambda: make_segments(rooms)().trim().absorb(2))}


def geometry_ladder(rooms):
    steps = [{"weight": "cells"}, {"weight": 0}, {"self._source": None}, {"grid.data": "x"}, {"grid.data": z((M, K), F64)},
             {"grid.data": z(M)}, {"grid.data": z((M + 1, K))}, {"grid.data": z((M, 2))}, {"grid.data": z((M, 65537))},
             {"grid.data": z((K, M)).t()}, {"grid.data": z((M, K), F32, META)}, {"grid.voxel_cell": "x"},
             {"grid.voxel_cell": z((M, 3), I64)}, {"grid.voxel_cell": z((M, 2), I32)}, {"grid.voxel_count": z(M + 1, I32)},
             {"grid.voxel_count": z(M, I32, META)}, {"grid.stats": z(4, I32)}, {"self.segment": z(M + 1, I32)},
             {"self.segment": z(2 * M, I32)[::2]}, {"self.stats": z(4, I32)}, {"out": "x"},
             {"out": grid.SegmentGeometry(M + 1, CPU)}, {"out": grid.SegmentGeometry(M, META)}]
    return {"ladder": ladder(method(make_segments(rooms), "geometry"), dict(weight="rows", out=None), steps),
            "on_trim": outcome(lambda: make_segments(rooms)().trim().geometry())}


# ---- provider and prestep -----------------------------------------------------------------------------------------------------

S, NSRC = 5, 8


def assemble_ladder():
    good = dict(data=z((S, NSRC, 3)), labels=z(S, U8), batch_size=2, num_points=4, perm=z(S, I32), start=1, rotate=True,
                jitter=True, sigma=0.01, clip=0.05, sort_cloud=True, seed=0, step=0, cos_sin=z((2, 2), F64),
                noise=z((2, 4, 3), F64), sort_method="morton", wide_sort=True)
    steps = [{"sort_method": "zyx"}, {"sort_method": None}, {"data": "x"}, {"data": z((S, NSRC, 3), F64)}, {"data": z((S, NSRC))},
             {"data": z((S, NSRC, 2))}, {"labels": "x"}, {"labels": z(S)},
             {"data": z(((1 << 31), 1, 3), F32, META), "labels": z(1, U8, META)}, {"labels": z(S, U8, META)},
             {"labels": z(S + 1, U8)}, {"labels": z((S, NSRC, 1), I32)}, {"data": z((3, NSRC, S)).permute(2, 1, 0)},
             {"labels": z((NSRC, S), I64).t()}, {"batch_size": -1}, {"num_points": NSRC + 1}, {"num_points": -1}, {"start": -1},
             {"perm": "x"}, {"perm": z(S, I64)}, {"perm": z((S, 1), I32)}, {"perm": z(S, I32, META)}, {"perm": z(2 * S, I32)[::2]},
             {"start": S - 1}, {"seed": -1}, {"step": 2 ** 64}, {"clip": 0.0}, {"sigma": -1.0},
             {"cos_sin": z((2, 2), F64), "rotate": False}, {"cos_sin": z((2, 2))}, {"cos_sin": z((3, 2), F64)},
             {"noise": z((2, 4, 3), F64), "jitter": False}, {"noise": z((2, 4, 2), F64)}, {"noise": z((2, 4, 3), F64, META)}]
    return {"ladder": ladder(provider.assemble_batch, good, steps),
            "start_without_perm": outcome(lambda: provider.assemble_batch(z((S, NSRC, 3)), z(S, U8), 2, start=2 ** 31 - 2)),
            "provider_method": outcome(lambda: provider.BatchProvider(z((S, NSRC, 3)), z(S, U8), 2, device="cpu",
                                                                      sort_method="hilbert"))}


def sort_methods():
    res = {}
    for mod in (provider, prestep):
        res[mod.__name__.split(".")[-1]] = {
            "methods": [str(m) for m in mod.SORT_METHODS],
            "checks": [outcome(lambda: mod._check_sort_method(m)) for m in ("xyz", "morton", "zyx", "XYZ", None, 0, ["xyz"])]}
    res["sort_order"] = ladder(prestep.sort_order, dict(batch_data=z((2, 8, 3)), sort_method="morton"),
                               [{"sort_method": "zyx"}, {"sort_method": ("xyz",)}])
    return res


# ---- views --------------------------------------------------------------------------------------------------------------------

def _fill(obj, **values):
    """Give every tensor of the object defined contents, then the words a view reads."""
    for name, t in vars(obj).items():
        if isinstance(t, torch.Tensor):
            t.zero_()
    for name, v in values.items():
        getattr(obj, name).copy_(torch.tensor(v, dtype=getattr(obj, name).dtype))
    return obj


def view_of(parent, view):
    """Every attribute of the view or of its parent, as the view has it: its type, and for a tensor its shape and whether
    it IS one of the parent's tensors or views one, from which storage offset.  An attribute the view does not have reads
    as None: that is how the package reads them (getattr(self, "_neigh", None))."""
    owners = {n: t for n, t in vars(parent).items() if isinstance(t, torch.Tensor)}
    res = {"class": type(view).__name__}
    for name in sorted(set(vars(view)) | set(vars(parent))):
        v = getattr(view, name, None)
        if not isinstance(v, torch.Tensor):
            res[name] = describe(v)
            continue
        same = [n for n, t in owners.items() if t is v]
        views = [n for n, t in owners.items() if t.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()]
        res[name] = {"shape": list(v.shape), "dtype": str(v.dtype), "is": sorted(same), "views": sorted(views),
                     "offset": v.storage_offset(), "stride": list(v.stride())}
    return res


def views():
    res = {}
    for labels in (True, False):
        tag = "labels" if labels else "plain"
        g = _fill(grid.GridSubsample(N, M, K, labels, CPU), stats=[2, 3, 0, 0, 0, 0, 0, 0])
        res["GridSubsample.trim/" + tag] = view_of(g, g.trim())
        g._neigh = z((M, 27), I32)
        res["GridSubsample.trim/neigh/" + tag] = view_of(g, g.trim())
        g._neigh = None
        res["GridSubsample.trim/neigh-none/" + tag] = view_of(g, g.trim())
        gr = _fill(grid.GridRoomSubsample(N, R, M, K, labels, CPU), stats=[3, 3, R, 0, 0, 0, 0, 0], voxel_start=[0, 1, 3])
        res["GridRoomSubsample.trim/" + tag] = view_of(gr, gr.trim())
        res["GridRoomSubsample.room/" + tag] = [view_of(gr, gr.room(r)) for r in range(R)]
        gr._neigh = z((M, 27), I32)
        res["GridRoomSubsample.trim/neigh/" + tag] = view_of(gr, gr.trim())
        res["GridRoomSubsample.room/neigh/" + tag] = view_of(gr, gr.room(1))
        res["GridRoomSubsample.trim.room/" + tag] = view_of(gr, gr.trim().room(1))
        sb = _fill(scene.SceneBlocks(M, 3, K, labels, CPU, 64), stats=[2, 2, 1, 1, 0, 0, 5, 0])
        res["SceneBlocks.trim/" + tag] = view_of(sb, sb.trim())
        res["SceneBlocks.needed/" + tag] = [sb.num_blocks(), sb.blocks_needed(), list(sb.trim().shape), list(sb.trim().points.shape)]
        sr = _fill(scene.SceneRoomBlocks(M, 3, K, labels, CPU, 64, R), stats=[3, 3, R, 2, 0, 0, 0, 0], room_blocks=[0, 2, 3])
        sr.room_start = z(R + 1, I32)
        res["SceneRoomBlocks.trim/" + tag] = view_of(sr, sr.trim())
        res["SceneRoomBlocks.room/" + tag] = [view_of(sr, sr.room(r)) for r in range(R)]
        res["SceneRoomBlocks.cache/" + tag] = describe(sr._room_blocks_host)
        res["SceneRoomBlocks.trim-after-room/" + tag] = view_of(sr, sr.trim())
        res["SceneRoomBlocks.trim.room/" + tag] = view_of(sr, sr.trim().room(0))
    res["GridRoomSubsample.room/r"] = [outcome(lambda: gr.room(r)) for r in (True, -1, R, 1.0, "0")]
    res["SceneRoomBlocks.room/r"] = [outcome(lambda: sr.room(r)) for r in (True, False, -1, R, 1.0, "0")]
    seg = _fill(make_segments(False)(), stats=[2, 4, 0, 0, 3, 3, 0, 0])
    res["GridSegments.trim"] = view_of(seg, seg.trim())
    seg.absorbed_label, seg.absorb_stats, seg._absorb_workspace = z(M, I32), z(4, I64), z(16, U8)
    seg.workspace = z(16, U8)
    res["GridSegments.trim/absorbed"] = view_of(seg, seg.trim())
    geo = _fill(grid.SegmentGeometry(M, CPU), stats=[3, 1, 0, 0])
    res["SegmentGeometry.trim"] = view_of(geo, geo.trim())
    return res


# ---- host-only arithmetic -----------------------------------------------------------------------------------------------------

def arithmetic():
    res = {"default_max_blocks": [], "default_max_blocks_rooms": [], "_rooms_bound": []}
    for block, stride in ((1.0, 1.0), (1.0, 0.5), (1.5, 1.0), (2, 1)):
        for min_points in (-5, 0, 1, 100):
            for num_point in (None, 1, 4096):
                args = (block, stride, min_points, num_point)
                res["default_max_blocks"].append([scene.default_max_blocks(n, *args) for n in (0, 1, 99, 4096, 10 ** 6, 1 << 24)])
                res["default_max_blocks_rooms"].append([scene.default_max_blocks_rooms(rooms, *args) for rooms in
                                                        ((), (0,), (0, 5, 0), (100, 4096, 7), (10 ** 6,) * 3)])
                res["_rooms_bound"].append([scene._rooms_bound(n, r, *args) for n in (0, 1, 4096, 1 << 26)
                                            for r in (0, 1, 3, 65536)])
    return res


TABLE = {"arithmetic": arithmetic, "views": views, "sort_methods": sort_methods, "assemble_batch": assemble_ladder,
         "SceneVotes": lambda: votes_constructor(scene.SceneVotes), "SceneScores": lambda: votes_constructor(scene.SceneScores),
         "SceneVotes.add": votes_add, "SceneScores.add": scores_add}
for _cover in (False, True):
    TABLE["scene_blocks/cover=%s" % _cover] = lambda c=_cover: scene_blocks_ladder(c)
for _host in (False, True):
    TABLE["scene_blocks_rooms/%s" % ("host" if _host else "device")] = lambda h=_host: scene_rooms_ladder(h)
for _mode in ("mean", "center"):
    TABLE["grid_subsample/" + _mode] = lambda m=_mode: grid_subsample_ladder(m)
    TABLE["grid_subsample_rooms/" + _mode] = lambda m=_mode: grid_rooms_ladder(m)
for _rooms in (False, True):
    _tag = "/rooms" if _rooms else "/single"
    TABLE["project" + _tag] = lambda r=_rooms: project_ladder(r)
    TABLE["neighbors" + _tag] = lambda r=_rooms: neighbors_ladder(r)
    for _ringed in (False, True):
        for _out in (False, True):
            TABLE["interpolate%s/%s/%s" % (_tag, "rings" if _ringed else "plain", "out" if _out else "fresh")] = \
                lambda r=_rooms, g=_ringed, o=_out: interpolate_ladder(r, g, o)
    TABLE["interpolate%s/scores-object" % _tag] = lambda r=_rooms: interpolate_ladder(r, True, False, i64=True)
    TABLE["interpolate%s/out-shapes" % _tag] = lambda r=_rooms: interpolate_out_shapes(r)
    TABLE["normals" + _tag] = lambda r=_rooms: normals_ladder(r)
    TABLE["with_normals" + _tag] = lambda r=_rooms: with_normals_ladder(r)
    TABLE["segments%s/labels" % _tag] = lambda r=_rooms: segments_ladder(r, True)
    TABLE["segments%s/geometric" % _tag] = lambda r=_rooms: segments_ladder(r, False)
    TABLE["clean_labels" + _tag] = lambda r=_rooms: clean_labels_ladder(r)
    TABLE["absorb" + _tag] = lambda r=_rooms: absorb_ladder(r)
    TABLE["geometry" + _tag] = lambda r=_rooms: geometry_ladder(r)


def count(x):
    """The number of outcomes in a recorded entry."""
    if isinstance(x, dict):
        return 1 if "raises" in x or "returns" in x else sum(count(v) for v in x.values())
    return sum(count(v) for v in x) if isinstance(x, list) else 0


def record():
    return {name: thunk() for name, thunk in sorted(TABLE.items())}


if __name__ == "__main__":
    table = record()
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries, %d recorded outcomes -> %s" % (len(table), sum(count(v) for v in table.values()), GOLDEN))
