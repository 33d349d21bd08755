"""GPU test of the nothing-to-launch paths of grid_subsample, grid_subsample_rooms, scene_blocks and scene_blocks_rooms: no
rows, no capacity or no rooms.  They run behind the device check, so tests/test_host_mirror_host.py cannot reach them;
nothing is launched there and the host fills the outputs with what the classes' docstrings state for the entries past the
emitted ones (data 0, labels -1, index / voxel_row / cells -1, counts 0, voxel_room / block_room -1, the prefixes and
stats 0).  Every case runs into fresh outputs and into an `out` whose every word was 7 before."""
import pytest
import torch

from pointwise_amd import grid, scene

pytestmark = pytest.mark.gpu
K, P = 6, 3
FILL = {"data": 0, "labels": -1, "inverse": -1, "index": -1, "voxel_row": -1, "voxel_cell": -1, "block_cell": -1,
        "voxel_count": 0, "block_count": 0, "voxel_room": -1, "block_room": -1, "voxel_start": 0, "room_blocks": 0,
        "room_stats": 0, "stats": 0}
CASES = {"no rows": (0, 3, 2), "no capacity": (5, 0, 2), "no rooms": (5, 4, 0)}            # N, max_voxels / max_blocks, R
CALLS = [(case, rooms) for case in sorted(CASES) for rooms in (False, True) if rooms or case != "no rooms"]


def _dirty(obj):
    for t in vars(obj).values():
        if isinstance(t, torch.Tensor):
            t.fill_(7)
    return obj


def _check(res, cls, fields, shapes):
    assert type(res) is cls
    for name in fields:
        t = getattr(res, name)
        assert tuple(t.shape) == shapes[name], name
        assert bool((t == FILL[name]).all()), name


@pytest.mark.parametrize("case,rooms", CALLS)
def test_grid_subsample_with_nothing_to_launch(case, rooms):
    N, M, R = CASES[case]
    dev = torch.device("cuda:0")
    data = torch.rand((N, K), device=dev)
    labels = torch.zeros((N,), dtype=torch.int32, device=dev)
    start = torch.tensor([0] + [N] * R, dtype=torch.int32, device=dev)
    shapes = {"data": (M, K), "labels": (M,), "inverse": (N,), "voxel_row": (M,), "voxel_count": (M,), "voxel_cell": (M, 3),
              "stats": (8,), "voxel_room": (M,), "voxel_start": (R + 1,), "room_stats": (R, 8)}
    fields = ["data", "labels", "inverse", "voxel_row", "voxel_count", "voxel_cell", "stats"]
    if rooms:
        fields += ["voxel_room", "voxel_start", "room_stats"]
        call = lambda out: grid.grid_subsample_rooms(data, start, labels, 0.5, "mean", 3, M, out)
        cls, dirty = grid.GridRoomSubsample, grid.GridRoomSubsample(N, R, M, K, True, dev)
    else:
        call = lambda out: grid.grid_subsample(data, labels, 0.5, "mean", 3, M, out)
        cls, dirty = grid.GridSubsample, grid.GridSubsample(N, M, K, True, dev)
    _check(call(None), cls, fields, shapes)
    dirty._neigh = torch.zeros((M, 27), dtype=torch.int32, device=dev)
    res = call(_dirty(dirty))
    assert res is dirty and res._neigh is None
    _check(res, cls, fields, shapes)


@pytest.mark.parametrize("cover", (False, True))
@pytest.mark.parametrize("case,rooms", CALLS)
def test_scene_blocks_with_nothing_to_launch(case, rooms, cover):
    N, B, R = CASES[case]
    dev = torch.device("cuda:0")
    data = torch.rand((N, K), device=dev)
    labels = torch.zeros((N,), dtype=torch.int64, device=dev)
    shapes = {"data": (B, P, K + 3), "labels": (B, P), "index": (B, P), "block_cell": (B,), "block_count": (B,), "stats": (8,),
              "block_room": (B,), "room_blocks": (R + 1,), "room_stats": (R, 8)}
    fields = ["data", "labels", "index", "block_cell", "block_count", "stats"]
    if rooms:
        fields += ["block_room", "room_blocks", "room_stats"]
        start = torch.tensor([0] + [N] * R, dtype=torch.int32, device=dev)
        call = lambda out: scene.scene_blocks_rooms(data, start, labels, P, 1.0, 1.0, 1, B, out=out, cover=cover)
        cls, dirty = scene.SceneRoomBlocks, scene.SceneRoomBlocks(B, P, K, True, dev, 0, R)
        dirty._room_blocks_host = [0] * (R + 1)
    else:
        call = lambda out: scene.scene_blocks(data, labels, P, 1.0, 1.0, 1, B, out=out, cover=cover)
        cls, dirty = scene.SceneBlocks, scene.SceneBlocks(B, P, K, True, dev)
    _check(call(None), cls, fields, shapes)
    res = call(_dirty(dirty))
    assert res is dirty
    _check(res, cls, fields, shapes)
    if rooms:
        assert res.room_start is start and res._room_blocks_host is None
        host = scene.scene_blocks_rooms(data, [0] + [N] * R, labels, P, 1.0, 1.0, 1, B, cover=cover)
        _check(host, cls, fields, shapes)
        assert host.room_start.dtype == torch.int32 and host.room_start.tolist() == [0] + [N] * R
