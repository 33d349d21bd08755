"""Three raw rooms through the whole path in single calls (-m gpu): grid_subsample_rooms (mean, majority labels) ->
scene_blocks_rooms(g.data, g.voxel_start, g.labels, cover=True, min_points=1) on the untrimmed voxel rows, voxel_start
used as it stands on the device -> SceneVotes over the global voxel numbers, fed the blocks' own labels as the
predictions -> labels() -> project.  Every finite raw row of every room must come out with the majority label of its own
room's voxel as tests/grid_rooms_ref.py computes it, every non-finite row as -1."""
import numpy as np
import pytest

from tests import grid_ref as gr
from tests import grid_rooms_ref as grr

NCLS, P, VOXEL = 13, 64, 0.08
SIZES = (3000, 2800, 3100)


def raw_rooms():
    from pointwise_amd import synth
    rng = np.random.default_rng(4200)
    parts = []
    for k, n in enumerate(SIZES):                        # the rooms overlap in space: each starts at its own origin
        xyz = synth.room_like(1, n, 4201 + k, (3.2 - 0.4 * k, 2.4 + 0.3 * k, 3.0))[0]
        parts.append(np.concatenate([xyz, rng.random((n, 3))], axis=1).astype(np.float32))
    data = np.concatenate(parts)
    N = data.shape[0]
    labels = rng.integers(0, NCLS, size=N).astype(np.int32)
    labels[::5] = -1                                     # unlabelled rows: some voxels have no valid label at all
    data[17, 0], data[2500, 2], data[3000, 1], data[8899, 0] = np.nan, np.inf, -np.inf, np.nan
    return data, labels, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)


@pytest.mark.gpu
def test_raw_rooms_to_voxels_to_covering_blocks_to_votes_and_back_to_every_row():
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data, labels, start = raw_rooms()
    N, R = data.shape[0], len(SIZES)
    want = grr.grid_subsample_rooms_ref(data, start, labels, voxel=VOXEL, mode="mean", num_class=NCLS)
    V = int(want["stats"][0])
    assert 1500 < V < N and int(want["stats"][5]) == 4 and (want["labels"][:V] == -1).any() and int(want["stats"][6]) > 1
    assert want["stats"][[2, 3, 4, 7]].tolist() == [R, R, 0, 0] and want["room_stats"][:, 0].min() > 500
    g = grid.grid_subsample_rooms(torch.from_numpy(data).to(dev), torch.from_numpy(start).to(dev),
                                  torch.from_numpy(labels).to(dev), voxel=VOXEL, num_class=NCLS)
    assert np.array_equal(g.data.cpu().numpy().view(np.uint32), want["data"].view(np.uint32))
    assert np.array_equal(g.labels.cpu().numpy(), want["labels"]) and np.array_equal(g.voxel_start.cpu().numpy(), want["voxel_start"])
    # the untrimmed rows and the device's voxel_start go straight into the tiling: rows from voxel_start[R] on are in no room
    sb = scene.scene_blocks_rooms(g.data, g.voxel_start, g.labels, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True,
                                  max_blocks=2048)
    assert sb.room_start is g.voxel_start
    assert sb.num_blocks() == sb.blocks_needed() < 2048 and int(sb.stats[7]) == 0 and int(sb.stats[4]) == 0 and int(sb.stats[2]) == R
    sb = sb.trim()
    rooms_of_rows = want["voxel_room"][sb.index.cpu().numpy()]               # index: the global voxel number of every row
    assert np.array_equal(rooms_of_rows, np.broadcast_to(sb.block_room.cpu().numpy()[:, None], rooms_of_rows.shape))
    assert g.num_voxels() == V                                               # the one host read of the grid stage
    votes = scene.SceneVotes(V, NCLS, dev)
    votes.add(sb.labels.contiguous(), sb.index.contiguous())                 # the blocks' own labels as the predictions
    voxel_pred = votes.labels()
    assert np.array_equal(voxel_pred.cpu().numpy(), want["labels"][:V])       # every voxel row was emitted and voted
    got = g.project(voxel_pred).cpu().numpy()                                # one projection serves every room
    fin = np.isfinite(data[:, :3]).all(axis=1)
    inv = want["inverse"]
    assert (inv[fin] >= 0).all() and np.array_equal(got[fin], want["labels"][inv[fin]])
    room_of_row = np.repeat(np.arange(R), SIZES)
    assert np.array_equal(want["voxel_room"][inv[fin]], room_of_row[fin])     # its own room's voxel
    assert (got[~fin] == -1).all() and np.array_equal(got, gr.project_ref(want["labels"][:V], inv))
    assert (got[fin] >= 0).sum() > 0.8 * fin.sum()                            # a fifth of the rows is unlabelled
    for r in range(R):                                                       # and per room: the single call's majority labels
        a, b = int(start[r]), int(start[r + 1])
        one = gr.grid_subsample_ref(data[a:b], labels[a:b], voxel=VOXEL, mode="mean", num_class=NCLS)
        assert np.array_equal(got[a:b], gr.project_ref(one["labels"][:int(one["stats"][0])], one["inverse"]))
