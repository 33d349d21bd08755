"""A raw room through the whole path (-m gpu): a synthetic room -> grid_subsample (mean, majority labels) ->
scene_blocks(cover=True, min_points=1) on the voxel rows -> SceneVotes fed the blocks' own labels as the predictions ->
labels() -> GridSubsample.project.  Every finite raw row must come out with the majority label of its voxel as
tests/grid_ref.py computes it."""
import numpy as np
import pytest

from tests import grid_ref as gr

NCLS, P, VOXEL = 13, 64, 0.08


def raw_room():
    from pointwise_amd import synth
    N = 4000
    rng = np.random.default_rng(4100)
    xyz = synth.room_like(1, N, 4101, (3.2, 2.4, 3.0))[0]
    data = np.concatenate([xyz, rng.random((N, 3))], axis=1).astype(np.float32)
    labels = rng.integers(0, NCLS, size=N).astype(np.int32)
    labels[::5] = -1                                     # unlabelled rows: some voxels have no valid label at all
    data[17, 0], data[2500, 2] = np.nan, np.inf
    return data, labels


@pytest.mark.gpu
def test_raw_room_to_voxels_to_covering_blocks_to_votes_and_back_to_every_row():
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data, labels = raw_room()
    N = data.shape[0]
    want = gr.grid_subsample_ref(data, labels, voxel=VOXEL, mode="mean", num_class=NCLS)
    V = int(want["stats"][0])
    assert 500 < V < N and int(want["stats"][5]) == 2 and (want["labels"][:V] == -1).any() and int(want["stats"][6]) > 1
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), torch.from_numpy(labels).to(dev), voxel=VOXEL, num_class=NCLS)
    assert g.num_voxels() == V
    g = g.trim()
    assert np.array_equal(g.data.cpu().numpy().view(np.uint32), want["data"][:V].view(np.uint32))
    assert np.array_equal(g.labels.cpu().numpy(), want["labels"][:V])
    sb = scene.scene_blocks(g.data, g.labels, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True)
    assert sb.num_blocks() == sb.blocks_needed() and int(sb.stats[7]) == 0 and int(sb.stats[4]) == 0
    sb = sb.trim()
    votes = scene.SceneVotes(V, NCLS, dev)
    votes.add(sb.labels.contiguous(), sb.index.contiguous())                 # the blocks' own labels as the predictions
    voxel_pred = votes.labels()
    assert np.array_equal(voxel_pred.cpu().numpy(), want["labels"][:V])       # every voxel row was emitted and voted
    got = g.project(voxel_pred).cpu().numpy()
    fin = np.isfinite(data[:, :3]).all(axis=1)
    assert np.array_equal(got[fin], want["labels"][want["inverse"][fin]]) and (want["inverse"][fin] >= 0).all()
    assert (got[~fin] == -1).all() and np.array_equal(got, gr.project_ref(want["labels"][:V], want["inverse"]))
    assert (got[fin] >= 0).sum() > 0.8 * fin.sum()                            # a fifth of the rows is unlabelled
