"""A raw room through the whole path with both endings (-m gpu): grid_subsample (mean, majority labels) -> the plain
scene_blocks on the voxel rows, whose min_points drops the sparse cells and whose num_point samples the crowded ones ->
SceneScores fed one-hot logits of the blocks' own labels -> project(scores.labels()) and interpolate(room, scores).

Which voxels are voted for is the tiling's, so the numpy references alone give the counts: of the 2998 finite rows project
leaves 971 at -1 (32 %; at least 10 % is the condition on the input), and interpolate, k = 3, labels 544 of those (56 %;
at least a quarter) -- their own voxel has no vote, a voxel of a neighbouring cell has.  The 427 rows left have no voted
voxel in their 27 cells."""
import numpy as np
import pytest

from tests import grid_interp_ref as gi
from tests import grid_ref as gr
from tests import scene_ref as sr

NCLS, N, VOXEL = 13, 3000, 0.08
TILING = dict(num_point=256, block=1.0, stride=1.0, min_points=150, max_blocks=64)
FINITE, PROJECTED, INTERPOLATED = 2998, 2027, 2571


def raw_room():
    from pointwise_amd import synth
    rng = np.random.default_rng(4300)
    xyz = synth.room_like(1, N, 4301, (3.2, 2.4, 3.0))[0]
    data = np.concatenate([xyz, rng.random((N, 3))], axis=1).astype(np.float32)
    labels = rng.integers(0, NCLS, size=N).astype(np.int32)
    data[17, 0], data[2500, 2] = np.nan, np.inf
    return data, labels


@pytest.mark.gpu
def test_a_raw_room_to_blocks_to_scores_and_back_by_both_endings():
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data, labels = raw_room()
    # the references alone: the condition on the input, and the exact counts
    want = gr.grid_subsample_ref(data, labels, voxel=VOXEL, mode="mean", num_class=NCLS)
    V = int(want["stats"][0])
    blocks = sr.scene_blocks_ref(want["data"][:V], want["labels"][:V], seed=0, step=0, **TILING)
    nb = int(blocks["stats"][0])
    assert V == 2053 and nb == 7 and int(blocks["stats"][5]) == 5             # five sparse cells are dropped
    voted = np.zeros(V, bool)
    slots = blocks["index"][:nb].reshape(-1)
    voted[slots[slots >= 0]] = True
    inv = want["inverse"]
    fin = inv >= 0
    neigh_ref = gi.neighbors_ref(want["voxel_cell"][:V], V)
    reach, _, _ = gi.interpolate_ref(data, inv, want["data"][:V], neigh_ref, np.ones((V, 1), np.float32), k=3,
                                     valid_labels=np.where(voted, 0, -1).astype(np.int32))
    proj_ref = fin & voted[np.maximum(inv, 0)]
    assert (int(fin.sum()), int(proj_ref.sum()), int((reach >= 0).sum())) == (FINITE, PROJECTED, INTERPOLATED)
    assert FINITE - PROJECTED >= 0.10 * FINITE and INTERPOLATED - PROJECTED >= 0.25 * (FINITE - PROJECTED)
    # the device
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample(d, torch.from_numpy(labels).to(dev), voxel=VOXEL, num_class=NCLS).trim()
    assert g.data.shape[0] == V
    sb = scene.scene_blocks(g.data, g.labels, **TILING).trim()
    assert sb.data.shape[0] == nb and np.array_equal(sb.index.cpu().numpy(), blocks["index"][:nb])
    scores = scene.SceneScores(V, NCLS, dev)
    logits = torch.nn.functional.one_hot(sb.labels.clamp(min=0).long(), NCLS).to(torch.float32) * 8.0
    scores.add(logits.contiguous(), sb.index.contiguous())
    valid = scores.labels().cpu().numpy()
    assert np.array_equal(valid >= 0, voted)
    got, got_scores = g.interpolate(d, scores, k=3, return_scores=True)
    ref = gi.interpolate_ref(data, g.inverse.cpu().numpy(), g.data.cpu().numpy(), g.neighbors().cpu().numpy(),
                             scores.scores.cpu().numpy(), k=3, valid_labels=valid)
    gi.assert_same(g.neighbors().cpu().numpy(), neigh_ref, "neighbours")
    gi.assert_same(got.cpu().numpy(), ref[0], "labels")
    gi.assert_same(got_scores.cpu().numpy(), ref[1], "scores")
    gi.assert_same(g.interp_stats.cpu().numpy(), ref[2], "stats")
    assert ref[2].tolist() == [INTERPOLATED, N - FINITE, FINITE - INTERPOLATED]
    got = got.cpu().numpy()
    proj = g.project(scores.labels()).cpu().numpy()
    assert np.array_equal(proj >= 0, proj_ref) and np.array_equal(got >= 0, reach >= 0)
    assert (got[fin] >= 0).sum() > (proj[fin] >= 0).sum() and (got[proj >= 0] >= 0).all()   # strictly more, and none lost
    assert (got[~fin] == -1).all() and (proj[~fin] == -1).all()
