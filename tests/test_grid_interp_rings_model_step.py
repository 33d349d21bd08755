"""A raw room through the whole path, ended by interpolate(rings=) (-m gpu): tests/test_grid_interp_model_step.py's room
through grid_subsample (mean, majority labels) -> scene_blocks -> SceneScores fed one-hot logits of the blocks' own labels
-> interpolate(room, scores, k=3, rings=r, return_ring=True) for r = 1, 2, 4, 8.

Two tilings leave holes of two kinds.  The plain one of that test (min_points drops five sparse cells, num_point samples the
crowded ones) leaves holes a few voxels wide: of 2998 finite rows project labels 2027, and the rings 2571, 2716, 2808, 2922.
The covering one cut by max_blocks (6 of the 14 blocks it needs) leaves whole tiling cells, 12.5 voxels wide, without a
vote: 1670, 1742, 1873, 2323 -- eight rings reach 64 cm at this voxel.  Which voxels are voted for is the tiling's, so the
numpy references alone give the counts; the device must give the same rows, rings and counters, and the count never
falls as the rings grow."""
import numpy as np
import pytest

from tests import grid_interp_ref as gi
from tests import grid_interp_rings_ref as rr
from tests import grid_ref as gr
from tests import scene_cover_ref as sc
from tests import scene_ref as sr
from tests.test_grid_interp_model_step import FINITE, N, NCLS, TILING, VOXEL, raw_room

RINGS = (1, 2, 4, 8)
COVER = dict(num_point=256, block=1.0, stride=1.0, min_points=1, max_blocks=6)
LABELLED = {"plain": (2571, 2716, 2808, 2922), "cover": (1670, 1742, 1873, 2323)}


@pytest.mark.gpu
@pytest.mark.parametrize("tiling", ["plain", "cover"])
def test_a_raw_room_labelled_ring_after_ring(tiling):
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data, labels = raw_room()
    # the references alone: which voxels are voted for, and the exact counts
    want = gr.grid_subsample_ref(data, labels, voxel=VOXEL, mode="mean", num_class=NCLS)
    V = int(want["stats"][0])
    if tiling == "plain":
        blocks = sr.scene_blocks_ref(want["data"][:V], want["labels"][:V], seed=0, step=0, **TILING)
    else:
        blocks = sc.cover_blocks_ref(want["data"][:V], want["labels"][:V], seed=0, step=0, **COVER)
        assert blocks["stats"][0] == 6 and blocks["stats"][6] == 14          # the cut: 6 of the 14 blocks the cover needs
    nb = int(blocks["stats"][0])
    voted = np.zeros(V, bool)
    slots = blocks["index"][:nb].reshape(-1)
    voted[slots[slots >= 0]] = True
    reach = [rr.interpolate_rings_ref(data, want["inverse"], want["data"][:V], want["voxel_cell"][:V], V, np.ones((V, 1), np.float32),
                                      k=3, rings=r, valid_labels=np.where(voted, 0, -1).astype(np.int32)) for r in RINGS]
    assert tuple(int((x[0] >= 0).sum()) for x in reach) == LABELLED[tiling]
    # the device
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample(d, torch.from_numpy(labels).to(dev), voxel=VOXEL, num_class=NCLS).trim()
    assert g.data.shape[0] == V
    if tiling == "plain":
        sb = scene.scene_blocks(g.data, g.labels, **TILING).trim()
    else:
        sb = scene.scene_blocks(g.data, g.labels, cover=True, **COVER).trim()
    assert sb.data.shape[0] == nb and np.array_equal(sb.index.cpu().numpy(), blocks["index"][:nb])
    scores = scene.SceneScores(V, NCLS, dev)
    logits = torch.nn.functional.one_hot(sb.labels.clamp(min=0).long(), NCLS).to(torch.float32) * 8.0
    scores.add(logits.contiguous(), sb.index.contiguous())
    valid = scores.labels().cpu().numpy()
    assert np.array_equal(valid >= 0, voted)
    before, counts = None, []
    for r, there in zip(RINGS, reach):
        lab, out, ring = g.interpolate(d, scores, k=3, rings=r, return_scores=True, return_ring=True)
        ref = rr.interpolate_rings_ref(data, g.inverse.cpu().numpy(), g.data.cpu().numpy(), g.voxel_cell.cpu().numpy(), V,
                                       scores.scores.cpu().numpy(), k=3, rings=r, valid_labels=valid)
        for name, a, b in (("labels", lab, ref[0]), ("scores", out, ref[1]), ("ring", ring, ref[2]),
                           ("interp_stats", g.interp_stats, ref[3]), ("ring_stats", g.ring_stats, ref[4])):
            gi.assert_same(a.cpu().numpy(), b, "rings = %d: %s" % (r, name))
        lab = lab.cpu().numpy()
        assert np.array_equal(lab >= 0, there[0] >= 0) and np.array_equal(ring.cpu().numpy(), there[2])
        assert ref[3].tolist() == [int((lab >= 0).sum()), N - FINITE, FINITE - int((lab >= 0).sum())]
        assert before is None or ((before >= 0) <= (lab >= 0)).all()          # no row is lost as the rings grow
        assert before is None or np.array_equal(lab[before >= 0], before[before >= 0])
        before = lab
        counts.append(int((lab >= 0).sum()))
    assert tuple(counts) == LABELLED[tiling] and counts == sorted(counts)
