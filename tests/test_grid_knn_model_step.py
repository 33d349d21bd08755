"""A raw room through the whole path, ended by knn(...).interpolate (-m gpu): tests/test_grid_interp_rings_model_step.py's
room and its two tilings through grid_subsample -> scene_blocks -> SceneScores -> g.knn(voxel, room, k=3, rings=r,
valid_labels=scores).interpolate(scores) for r = 1, 2, 4, 8.

The rows the table labels are a superset of the plain call's and exactly the ring call's at the same r (the counts of that
test: both label the rows with a voted voxel in the cube of r).  At r = 1 labels and scores are the plain call's to the
bit.  Where the two differ at r > 1 the k-NN's neighbours are the nearer ones by construction: the ring call stops at the
first cube that is not empty, the table holds the 3 nearest of the cube of r.  The share of labelled rows whose label
differs from the ring call's is RECORDED (printed with -s, next to the mean scanned ring and the certified share), not
asserted."""
import numpy as np
import pytest

from tests import grid_interp_ref as gi
from tests.test_grid_interp_model_step import NCLS, TILING, VOXEL, raw_room
from tests.test_grid_interp_rings_model_step import COVER, LABELLED, RINGS


@pytest.mark.gpu
@pytest.mark.parametrize("tiling", ["plain", "cover"])
def test_a_raw_room_labelled_from_its_nearest_voted_voxels(tiling):
    import torch
    from pointwise_amd import _lib, grid, scene
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data, labels = raw_room()
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample(d, torch.from_numpy(labels).to(dev), voxel=VOXEL, num_class=NCLS).trim()
    V = g.data.shape[0]
    if tiling == "plain":
        sb = scene.scene_blocks(g.data, g.labels, **TILING).trim()
    else:
        sb = scene.scene_blocks(g.data, g.labels, cover=True, **COVER).trim()
    scores = scene.SceneScores(V, NCLS, dev)
    logits = torch.nn.functional.one_hot(sb.labels.clamp(min=0).long(), NCLS).to(torch.float32) * 8.0
    scores.add(logits.contiguous(), sb.index.contiguous())
    plain = g.interpolate(d, scores, k=3, return_scores=True)
    counts, shares = [], []
    for r in RINGS:
        ringed = g.interpolate(d, scores, k=3, rings=r)
        t = g.knn(VOXEL, d, k=3, rings=r, valid_labels=scores)
        lab, out = t.interpolate(scores, return_scores=True)
        assert bool(((plain[0] >= 0) <= (lab >= 0)).all())               # a superset of the plain call's rows
        assert torch.equal(lab >= 0, ringed >= 0)                        # the ring call's rows at the same r
        if r == 1:
            gi.assert_same(lab.cpu().numpy(), plain[0].cpu().numpy(), "one ring: labels")
            gi.assert_same(out.cpu().numpy(), plain[1].cpu().numpy(), "one ring: scores")
        n = int((lab >= 0).sum())
        counts.append(n)
        shares.append(int(((lab != ringed) & (lab >= 0)).sum()) / max(n, 1))
        st = t.stats.cpu().tolist()
        print("%s, rings = %d: %d rows labelled, %.4f of them differ from the ring call's; mean scanned %.3f, certified %.4f" % (
            tiling, r, n, shares[-1], st[5] / max(sum(st[:3]), 1), st[4] / max(sum(st[:3]), 1)))
    assert tuple(counts) == LABELLED[tiling] and shares[0] == 0.0
