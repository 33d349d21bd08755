"""A planted room through the object side of the pipeline, ended by match() (-m gpu): tests/grid_match_cases.py's separated
boxes, the instance id of a row the box it was drawn in.

First grid_subsample -> segments() (geometric: connected occupied voxels) -> match: the segments ARE the boxes, so every
instance is matched, PQ is 1.0 exactly and the coverage sums are instances * 2^30.  Then 5 % of the voxel labels are redrawn
(tests/test_grid_match_host.py chose the seed on the references): segments(labels) -> adjacency().agglomerate(min_size=8) ->
match; summary() equals the reference's on the arrays read back, and PQ after the agglomeration is not below PQ before --
a property of the planted scene, where a redrawn voxel is a tiny segment inside a box."""
import numpy as np
import pytest

from tests import grid_match_cases as mc
from tests import grid_match_ref as mr


@pytest.mark.gpu
def test_planted_boxes_are_matched_and_agglomeration_does_not_lower_pq():
    import torch
    from pointwise_amd import _lib, grid
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    boxes = 4
    data, inst, _, _ = mc.boxes_scene(boxes)
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=0.1)
    truth = torch.from_numpy(inst).to(dev)
    M = g.data.shape[0]
    assert g.num_voxels() == 125 * boxes

    m = g.segments().match(truth, boxes)
    assert m.num_pairs() == boxes and bool((m.truth_match >= 0).all())
    s = m.summary()
    assert s["pq"] == [1.0] and s["mean_pq"] == s["mean_sq"] == s["mean_rq"] == s["mcov"] == s["mwcov"] == 1.0
    st = m.stats.cpu().tolist()
    assert st[8] == boxes << 30 and st[9] == data.shape[0] << 30 and st[10] == data.shape[0] and st[3] == boxes

    cells = g.voxel_cell.cpu().numpy()[:125 * boxes]
    labels = np.full(M, -1, np.int32)
    labels[:cells.shape[0]] = mc.redrawn_labels(cells, mc.MODEL_STEP_SEED)
    tcls = (np.arange(boxes) % 3).astype(np.int32)
    tc = torch.from_numpy(tcls).to(dev)
    seg = g.segments(torch.from_numpy(labels).to(dev), 3)
    agg = seg.adjacency().agglomerate(min_size=8)
    assert agg.converged()
    pq = []
    for what, sg in (("before", seg), ("after", agg.segments)):
        m = sg.match(truth, boxes, pred_class=sg.label, truth_class=tc, num_class=3)
        ref = mr.match_ref(sg.segment.cpu().numpy(), int(sg.stats[0]), g.inverse.cpu().numpy(), int(g.stats[0]), inst, boxes, "rows",
                           sg.label.cpu().numpy(), tcls, 3, (1, 2), M)
        for name in mr.OUTPUTS:
            assert np.array_equal(getattr(m, name).cpu().numpy(), ref[name]), (what, name)
        s = m.summary()
        assert s == mr.summary_ref(ref)
        print("%s: %d segments, mean PQ %.6f, SQ %.6f, RQ %.6f, mCov %.6f" % (what, sg.num_segments(), s["mean_pq"], s["mean_sq"],
                                                                            s["mean_rq"], s["mcov"]))
        pq.append(s["mean_pq"])
    assert pq[0] < pq[1] == 1.0
