"""Noisy voxel labels cleaned up on the way back to the raw rows (-m gpu): the synthetic room of the other model-step tests
-> grid_subsample (mean) -> a label per voxel in bands with a tenth of them redrawn -> GridSubsample.segments ->
GridSegments.adjacency -> SegmentAdjacency.agglomerate(min_size=8) -> GridSubsample.project: no group below 8 voxels (or,
with weight="rows", below 8 raw rows) that has a neighbour is left, a labelled row is never unlabelled, and the cleaned rows
-- and the number of rows whose label changed -- equal tests/grid_agglomerate_ref.py on the references' own segmentation and
adjacency."""
import numpy as np
import pytest

from tests import grid_adjacency_ref as ga
from tests import grid_agglomerate_ref as ar
from tests import grid_ref as gr
from tests import grid_segments_ref as gs
from tests.test_grid_segments_model_step import NCLS, VOXEL, raw_room

MIN_SIZE = 8


@pytest.mark.gpu
def test_a_room_s_noisy_labels_are_folded_into_their_surroundings():
    import torch
    from pointwise_amd import _lib, grid
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data = raw_room()
    want = gr.grid_subsample_ref(data, None, voxel=VOXEL, mode="mean")
    V = int(want["stats"][0])
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=VOXEL).trim()
    cells = g.voxel_cell.cpu().numpy()
    rng = np.random.default_rng(6210)
    lab = ((cells[:, 2] // 6 + 2 * (cells[:, 0] // 16)) % NCLS).astype(np.int32)
    noise = rng.random(V) < 0.1
    lab[noise] = rng.integers(0, NCLS, int(noise.sum()))
    voxel_labels = torch.from_numpy(lab).to(dev)

    seg = g.segments(voxel_labels, NCLS)
    adj = seg.adjacency(max_edges=26 * V)
    assert not adj.overflowed()
    neigh, count = g.neighbors().cpu().numpy(), g.voxel_count.cpu().numpy()
    ref = gs.segments_ref(neigh, lab, V, count, V, NCLS, 26)
    ref_adj = ga.adjacency_ref(neigh, ref["segment"], ref["stats"][0], V, 26, 26 * V)
    S = int(ref["stats"][0])
    row_before = gr.project_ref(lab, want["inverse"])
    fin = np.isfinite(data[:, :3]).all(axis=1)
    for weight, sizes in (("voxels", "size"), ("rows", "rows")):
        res = adj.agglomerate(MIN_SIZE, weight=weight)
        rows_out = g.project(res.voxel_label).cpu().numpy()
        r = ar.agglomerate_ref(ref, ref_adj, MIN_SIZE, weight=int(weight == "rows"))
        assert r["agg_stats"][5] == 0 and res.converged()                      # the fixed point, within the default rounds
        for k in ("segment", "size", "rows", "label", "stats"):
            assert np.array_equal(getattr(res.segments, k).cpu().numpy(), r[k]), (weight, k)
        assert np.array_equal(res.stats.cpu().numpy(), r["agg_stats"]) and np.array_equal(res.voxel_label.cpu().numpy(), r["voxel_label"])
        G = res.num_groups()
        small = r[sizes][:G] < MIN_SIZE                                        # what is left below the threshold ...
        assert small.sum() == r["agg_stats"][4] and not np.diff(r["start"][:G + 1])[small].any()     # ... touches nothing
        assert (ref[sizes][:S] < MIN_SIZE).sum() > small.sum() and G < S
        want_rows = gr.project_ref(r["voxel_label"], want["inverse"])
        assert np.array_equal(rows_out, want_rows)
        assert (rows_out[row_before >= 0] >= 0).all() and (rows_out[fin] >= 0).all() and (rows_out[~fin] == -1).all()
        changed = int((rows_out != row_before).sum())
        assert changed == int((want_rows != row_before).sum()) and 0 < changed < fin.sum() // 2
        print("%s: %d voxels, %d segments -> %d groups in %d rounds, %d small left, %d of %d rows relabelled"
              % (weight, V, S, G, res.num_rounds(), small.sum(), changed, fin.sum()))
