"""The model's segments joined by a caller's policy on the way back to the raw rows (-m gpu): a synthetic room, xyz + rgb ->
grid_subsample (mean) -> scene_blocks(cover=True, min_points=1) -> BatchProvider(sort_cloud=True) with the blocks' `index`
as the per-point labels -> the five-layer scene stack -> SceneScores -> labels() -> GridSubsample.segments ->
GridSegments.adjacency -> a policy written as a torch expression on `contacts` and `start` (every segment below 4 voxels
joins the neighbour it shares the most contacts with) -> SegmentAdjacency.merge -> GridSubsample.project: the adjacency,
the merge and the projected rows equal tests/grid_adjacency_ref.py to the bit, and the segment counts and sizes add up."""
import numpy as np
import pytest

from tests import grid_adjacency_ref as ga
from tests import grid_ref as gr
from tests import grid_segments_ref as gs
from tests.test_grid_segments_model_step import BATCH, NCLS, P, VOXEL, raw_room

MIN_SIZE = 4
ADJ = ("start", "src", "dst", "contacts", "voxels", "offset", "twin", "border", "stats")


@pytest.mark.gpu
def test_a_room_s_small_segments_join_the_neighbour_they_touch_most():
    import torch
    from pointwise_amd import _lib, grid, provider, scene, stack
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data = raw_room()
    N = data.shape[0]
    want = gr.grid_subsample_ref(data, None, voxel=VOXEL, mode="mean")
    V = int(want["stats"][0])
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=VOXEL).trim()
    sb = scene.scene_blocks(g.data, None, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True).trim()
    pad = -sb.data.shape[0] % BATCH                      # the provider drops a remainder: the first blocks vote twice
    blocks, index = torch.cat([sb.data, sb.data[:pad]]).contiguous(), torch.cat([sb.index, sb.index[:pad]]).contiguous()
    pv = provider.BatchProvider(blocks, index, BATCH, training=False, sort_cloud=True, device=dev)
    st = stack.Conv3pStack(pv.num_channels, NCLS, device=dev, seed=6203)
    scores = scene.SceneScores(V, NCLS, dev)
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        scores.add(st.forward(points, inp)[4].contiguous(), rows)
        if pv.has_next_batch():
            pv.next_batch()
    voxel_labels = scores.labels()

    seg = g.segments(voxel_labels, NCLS)
    adj = seg.adjacency()
    if adj.overflowed():                                 # an untrained model's labels are speckle: more than 2 V edges
        adj = seg.adjacency(max_edges=adj.edges_bound())  # always fits
    assert not adj.overflowed()
    rows_e = adj.shape[1]
    # the policy, on the device: a segment below MIN_SIZE voxels joins along its edge(s) of most contacts
    degree = adj.start[1:] - adj.start[:-1]
    row = torch.repeat_interleave(torch.arange(V, device=dev), degree.long())          # the src of every edge, from start
    E = adj.num_edges()
    assert row.numel() == E and torch.equal(row.to(torch.int32), adj.src[:E])
    contacts = adj.contacts[:E]
    most = torch.zeros(V, dtype=torch.int32, device=dev).scatter_reduce(0, row, contacts, "amax")
    select = torch.zeros(adj.shape[1], dtype=torch.bool, device=dev)
    select[:E] = (seg.size[row] < MIN_SIZE) & (contacts == most[row])
    merged = adj.merge(select)

    neigh, lab = g.neighbors().cpu().numpy(), voxel_labels.cpu().numpy()
    ref = gs.segments_ref(neigh, lab, V, g.voxel_count.cpu().numpy(), V, NCLS, 26)
    ref_adj = ga.adjacency_ref(neigh, ref["segment"], ref["stats"][0], V, 26, rows_e)
    for k in ADJ:
        assert np.array_equal(getattr(adj, k).cpu().numpy(), ref_adj[k]), k
    S, Er = int(ref["stats"][0]), int(ref_adj["stats"][0])
    src, con = ref_adj["src"][:Er], ref_adj["contacts"][:Er]
    top = np.zeros(V, np.int32)
    np.maximum.at(top, src, con)
    sel = np.zeros(rows_e, bool)
    sel[:Er] = (ref["size"][src] < MIN_SIZE) & (con == top[src])
    assert np.array_equal(select.cpu().numpy(), sel)
    ref_m = ga.merge_ref(ref, ref_adj["src"], ref_adj["dst"], sel)
    for k in ("segment", "root", "size", "rows", "label", "stats", "seg_map", "merge_stats"):
        assert np.array_equal(getattr(merged, k).cpu().numpy(), ref_m[k]), k

    # the counts add up: every small segment with a neighbour is gone into a group, nothing else moved
    S2 = merged.num_segments()
    small = ref["size"][:S] < MIN_SIZE
    touched = np.diff(ref_adj["start"][:S + 1]) > 0
    ms = ref_m["merge_stats"]
    print("%d voxels, %d segments, %d edges, %d small of which %d touch another: %d groups, %d of more than one segment"
          % (V, S, Er, small.sum(), (small & touched).sum(), S2, ms[3]))
    assert ms[0] == S2 <= S and ms[1] == S and (small & touched).any() and S2 < S
    assert ref_m["size"][:S2].sum() == ref["size"][:S].sum() == ref["stats"][1] and ref_m["rows"][:S2].sum() == N - 2
    untouched = np.ones(S, bool)                         # segments on no selected edge keep their size under their new number
    untouched[src[sel[:Er]]] = False
    untouched[ref_adj["dst"][:Er][sel[:Er]]] = False
    assert np.array_equal(ref_m["size"][ref_m["seg_map"][:S][untouched]], ref["size"][:S][untouched])
    rows_out = g.project(merged.segment).cpu().numpy()                       # a group number per raw row
    assert np.array_equal(rows_out, gr.project_ref(ref_m["segment"], want["inverse"]))
    fin = np.isfinite(data[:, :3]).all(axis=1)
    assert (rows_out[fin] >= 0).all() and (rows_out[~fin] == -1).all()
