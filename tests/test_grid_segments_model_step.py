"""The model's labels cleaned up on the way back to the raw rows (-m gpu): a synthetic room, xyz + rgb -> grid_subsample
(mean) -> scene_blocks(cover=True, min_points=1) -> BatchProvider(sort_cloud=True) with the blocks' `index` as the
per-point labels -> the five-layer scene stack -> SceneScores -> labels() -> GridSubsample.clean_labels(min_size=4) ->
GridSubsample.project: the cleaned labels equal tests/grid_segments_ref.py to the bit, voxels of segments that are not
small keep their label, and the counts of the clean-up add up."""
import numpy as np
import pytest

from tests import grid_ref as gr
from tests import grid_segments_ref as gs

NCLS, P, BATCH, VOXEL, MIN_SIZE = 13, 64, 16, 0.08, 4


def raw_room():
    from pointwise_amd import synth
    N = 4000
    rng = np.random.default_rng(6200)
    xyz = synth.room_like(1, N, 6201, (3.2, 2.4, 3.0))[0]
    data = np.concatenate([xyz, rng.random((N, 3))], axis=1).astype(np.float32)
    data[17, 0], data[2500, 2] = np.nan, np.inf
    return data


@pytest.mark.gpu
def test_a_room_s_predictions_are_segmented_and_cleaned_before_they_reach_the_rows():
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
    assert g.data.shape == (V, 6) and 500 < V < N
    sb = scene.scene_blocks(g.data, None, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True)
    assert sb.num_blocks() == sb.blocks_needed() and int(sb.stats[7]) == 0
    sb = sb.trim()
    nb = sb.data.shape[0]
    pad = -nb % BATCH                                    # the provider drops a remainder: the first blocks vote twice
    blocks, index = torch.cat([sb.data, sb.data[:pad]]).contiguous(), torch.cat([sb.index, sb.index[:pad]]).contiguous()
    pv = provider.BatchProvider(blocks, index, BATCH, training=False, sort_cloud=True, device=dev)
    st = stack.Conv3pStack(pv.num_channels, NCLS, device=dev, seed=6203)
    scores = scene.SceneScores(V, NCLS, dev)
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        acts = st.forward(points, inp)
        scores.add(acts[4].contiguous(), rows)
        if pv.has_next_batch():
            pv.next_batch()
    voxel_labels = scores.labels()
    assert scores.counts().tolist() == [V, 0] and int(voxel_labels.min()) >= 0

    seg = g.segments(voxel_labels, NCLS)
    cleaned = seg.absorb(MIN_SIZE)
    assert torch.equal(g.clean_labels(voxel_labels, NCLS, MIN_SIZE), cleaned)
    neigh, lab = g.neighbors().cpu().numpy(), voxel_labels.cpu().numpy()
    ref = gs.segments_ref(neigh, lab, V, g.voxel_count.cpu().numpy(), V, NCLS, 26)
    for k in ("segment", "root", "size", "rows", "label", "stats"):
        assert np.array_equal(getattr(seg, k).cpu().numpy(), ref[k]), k
    ref_a = gs.absorb_ref(neigh, lab, V, ref, V, NCLS, 26, MIN_SIZE, False)
    got = cleaned.cpu().numpy()
    assert np.array_equal(got, ref_a["labels"]) and np.array_equal(seg.absorbed_label.cpu().numpy(), ref_a["seg_label"])
    stats = seg.absorb_stats.cpu().numpy()
    assert np.array_equal(stats, ref_a["stats"])
    S = seg.num_segments()
    small = ref["size"][ref["segment"]] < MIN_SIZE
    assert np.array_equal(got[~small], lab[~small])                          # segments that are not small are untouched
    assert stats[0] == stats[1] + stats[2] == (ref["size"][:S] < MIN_SIZE).sum()
    assert stats[3] == (got != lab).sum() <= small.sum() and ref["rows"][:S].sum() == N - 2
    print("%d voxels, %d segments, %d small: %d absorbed, %d orphans, %d voxels relabelled"
          % (V, S, stats[0], stats[1], stats[2], stats[3]))

    rows_out = g.project(cleaned).cpu().numpy()
    fin = np.isfinite(data[:, :3]).all(axis=1)
    assert np.array_equal(rows_out, gr.project_ref(ref_a["labels"], want["inverse"]))
    assert (rows_out[fin] >= 0).all() and (rows_out[~fin] == -1).all()
    row_segment = g.project(seg.segment).cpu().numpy()                       # a segment number per raw row
    assert np.array_equal(row_segment, gr.project_ref(ref["segment"], want["inverse"]))
