"""The model's labels as a list of objects (-m gpu): the room and the pipeline of tests/test_grid_segments_model_step.py --
grid_subsample (mean) -> scene_blocks(cover=True) -> BatchProvider -> the five-layer scene stack -> SceneScores -> labels()
-> clean_labels(min_size=4) -> segments -> geometry -- checked against numpy on the host: every member's cell lies in its
segment's cell box, every raw row lies in that box mapped to space, and the zeroth moments are the segments' sizes and
rows."""
import numpy as np
import pytest

from tests import grid_ref as gr

NCLS, P, BATCH, VOXEL, MIN_SIZE = 13, 64, 16, 0.08, 4
F = np.float32


def raw_room():
    from pointwise_amd import synth
    N = 4000
    rng = np.random.default_rng(6200)
    xyz = synth.room_like(1, N, 6201, (3.2, 2.4, 3.0))[0]
    data = np.concatenate([xyz, rng.random((N, 3))], axis=1).astype(np.float32)
    data[17, 0], data[2500, 2] = np.nan, np.inf
    return data


def rows_lie_in_the_boxes(data, lo, voxel, row_segment, cell_box):
    """Every raw row with a segment: its xyz within [lo + low cell * voxel, lo + (high cell + 1) * voxel], in float64 from
    the float32 lo and voxel, widened by one float32 ulp of the coordinate (the cell is the floor of a rounded float32
    difference divided by voxel, rounded again)."""
    rows = np.nonzero(row_segment >= 0)[0]
    xyz = data[rows, :3]
    box = cell_box[row_segment[rows]].astype(np.float64)
    ulp = np.spacing(np.abs(xyz)).astype(np.float64)
    low = lo.astype(np.float64) + box[:, :3] * np.float64(F(voxel))
    high = lo.astype(np.float64) + (box[:, 3:] + 1.0) * np.float64(F(voxel))
    x = xyz.astype(np.float64)
    return rows.size, bool((x >= low - ulp).all() and (x <= high + ulp).all())


@pytest.mark.gpu
def test_a_room_s_predictions_become_boxes_that_hold_their_rows():
    import torch
    from pointwise_amd import _lib, grid, provider, scene, stack
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data = raw_room()
    N = data.shape[0]
    g = grid.grid_subsample(torch.from_numpy(data).to(dev), None, voxel=VOXEL).trim()
    V = g.data.shape[0]
    assert 500 < V < N
    sb = scene.scene_blocks(g.data, None, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True).trim()
    nb = sb.data.shape[0]
    pad = -nb % BATCH                                    # the provider drops a remainder: the first blocks vote twice
    blocks, index = torch.cat([sb.data, sb.data[:pad]]).contiguous(), torch.cat([sb.index, sb.index[:pad]]).contiguous()
    pv = provider.BatchProvider(blocks, index, BATCH, training=False, sort_cloud=True, device=dev)
    st = stack.Conv3pStack(pv.num_channels, NCLS, device=dev, seed=6203)
    scores = scene.SceneScores(V, NCLS, dev)
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        scores.add(st.forward(points, inp)[4].contiguous(), rows)
        if pv.has_next_batch():
            pv.next_batch()
    cleaned = g.clean_labels(scores.labels(), NCLS, MIN_SIZE)
    seg = g.segments(cleaned, NCLS)
    S = seg.num_segments()
    by_voxels, by_rows = seg.geometry("voxels"), seg.geometry("rows")
    assert by_voxels.num_segments() == S == by_rows.num_segments() and S > 1

    segment, cells = seg.segment.cpu().numpy(), g.voxel_cell.cpu().numpy()
    box = by_voxels.cell_box.cpu().numpy()
    assert np.array_equal(box, by_rows.cell_box.cpu().numpy()) and (segment >= 0).all()
    assert (cells >= box[segment, :3]).all() and (cells <= box[segment, 3:]).all()         # every member's cell
    for a in range(3):                                   # and the box is tight: some member touches every face
        assert np.array_equal(np.bincount(segment, weights=cells[:, a] == box[segment, a], minlength=S) > 0, np.ones(S, bool))
        assert np.array_equal(np.bincount(segment, weights=cells[:, a] == box[segment, 3 + a], minlength=S) > 0, np.ones(S, bool))
    _, lo, _, _, _ = gr.cells_of(data, VOXEL)
    row_segment = g.project(seg.segment).cpu().numpy()
    n, inside = rows_lie_in_the_boxes(data, lo, VOXEL, row_segment, box)
    assert n == N - 2 and inside                                                            # every finite raw row
    assert np.array_equal(by_voxels.moments[:, 0].cpu().numpy(), seg.size.cpu().numpy().astype(np.int64))
    assert np.array_equal(by_rows.moments[:, 0].cpu().numpy(), seg.rows.cpu().numpy().astype(np.int64))
    assert int(by_rows.moments[:, 0].sum()) == N - 2 and int(by_voxels.moments[:, 0].sum()) == V
    # the centroid lies in the box, the representatives' box in the cell box mapped to space
    cen = by_rows.centroid[:S].cpu().numpy()
    assert (cen >= box[:S, :3]).all() and (cen <= box[:S, 3:]).all()
    fbox = by_voxels.box[:S].cpu().numpy().astype(np.float64)
    step = np.float64(F(VOXEL))
    assert (fbox[:, :3] >= lo + box[:S, :3] * step - 1e-6).all() and (fbox[:, 3:] <= lo + (box[:S, 3:] + 1) * step + 1e-6).all()
    print("%d voxels, %d segments, %d of one voxel, %d flat" % ((V, S) + tuple(by_voxels.stats[1:3].tolist())))
