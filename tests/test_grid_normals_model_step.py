"""A raw room with estimated normals through the whole path (-m gpu): a synthetic room, xyz + rgb -> grid_subsample (mean)
-> GridSubsample.normals towards a viewpoint in the room -> with_normals -> scene_blocks(cover=True, min_points=1) on the
(V, 9) rows -> blocks of 12 channels (xyz, rgb, normal, room-normalised xyz) -> BatchProvider(sort_cloud=True) with the
blocks' `index` as the per-point labels -> the five-layer scene stack with 12 input channels -> SceneScores -> labels()
-> GridSubsample.project: every finite raw row comes out with a label."""
import numpy as np
import pytest

from tests import grid_normals_ref as gn
from tests import grid_ref as gr

NCLS, P, BATCH, VOXEL = 13, 64, 16, 0.08


def raw_room():
    from pointwise_amd import synth
    N = 4000
    rng = np.random.default_rng(6100)
    xyz = synth.room_like(1, N, 6101, (3.2, 2.4, 3.0))[0]
    data = np.concatenate([xyz, rng.random((N, 3))], axis=1).astype(np.float32)
    data[17, 0], data[2500, 2] = np.nan, np.inf
    return data


@pytest.mark.gpu
def test_a_raw_room_gains_normals_and_goes_through_a_twelve_channel_model():
    import torch
    from pointwise_amd import _lib, grid, provider, scene, stack
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    data = raw_room()
    N = data.shape[0]
    want = gr.grid_subsample_ref(data, None, voxel=VOXEL, mode="mean")
    V = int(want["stats"][0])
    d = torch.from_numpy(data).to(dev)
    g = grid.grid_subsample(d, None, voxel=VOXEL).trim()
    assert g.data.shape == (V, 6) and 500 < V < N
    viewpoint = (1.6, 1.2, 1.5)
    nrm = g.normals(viewpoint=viewpoint, return_moments=True)
    samples, flags, moments, stats = gn.moments_ref(g.data.cpu().numpy(), g.neighbors().cpu().numpy(), V, 6)
    assert np.array_equal(nrm.flags.cpu().numpy(), flags) and nrm.stats.cpu().numpy().tolist() == stats.tolist()
    assert np.array_equal(nrm.moments.cpu().numpy().view(np.uint32), moments.view(np.uint32))
    gn.compare_r5(nrm.normals.cpu().numpy(), nrm.curvature.cpu().numpy(), flags, moments, g.data.cpu().numpy(), viewpoint)
    assert nrm.count() == stats[0] > 0 and int(stats[:3].sum()) == V and stats[3] == 0   # a sparse room: many voxels have too few samples
    rows9 = g.with_normals(nrm)
    assert rows9.shape == (V, 9) and rows9.is_contiguous()
    sb = scene.scene_blocks(rows9, None, num_point=P, block=1.0, stride=0.5, min_points=1, cover=True)
    assert sb.num_blocks() == sb.blocks_needed() and int(sb.stats[7]) == 0
    sb = sb.trim()
    nb = sb.data.shape[0]
    assert tuple(sb.data.shape) == (nb, P, 12)                                # xyz, rgb, normal, room-normalised xyz
    idx = sb.index.cpu().numpy()
    blk = sb.data.cpu().numpy()
    ok = idx >= 0
    assert np.array_equal(np.ascontiguousarray(blk[ok][:, 3:9]).view(np.uint32),
                          np.ascontiguousarray(rows9.cpu().numpy()[idx[ok]][:, 3:9]).view(np.uint32))   # carried as they are
    assert np.unique(idx[ok]).size == V                                         # covering: every voxel is in a block
    pad = -nb % BATCH                                    # the provider drops a remainder: the first blocks vote twice
    blocks, index = torch.cat([sb.data, sb.data[:pad]]).contiguous(), torch.cat([sb.index, sb.index[:pad]]).contiguous()
    pv = provider.BatchProvider(blocks, index, BATCH, training=False, sort_cloud=True, device=dev)
    assert pv.num_channels == 12 and pv.num_batches * BATCH == nb + pad and nb > pad
    st = stack.Conv3pStack(12, NCLS, device=dev, seed=6103)
    scores = scene.SceneScores(V, NCLS, dev)
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        assert tuple(inp.shape)[-1] == 12 and int(pv.bad_index) == 0
        acts = st.forward(points, inp)
        assert tuple(acts[4].shape)[-1] == NCLS and bool(torch.isfinite(acts[4]).all())
        scores.add(acts[4].contiguous(), rows)
        if pv.has_next_batch():
            pv.next_batch()
    voxel_labels = scores.labels()
    assert scores.counts().tolist() == [V, 0] and int(voxel_labels.min()) >= 0
    got = g.project(voxel_labels).cpu().numpy()
    fin = np.isfinite(data[:, :3]).all(axis=1)
    assert np.array_equal(got, gr.project_ref(voxel_labels.cpu().numpy(), want["inverse"]))
    assert (got[fin] >= 0).all() and (got[~fin] == -1).all() and fin.sum() == N - 2
