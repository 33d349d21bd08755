"""A room through the whole path (-m gpu): room B -> scene_blocks -> BatchProvider(sort_cloud=True) with the blocks'
`index` carried as the per-point labels -> the five-layer scene stack forward at B x 256 points ->
SegmentationHead.evaluate predictions -> SceneVotes.  The sort permutes every block's rows, and the room rows ride
along, so the votes a room row receives are exactly the number of times it was emitted: integers, compared for
equality."""
import numpy as np
import pytest

from tests import scene_ref as ref


@pytest.mark.gpu
def test_room_to_blocks_to_model_to_votes():
    import torch
    from pointwise_amd import _lib, provider, scene, stack
    from pointwise_amd.seg_head import SegmentationHead
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    NCLS, P, BATCH = 13, 256, 10
    room = ref.room(3000, 2, (4.2, 3.1, 3.0))
    N, K = room.shape
    room_labels = np.random.default_rng(52).integers(0, NCLS, size=N).astype(np.uint8)
    want = ref.scene_blocks_ref(room, room_labels, P, 1.0, 0.5, 100, 30, seed=7, step=3)
    sb = scene.scene_blocks(torch.from_numpy(room).to(dev), torch.from_numpy(room_labels).to(dev), num_point=P, stride=0.5,
                            max_blocks=30, seed=7, step=3)
    assert sb.stats.tolist() == want["stats"].tolist() and sb.stats[7] == 0
    t = sb.trim()
    assert t.data.shape == (30, P, K + 3) and np.array_equal(t.index.cpu().numpy(), want["index"])
    pv = provider.BatchProvider(t.data, t.index, BATCH, training=False, sort_cloud=True, device=dev)
    assert pv.num_batches == 3 and pv.num_channels == K + 3 and not pv.rotate and not pv.jitter
    st = stack.Conv3pStack(K + 3, NCLS, device=dev, seed=3303)
    hd = SegmentationHead(NCLS, device=dev)
    votes = scene.SceneVotes(N, NCLS, dev)
    lab_dev = torch.from_numpy(room_labels.astype(np.int64)).to(dev)
    seen = np.zeros(N, np.int64)
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (BATCH, P) and int(pv.bad_index) == 0
        r = rows.cpu().numpy()
        blocks = want["index"][k * BATCH:(k + 1) * BATCH]
        assert np.array_equal(np.sort(r, axis=1), np.sort(blocks, axis=1))             # the rows rode through the sort
        assert torch.equal(inp[:, :, 3:K], torch.from_numpy(room).to(dev)[rows.long()][:, :, 3:K])
        acts = st.forward(points, inp)
        labels = lab_dev[rows.long()].to(torch.int32)
        pred, counts = hd.evaluate(acts[4], labels)
        assert pred.dtype == torch.int32 and int(pred.min()) >= 0 and int(pred.max()) < NCLS
        assert int(counts["invalid"]) == 0
        votes.add(pred.contiguous(), rows)
        seen += np.bincount(r.reshape(-1), minlength=N)
        if pv.has_next_batch():
            pv.next_batch()
    assert np.array_equal(votes.votes.sum(dim=1).cpu().numpy(), seen) and seen.sum() == 30 * P
    assert np.array_equal(seen, np.bincount(want["index"].reshape(-1), minlength=N))
    lab = votes.labels().cpu().numpy()
    assert np.array_equal(lab >= 0, seen > 0) and votes.counts().tolist() == [int((seen > 0).sum()), int((seen == 0).sum())]
