"""A room through the whole evaluation path (-m gpu): room A -> scene_blocks(cover=True, min_points=1) -> 58 blocks that
hold every one of its 3000 rows -> BatchProvider(sort_cloud=True) with the blocks' `index` carried as the per-point labels
-> the five-layer scene stack forward at 29 x 64 points -> SegmentationHead.evaluate predictions -> SceneVotes, and the
stack's last activations -> SceneScores.  Every room row gets a label; the plain mode shows the model 911 of them."""
import numpy as np
import pytest

from tests import scene_cover_ref as cref
from tests import scene_ref as ref


@pytest.mark.gpu
def test_room_to_covering_blocks_to_model_to_votes_and_scores():
    import torch
    from pointwise_amd import _lib, provider, scene, stack
    from pointwise_amd.seg_head import SegmentationHead
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    NCLS, P, BATCH = 13, 64, 29
    room, room_labels, a, want = cref.fixture("A64min1")
    N, K = room.shape
    plain = ref.scene_blocks_ref(room, None, **dict(a, max_blocks=20))
    assert np.unique(plain["index"]).size == 911                            # what the plain mode emits of this room
    sb = scene.scene_blocks(torch.from_numpy(room).to(dev), torch.from_numpy(room_labels).to(dev), cover=True, **a)
    assert sb.stats.tolist() == want["stats"].tolist() and sb.num_blocks() == sb.blocks_needed() == 58
    t = sb.trim()
    assert t.data.shape == (58, P, K + 3) and np.array_equal(t.index.cpu().numpy(), want["index"])
    pv = provider.BatchProvider(t.data, t.index, BATCH, training=False, sort_cloud=True, device=dev)
    assert pv.num_batches == 2 and pv.num_channels == K + 3
    st = stack.Conv3pStack(K + 3, NCLS, device=dev, seed=3303)
    hd = SegmentationHead(NCLS, device=dev)
    votes = scene.SceneVotes(N, NCLS, dev)
    scores = scene.SceneScores(N, NCLS, dev)
    lab_dev = torch.from_numpy(room_labels.astype(np.int64)).to(dev)
    seen = np.zeros(N, np.int64)
    all_acts, all_rows = [], []
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (BATCH, P) and int(pv.bad_index) == 0
        r = rows.cpu().numpy()
        blocks = want["index"][k * BATCH:(k + 1) * BATCH]
        assert np.array_equal(np.sort(r, axis=1), np.sort(blocks, axis=1))             # the rows rode through the sort
        acts = st.forward(points, inp)
        labels = lab_dev[rows.long()].to(torch.int32)
        pred, counts = hd.evaluate(acts[4], labels)
        assert int(counts["invalid"]) == 0
        votes.add(pred.contiguous(), rows)
        scores.add(acts[4].contiguous(), rows)
        all_acts.append(acts[4].cpu().numpy().reshape(-1, NCLS))
        all_rows.append(r.reshape(-1))
        seen += np.bincount(r.reshape(-1), minlength=N)
        if pv.has_next_batch():
            pv.next_batch()
    assert votes.counts().tolist() == [3000, 0] and scores.counts().tolist() == [3000, 0]   # every room row has a label
    assert np.array_equal(seen, np.bincount(want["index"].reshape(-1), minlength=N)) and seen.sum() == 58 * P
    assert seen.min() >= 1
    assert np.array_equal(votes.votes.sum(dim=1).cpu().numpy(), seen)       # the vote totals are the emission counts
    acts, rows = np.concatenate(all_acts), np.concatenate(all_rows)
    assert np.isfinite(acts).all() and scores.vote_stats.tolist() == [58 * P, 0]
    ref64, nvotes = cref.scores_ref64(acts, rows, N)
    assert np.array_equal(nvotes, seen)
    got = scores.scores.cpu().numpy()
    err = np.abs(got / float(cref.SCALE) - ref64).max(axis=1)
    print("max |scores / 2^30 - ref| / votes %.3e (bound %.3e)" % ((err / seen).max(), cref.SCORE_TOL))
    assert np.all(err <= seen * cref.SCORE_TOL)
    lab = scores.labels().cpu().numpy()
    assert np.array_equal(lab, cref.score_labels_ref(got)[0]) and lab.min() >= 0
