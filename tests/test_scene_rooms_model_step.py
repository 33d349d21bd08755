"""Two rooms through the whole evaluation path in one call (-m gpu): rooms A and C -> scene_blocks_rooms(cover=True,
min_points=1) -> BatchProvider(sort_cloud=True) with the global rows carried as the per-point labels -> the five-layer
scene stack -> SegmentationHead.evaluate -> one SceneScores over the rows of both rooms -> conv3p_seg_confusion over the
global rows.  Every finite row of both rooms gets a label, and room A's labels are those of the single-room chain
(tests/test_scene_cover_model_step.py's) run with the same key."""
import numpy as np
import pytest

from tests import scene_ref as base
from tests import scene_rooms_ref as rr

NCLS, P = 13, 64


def _labels_of(data_t, index_t, N, batch, dev, rows_labels):
    """blocks -> provider -> stack -> scores: (labels (N) int32 device tensor, rows seen)."""
    import torch
    from pointwise_amd import provider, scene, stack
    from pointwise_amd.seg_head import SegmentationHead
    pv = provider.BatchProvider(data_t, index_t, batch, training=False, sort_cloud=True, device=dev)
    st = stack.Conv3pStack(data_t.shape[2], NCLS, device=dev, seed=3303)
    hd = SegmentationHead(NCLS, device=dev)
    scores = scene.SceneScores(N, NCLS, dev)
    seen = 0
    for k in range(pv.num_batches):
        points, inp, rows = pv.get_batch_point_cloud()
        assert int(pv.bad_index) == 0
        acts = st.forward(points, inp)
        valid = rows >= 0
        lab = torch.where(valid, rows_labels[rows.clamp(min=0).long()], torch.full_like(rows, -1)).to(torch.int32)
        pred, counts = hd.evaluate(acts[4], lab)
        scores.add(acts[4].contiguous(), rows)
        seen += int(valid.sum())
        if pv.has_next_batch():
            pv.next_batch()
    return scores, seen


@pytest.mark.gpu
def test_two_rooms_to_covering_blocks_to_model_to_one_score_table():
    import torch
    from pointwise_amd import _lib, scene
    from pointwise_amd.conv3p_op import _call
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    room_a, room_c = base.room(**rr.ROOM_A), base.room(**rr.ROOM_C)
    data, rs, labels = rr.concat([room_a, room_c])
    N = data.shape[0]
    a = rr.call_args(min_points=1)
    d = torch.from_numpy(data).to(dev)
    lab32 = torch.from_numpy(labels.astype(np.int32)).to(dev)
    sb = scene.scene_blocks_rooms(d, rs, None, cover=True, **a)
    nb = sb.num_blocks()
    assert nb == sb.blocks_needed() and sb.stats[7].item() == 0
    t = sb.trim()
    na = t.room(0).data.shape[0]
    assert na == 58 and nb == 88                                             # room A alone needs 58 (A64min1), room C 30
    batch = 2                        # divides both 58 and 88 (the provider drops a remainder): room A's blocks fill the
    scores, seen = _labels_of(t.data, t.index, N, batch, dev, lab32)         # same batches in both chains
    assert seen == nb * P
    got = scores.labels()
    assert scores.counts().tolist() == [N, 0] and int(got.min()) >= 0        # every row of both rooms is labelled
    # the confusion matrix over the global rows of both rooms
    conf = torch.empty((NCLS, NCLS), dtype=torch.int64, device=dev)
    need = lib.conv3p_seg_confusion_workspace_bytes(N, NCLS)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _call(lib.conv3p_seg_confusion, lab32.data_ptr(), got.data_ptr(), N, NCLS, conf.data_ptr(), ws.data_ptr(), need,
              torch.cuda.current_stream(dev).cuda_stream)
    want = np.zeros((NCLS, NCLS), np.int64)
    np.add.at(want, (labels.astype(np.int64), got.cpu().numpy().astype(np.int64)), 1)
    assert np.array_equal(conf.cpu().numpy(), want) and int(conf.sum()) == N
    # room A alone, by the single-room call with the key seed + 0: the same blocks, so the same labels for its rows
    one = scene.scene_blocks(d[:3000].contiguous(), None, cover=True, **a).trim()
    assert np.array_equal(one.index.cpu().numpy(), t.room(0).index.cpu().numpy())
    assert np.array_equal(one.data.cpu().numpy().view(np.uint32), t.room(0).data.cpu().numpy().view(np.uint32))
    single, _ = _labels_of(one.data, one.index, 3000, batch, dev, lab32[:3000].contiguous())
    assert np.array_equal(single.labels().cpu().numpy(), got[:3000].cpu().numpy())
