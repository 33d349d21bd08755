"""CPU tests (not gpu) of the segmentation loss head's host side: the module imports, the C ABI exports and binds the
three seg-head symbols, workspace sizing, status codes that are decided before any HIP call, the argument checks of
SegmentationHead, the summary arithmetic, and the numpy restatement against the reference's per-point loop."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op

from tests.seg_head_ref import seg_head_ref, selu


def test_module_imports_and_is_exported():
    import pointwise_amd
    from pointwise_amd import seg_head
    assert pointwise_amd.SegmentationHead is seg_head.SegmentationHead
    assert "SegmentationHead" in pointwise_amd.__all__


def test_symbols_are_bound_and_the_profile_kind_is_last():
    lib = _lib.load()
    for n in ("conv3p_seg_head_workspace_bytes", "conv3p_seg_head_f32", "conv3p_seg_head_f64"):
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert names[-1] == "seg_head_kernel"
    assert names.index("generic_backward_kernel") == len(names) - 2        # appended: no earlier index moved
    assert lib.conv3p_abi_version() == 5


def test_workspace_bytes():
    lib = _lib.load()
    f = lib.conv3p_seg_head_workspace_bytes
    sizes = [f(r, 13) for r in (1, 63, 64, 65, 1000, 65536, 524288, 1 << 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[5]
    assert f(1000, 41) > f(1000, 13) and f(65536, 128) > f(65536, 41)
    assert f(1, 13) >= 8 + 4 * (2 + 3 * 13)                                 # one record: {double, int32[2 + 3 C]}
    assert f(0, 13) == 0 and f(100, 1) == 0 and f(100, 129) == 0


def test_status_codes_before_any_launch():
    """Everything here is decided before a HIP call: bogus (never dereferenced) pointers are fine."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)

    def call(fn, real, act=p, lab=p, rows=100, C=13, loss=p, cnt=p, ws=p, wsb=1 << 20):
        return fn(act, lab, rows, C, real(0.01), None, None, loss, cnt, ws, wsb, None)
    f32, f64 = lib.conv3p_seg_head_f32, lib.conv3p_seg_head_f64
    for fn, real in ((f32, ctypes.c_float), (f64, ctypes.c_double)):
        assert call(fn, real, rows=0) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, C=1) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, act=None) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, lab=None) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, loss=None) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, cnt=None) == _lib.ERR_INVALID_ARGUMENT
        assert call(fn, real, C=129) == _lib.ERR_UNSUPPORTED
        assert call(fn, real, wsb=8) == _lib.ERR_WORKSPACE
        assert call(fn, real, ws=None) == _lib.ERR_WORKSPACE
    assert call(f64, ctypes.c_double, C=128) == _lib.ERR_UNSUPPORTED        # four fp64 tiles of 129 do not fit in LDS


def test_argument_checks():
    from pointwise_amd.seg_head import SegmentationHead
    with pytest.raises(op.Conv3pInvalidArgument, match="num_class must be an integer >= 2"):
        SegmentationHead(1, device="cpu")
    hd = SegmentationHead(13, device="cpu")
    act, lab = torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        hd.loss(act, lab)
    with pytest.raises(op.Conv3pInvalidArgument, match="must live on a HIP device"):
        hd.evaluate(act, lab)
    with pytest.raises(op.Conv3pInvalidArgument, match=r"\(batch_size, num_points, num_class\) activations"):
        hd.loss(torch.zeros(16, 13), lab)
    with pytest.raises(op.Conv3pInvalidArgument, match=r"\(batch_size, num_points, num_class\) activations"):
        hd.loss(torch.zeros(2, 8, 12), lab)
    with pytest.raises(op.Conv3pInvalidArgument, match="same batch size and number of points"):
        hd.loss(act, torch.zeros(2, 9, dtype=torch.int64))
    with pytest.raises(op.Conv3pInvalidArgument, match=r"\(batch_size, num_points\) labels"):
        hd.loss(act, torch.zeros(16, dtype=torch.int64))
    with pytest.raises(op.Conv3pInvalidArgument, match="labels must be int32 or int64"):
        hd.loss(act, torch.zeros(2, 8))
    with pytest.raises(op.Conv3pInvalidArgument, match="float32 or float64"):
        hd.loss(act.half(), lab)
    with pytest.raises(op.Conv3pInvalidArgument, match="global_points must be positive"):
        hd.loss(act, lab, global_points=0)
    with pytest.raises(op.Conv3pRuntimeError, match="no call yet"):
        hd.counts()


def test_summary_arithmetic_on_hand_made_counts():
    from pointwise_amd.seg_head import summarize
    # 4 classes; class 2 never seen but predicted 3 times; class 3 neither seen nor predicted
    seen, cc, predicted = [10, 5, 0, 0], [8, 1, 0, 0], [9, 3, 3, 0]
    counts = torch.tensor([9, 2] + seen + cc + predicted, dtype=torch.int64)
    s = summarize(counts, loss_total=3.0, batches=2, num_class=4)
    assert s["mean_loss"] == 1.5
    assert s["mean_accuracy"] == 9 / 15                                    # ignored points are in no ratio
    assert s["avg_class_accuracy"] == (8 / 10 + 1 / 5) / 2                 # the unseen classes are left out
    assert s["unseen_classes"] == [2, 3]
    assert s["iou"] == [8 / (10 + 9 - 8), 1 / (5 + 3 - 1), 0.0, None]
    assert s["mean_iou"] == (8 / 11 + 1 / 7 + 0.0) / 3
    assert s["invalid"] == 2 and s["points"] == 15 and s["batches"] == 2
    with pytest.raises(op.Conv3pInvalidArgument):
        summarize(counts[:-1], 0.0, 1, 4)


def test_ref_agrees_with_the_reference_loop():
    """seg_head_ref against a per-point Python loop written like train_scene_seg_s3dis.py:134-145 and a per-point
    softmax cross-entropy, R = 500 (labels partly outside [0, C): the ignored-row rule)."""
    rng = np.random.default_rng(5)
    B, N, C = 2, 250, 13
    act = selu(2.0 * rng.standard_normal((B, N, C)))
    act[0, :40] = np.round(act[0, :40] * 4) / 4                              # ties: first index wins
    gt = rng.integers(-1, C + 1, size=(B, N))
    r = seg_head_ref(act, gt)
    pred_label = np.argmax(act, axis=2)
    seen, corr, predicted = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    correct = invalid = 0
    loss, dact = 0.0, np.zeros_like(act)
    for i in range(B):
        for j in range(N):
            l = gt[i, j]
            if l < 0 or l >= C:
                invalid += 1
                continue
            seen[l] += 1
            corr[l] += (pred_label[i, j] == l)
            predicted[pred_label[i, j]] += 1
            correct += int(pred_label[i, j] == l)
            p = np.exp(act[i, j] - act[i, j].max())
            p /= p.sum()
            loss += -np.log(p[l])
            dact[i, j] = p
            dact[i, j, l] -= 1.0
    assert np.array_equal(r["pred"], pred_label)
    assert np.array_equal(r["counts"], np.concatenate([[correct, invalid], seen, corr, predicted]))
    assert invalid > 0 and correct > 0
    assert abs(r["loss"] - loss / (B * N)) <= 1e-12 * max(1.0, loss / (B * N))
    assert np.abs(r["dact"] * (B * N) - dact).max() <= 1e-12
    r1 = seg_head_ref(act, gt, points=1)
    assert abs(r1["loss"] - loss) <= 1e-12 * loss and np.abs(r1["dact"] - dact).max() <= 1e-12
