"""CPU tests (not gpu) of the weighted segmentation head's host side: the new C-ABI symbols, workspace sizing, the
status codes decided before any HIP call, SegmentationHead's new argument checks, class_weights_from_counts, the
confusion part of summarize(), and -- independent of the code under test -- the numpy restatement
tests/seg_weighted_ref.py against torch.nn.functional.cross_entropy in float64."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op

from tests.seg_head_ref import seg_head_ref, selu
from tests.seg_weighted_ref import confusion_ref, seg_weighted_ref, weight_totals

NEW = ("conv3p_seg_head_weighted_workspace_bytes", "conv3p_seg_weight_total_f32", "conv3p_seg_weight_total_f64",
       "conv3p_seg_head_weighted_f32", "conv3p_seg_head_weighted_f64", "conv3p_seg_confusion_workspace_bytes",
       "conv3p_seg_confusion")


def test_symbols_are_bound_and_nothing_pinned_moved():
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"
    assert lib.conv3p_abi_version() == 5
    import pointwise_amd
    from pointwise_amd import seg_head
    assert pointwise_amd.class_weights_from_counts is seg_head.class_weights_from_counts
    assert "class_weights_from_counts" in pointwise_amd.__all__


def test_workspace_bytes():
    lib = _lib.load()
    plain, weighted, conf = (lib.conv3p_seg_head_workspace_bytes, lib.conv3p_seg_head_weighted_workspace_bytes,
                             lib.conv3p_seg_confusion_workspace_bytes)
    for C in (2, 13, 41, 128):
        for R in (1, 64, 1000, 65536, 70000, 1 << 30):
            w = weighted(R, C)
            assert w % 256 == 0 and w >= plain(R, C)                        # the main pass's records
            assert w >= min((R + 1023) // 1024, 256) * 16                   # the pre-pass's {double, int64} records
            blocks = min((R + 1023) // 1024, 64)                            # the confusion kernel's grid cap
            c = conf(R, C)
            assert c % 256 == 0 and blocks * 4 * C * C <= c < blocks * 4 * C * C + 256
    assert conf(1 << 30, 128) == 64 * 4 * 128 * 128                         # 4 MB: the cap holds whatever the rows
    for f in (weighted, conf):
        assert f(0, 13) == 0 and f(100, 1) == 0 and f(100, 129) == 0


def test_status_codes_before_any_launch():
    """Everything here is decided before a HIP call: bogus (never dereferenced) pointers are fine."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    BIG = 1 << 24

    def head(fn, real, act=p, lab=p, rows=100, C=13, cw=p, pw=p, ls=0.1, den=p, loss=p, cnt=p, ws=p, wsb=BIG):
        return fn(act, lab, rows, C, cw, pw, ls, real(0.01), den, None, None, loss, cnt, ws, wsb, None)

    def total(fn, lab=p, rows=100, C=13, out=p, ws=p, wsb=BIG):
        return fn(lab, rows, C, p, p, out, ws, wsb, None)

    def conf(lab=p, pred=p, rows=100, C=13, out=p, ws=p, wsb=BIG):
        return lib.conv3p_seg_confusion(lab, pred, rows, C, out, ws, wsb, None)

    for sfx, real, cmax in (("f32", ctypes.c_float, 128), ("f64", ctypes.c_double, 79)):
        fn = getattr(lib, "conv3p_seg_head_weighted_" + sfx)
        for kw in (dict(rows=0), dict(C=1), dict(act=None), dict(lab=None), dict(loss=None), dict(cnt=None),
                   dict(ls=-0.01), dict(ls=1.0), dict(ls=1.5), dict(ls=float("nan")), dict(ls=float("inf"))):
            assert head(fn, real, **kw) == _lib.ERR_INVALID_ARGUMENT, kw
        # ... also on the route that is the plain head (no weights, no smoothing, no denominator)
        for kw in (dict(rows=0), dict(C=1), dict(act=None), dict(cnt=None)):
            assert head(fn, real, cw=None, pw=None, ls=0.0, den=None, **kw) == _lib.ERR_INVALID_ARGUMENT, kw
        assert head(fn, real, C=cmax + 1) == _lib.ERR_UNSUPPORTED
        assert head(fn, real, cw=None, pw=None, ls=0.0, den=None, C=cmax + 1) == _lib.ERR_UNSUPPORTED
        assert head(fn, real, wsb=8) == _lib.ERR_WORKSPACE and head(fn, real, ws=None) == _lib.ERR_WORKSPACE
        assert head(fn, real, cw=None, pw=None, ls=0.0, den=None, wsb=8) == _lib.ERR_WORKSPACE
        tot = getattr(lib, "conv3p_seg_weight_total_" + sfx)
        for kw in (dict(rows=0), dict(C=1), dict(lab=None), dict(out=None)):
            assert total(tot, **kw) == _lib.ERR_INVALID_ARGUMENT, kw
        assert total(tot, C=cmax + 1) == _lib.ERR_UNSUPPORTED
        assert total(tot, wsb=8) == _lib.ERR_WORKSPACE and total(tot, ws=None) == _lib.ERR_WORKSPACE
    for kw in (dict(rows=0), dict(C=1), dict(lab=None), dict(pred=None), dict(out=None)):
        assert conf(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert conf(C=129) == _lib.ERR_UNSUPPORTED
    assert conf(wsb=8) == _lib.ERR_WORKSPACE and conf(ws=None) == _lib.ERR_WORKSPACE


def test_argument_checks():
    from pointwise_amd.seg_head import SegmentationHead
    bad = op.Conv3pInvalidArgument
    for ls in (-0.1, 1.0, 2.0, float("nan"), "0.1"):
        with pytest.raises(bad, match=r"label_smoothing must be in \[0, 1\)"):
            SegmentationHead(13, device="cpu", label_smoothing=ls)
    with pytest.raises(bad, match="reduction must be one of"):
        SegmentationHead(13, device="cpu", reduction="mean")
    with pytest.raises(bad, match="class_weights must have num_class entries"):
        SegmentationHead(13, device="cpu", class_weights=torch.ones(12))
    with pytest.raises(bad, match="class_weights must have num_class entries"):
        SegmentationHead(13, device="cpu", class_weights=torch.ones(1, 13))
    with pytest.raises(bad, match="class_weights must be float32 or float64"):
        SegmentationHead(13, device="cpu", class_weights=torch.ones(13, dtype=torch.int64))
    with pytest.raises(bad, match="class_weights must be on the host or on the head's device"):
        SegmentationHead(13, device="cpu", class_weights=torch.ones(13, device="meta"))
    hd = SegmentationHead(13, device="cpu", class_weights=[1.0] * 12 + [0.5], label_smoothing=0.1, reduction="sum_weights")
    assert hd.class_weights.dtype == torch.float64 and float(hd.class_weights[12]) == 0.5
    assert SegmentationHead(13, device="cpu", class_weights=np.ones(13, np.float32)).class_weights.shape == (13,)
    act, lab = torch.zeros(2, 8, 13), torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(bad, match=r"\(batch_size, num_points\) point_weights"):
        hd.loss(act, lab, point_weights=torch.ones(2, 9))
    with pytest.raises(bad, match=r"\(batch_size, num_points\) point_weights"):
        hd.evaluate(act, lab, point_weights=torch.ones(16))
    with pytest.raises(bad, match="point_weights must have the activations' dtype"):
        hd.loss(act, lab, point_weights=torch.ones(2, 8, dtype=torch.float64))
    with pytest.raises(bad, match="point_weights must be on the labels' device"):
        hd.loss(act, lab, point_weights=torch.ones(2, 8, device="meta"))
    with pytest.raises(bad, match="point_weights must be a tensor"):
        hd.loss(act, lab, point_weights=[[1.0] * 8] * 2)
    with pytest.raises(bad, match="denominator must be a float64 tensor of one element"):
        hd.loss(act, lab, denominator=torch.ones(2, dtype=torch.float64))
    with pytest.raises(bad, match="denominator must be a float64 tensor of one element"):
        hd.loss(act, lab, denominator=torch.ones(()))
    with pytest.raises(bad, match="denominator must be a float64 tensor of one element"):
        hd.loss(act, lab, denominator=3.0)
    with pytest.raises(bad, match="denominator must be on the activations' device"):
        hd.loss(act, lab, denominator=torch.ones((), dtype=torch.float64, device="meta"))
    with pytest.raises(bad, match="global_points goes with reduction 'points'"):
        hd.loss(act, lab, global_points=16)
    with pytest.raises(bad, match="denominator= goes with reduction"):
        SegmentationHead(13, device="cpu").loss(act, lab, denominator=torch.ones((), dtype=torch.float64))
    with pytest.raises(bad, match="reduction 'points' has no weight total"):
        SegmentationHead(13, device="cpu").weight_total(lab)
    with pytest.raises(bad, match="must live on a HIP device"):
        hd.weight_total(lab)
    # everything valid: the only complaint left is the device (there is no CPU path)
    with pytest.raises(bad, match="must live on a HIP device"):
        hd.loss(act, lab, point_weights=torch.ones(2, 8), denominator=torch.ones((), dtype=torch.float64))
    with pytest.raises(bad, match="must live on a HIP device"):
        hd.evaluate(act, lab, point_weights=torch.ones(2, 8), confusion=True)


def make(R, C, seed):
    rng = np.random.default_rng(seed)
    act = selu(2.0 * rng.standard_normal((R, C)))
    labels = rng.integers(-1, C, size=R)                                    # -1: ignored points
    cw = rng.uniform(0.25, 4.0, size=C)
    cw[rng.integers(0, C)] = 0.0                                            # a class that does not count
    pw = rng.uniform(0.0, 2.0, size=R)
    pw[rng.integers(0, R, size=R // 10)] = 0.0
    return act, labels, cw, pw


@pytest.mark.parametrize("C", [2, 13, 41])
def test_ref_agrees_with_torch_class_weights_and_ignore_index(C):
    """F.cross_entropy(weight=, ignore_index=-1) at ls = 0: "mean" is sum_weights, "sum" the unnormalised sum; the
    gradients through autograd."""
    import torch.nn.functional as F
    R = 300
    act, labels, cw, _ = make(R, C, 40 + C)
    x = torch.from_numpy(act).requires_grad_(True)
    t, wt = torch.from_numpy(labels), torch.from_numpy(cw)
    mean = F.cross_entropy(x, t, weight=wt, ignore_index=-1, reduction="mean")
    (gmean,) = torch.autograd.grad(mean, x)
    total = F.cross_entropy(x, t, weight=wt, ignore_index=-1, reduction="sum")
    (gsum,) = torch.autograd.grad(total, x)
    r = seg_weighted_ref(act, labels, class_weights=cw, reduction="sum_weights")
    assert r["denominator"] == r["weight_sum"] > 0 and (labels == -1).sum() > 0
    assert abs(r["loss"] - mean.item()) <= 1e-12 * max(1.0, abs(mean.item()))
    assert np.abs(r["dact"] - gmean.numpy()).max() <= 1e-14
    assert abs(r["loss_sum"] - total.item()) <= 1e-12 * total.item()
    r1 = seg_weighted_ref(act, labels, class_weights=cw, reduction="points", points=1)
    assert abs(r1["loss"] - total.item()) <= 1e-12 * total.item()
    assert np.abs(r1["dact"] - gsum.numpy()).max() <= 1e-12
    # TensorFlow's default divides the same sum by the rows that count
    rn = seg_weighted_ref(act, labels, class_weights=cw, reduction="nonzero_weights")
    nz = int(((labels >= 0) & (cw[np.maximum(labels, 0)] != 0)).sum())
    assert rn["denominator"] == nz == weight_totals(labels, C, cw)[1] and 0 < nz < (labels >= 0).sum()
    assert abs(rn["loss"] - total.item() / nz) <= 1e-12 * total.item() / nz


@pytest.mark.parametrize("C", [2, 13, 41])
def test_ref_agrees_with_torch_label_smoothing(C):
    """Without class weights torch's smoothing is TensorFlow's: (1 - ls) onehot + ls / C."""
    import torch.nn.functional as F
    R = 300
    act, labels, _, pw = make(R, C, 60 + C)
    labels = np.abs(labels)                                                 # all valid: mean = sum / R
    x = torch.from_numpy(act).requires_grad_(True)
    t = torch.from_numpy(labels)
    mean = F.cross_entropy(x, t, label_smoothing=0.1)
    (g,) = torch.autograd.grad(mean, x)
    r = seg_weighted_ref(act, labels, label_smoothing=0.1)
    assert abs(r["loss"] - mean.item()) <= 1e-12 * mean.item()
    assert np.abs(r["dact"] - g.numpy()).max() <= 1e-14
    # per-point weights: the weighted sum of torch's per-point smoothed losses
    rows = F.cross_entropy(x, t, label_smoothing=0.1, reduction="none")
    wsum = (rows * torch.from_numpy(pw)).sum()
    (gw,) = torch.autograd.grad(wsum, x)
    rp = seg_weighted_ref(act, labels, point_weights=pw, label_smoothing=0.1, reduction="nonzero_weights")
    nz = int((pw != 0).sum())
    assert rp["denominator"] == nz and 0 < nz < R
    assert abs(rp["loss"] - wsum.item() / nz) <= 1e-12 * wsum.item() / nz
    assert np.abs(rp["dact"] - gw.numpy() / nz).max() <= 1e-14


def test_ref_with_everything_off_is_the_plain_ref_and_zero_denominators():
    act, labels, cw, pw = make(200, 13, 7)
    a, b = seg_weighted_ref(act, labels), seg_head_ref(act, labels)
    assert abs(a["loss"] - b["loss"]) <= 1e-14 and np.abs(a["dact"] - b["dact"]).max() <= 1e-16
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["pred"], b["pred"])
    conf = a["confusion"]
    C = 13
    assert np.array_equal(conf.sum(axis=1), b["counts"][2:2 + C]) and np.array_equal(np.diag(conf), b["counts"][2 + C:2 + 2 * C])
    assert np.array_equal(conf.sum(axis=0), b["counts"][2 + 2 * C:]) and conf.sum() == (labels >= 0).sum()
    assert np.array_equal(confusion_ref([0, 1, 1, 5, -1], [1, 1, 0, 1, 1], 2), [[0, 1], [1, 1]])
    for red in ("nonzero_weights", "sum_weights"):
        z = seg_weighted_ref(act, labels, point_weights=np.zeros(200), reduction=red)
        assert z["denominator"] == 0 and z["loss"] == 0.0 and not z["dact"].any()
        z = seg_weighted_ref(act, np.full(200, 13), class_weights=cw, reduction=red)
        assert z["denominator"] == 0 and z["loss"] == 0.0 and not z["dact"].any() and z["counts"][1] == 200
    half = seg_weighted_ref(act, labels, cw, pw, 0.1, "sum_weights")
    twice = seg_weighted_ref(act, labels, cw, pw, 0.1, "sum_weights", denominator=2 * half["denominator"])
    assert np.allclose(twice["dact"] * 2, half["dact"], rtol=1e-15, atol=0) and abs(twice["loss"] * 2 - half["loss"]) < 1e-15


def test_class_weights_from_counts():
    from pointwise_amd import class_weights_from_counts
    seen = [50, 30, 0, 20]
    w = class_weights_from_counts(seen)
    assert w.dtype == torch.float64 and w.tolist() == [100 / 150, 100 / 90, 0.0, 100 / 60]
    assert abs(sum(x * n for x, n in zip(w.tolist(), seen)) - 100) < 1e-12   # weighted and unweighted counts agree
    assert class_weights_from_counts(torch.tensor(seen), kind="inverse").tolist() == w.tolist()
    m = class_weights_from_counts(seen, kind="median_frequency")
    assert m.tolist() == [30 / 50, 1.0, 0.0, 30 / 20]                        # median of {20, 30, 50}
    m2 = class_weights_from_counts([10, 40, 20, 30], kind="median_frequency")
    assert m2.tolist() == [2.5, 25 / 40, 25 / 20, 25 / 30]                   # even number of classes: (20 + 30) / 2
    for bad, kw in (([0, 0, 0], {}), ([5], {}), ([3, -1], {}), ([1, 2], dict(kind="sqrt"))):
        with pytest.raises(op.Conv3pInvalidArgument):
            class_weights_from_counts(bad, **kw)


def test_summarize_carries_the_confusion_matrix():
    from pointwise_amd.seg_head import summarize
    conf = [[8, 2, 0], [1, 4, 0], [0, 0, 0]]                                  # [label][pred]; class 2 never seen
    seen, cc, predicted = [10, 5, 0], [8, 4, 0], [9, 6, 0]
    counts = [12, 3] + seen + cc + predicted
    s = summarize(counts, 1.0, 2, 3, confusion=torch.tensor(conf))
    assert s["confusion"] == conf and all(isinstance(v, int) for row in s["confusion"] for v in row)
    assert [sum(r) for r in s["confusion"]] == seen and [s["confusion"][k][k] for k in range(3)] == cc
    assert [sum(r[k] for r in s["confusion"]) for k in range(3)] == predicted
    assert s["iou"] == [8 / 11, 4 / 7, None] and s["mean_loss"] == 0.5
    assert "confusion" not in summarize(counts, 1.0, 2, 3)
    with pytest.raises(op.Conv3pInvalidArgument, match="num_class x num_class"):
        summarize(counts, 1.0, 2, 3, confusion=[[1, 2], [3, 4]])
