"""CPU tests (not gpu) of the classification model's fused tail: the C ABI exports and binds its three symbols under
the unchanged ABI version and profile-kind list, workspace sizing, the status codes decided before any HIP call, the
Python argument checks, the numpy Philox4x32-10 restatement against the generator's published known answers, the numpy
reference against oracle/head_numpy.py, and the summary arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import head_numpy
from pointwise_amd import _lib, conv3p_op as op, head

from tests.cls_tail_ref import cls_tail_ref, counters, keep_mask, philox4x32_10


def test_symbols_are_bound_and_abi_and_profile_kinds_are_unchanged():
    lib = _lib.load()
    for n in ("conv3p_cls_tail_workspace_bytes", "conv3p_cls_tail_f32", "conv3p_cls_tail_step_f32"):
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"
    assert lib.conv3p_abi_version() == 5 and _lib.ABI_VERSION == 5


def test_public_interface_exists():
    for n in ("forward_backward", "evaluate", "counts", "accumulate", "summary"):
        assert callable(getattr(head.ClassificationHead, n))
    assert callable(head.classification_tail)
    assert "handful of elementwise torch ops" not in head.__doc__


def test_workspace_bytes():
    f = _lib.load().conv3p_cls_tail_workspace_bytes
    by_m = [f(m, 512, 40) for m in (1, 3, 32, 33, 128)]
    by_c = [f(32, 512, c) for c in (2, 10, 13, 40, 128)]
    for sizes in (by_m, by_c):
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert f(32, 512, 40) >= 4 * 32 * (512 + 40) + 12 * 32              # drop, dz, a loss and a prediction per row
    assert f(1, 8, 2) > 0 and f(128, 1024, 128) > 0
    for M, H, C in ((0, 512, 40), (129, 512, 40), (32, 0, 40), (32, 12, 40), (32, 1032, 40), (32, 512, 1), (32, 512, 129)):
        assert f(M, H, C) == 0


def _call(step=False, **kw):
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    a = dict(fc1=p, W2=p, b2=p, labels=p, M=32, H=512, C=40, training=1, rate=0.5, keep_mask=None, seed=1, step=2,
             scale=1 / 32, logits=p, pred=None, dfc1=p, g0=p, g1=p, keep_out=None, loss=p, counts=p, ws=p, wsb=1 << 20)
    a.update(kw)
    head_ = (a["fc1"], a["W2"], a["b2"], a["labels"], a["M"], a["H"], a["C"], a["training"], a["rate"], a["keep_mask"],
             a["seed"], a["step"], a["scale"], a["logits"], a["pred"], a["dfc1"], a["g0"], a["g1"])
    tail = (a["keep_out"], a["loss"], a["counts"], a["ws"], a["wsb"], None)
    if step:
        return lib.conv3p_cls_tail_step_f32(*head_, 0.001, 0.9, *tail)
    return lib.conv3p_cls_tail_f32(*head_, *tail)


@pytest.mark.parametrize("step", [False, True])
def test_status_codes_before_any_launch(step):
    """Everything here is decided before a HIP call: bogus (never dereferenced) pointers are fine."""
    INV, UNS, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    for name in ("fc1", "W2", "b2", "labels", "logits", "loss", "counts"):
        assert _call(step, **{name: None}) == INV
    assert _call(step, M=0) == INV
    assert _call(step, C=1) == INV
    for rate in (-0.1, 1.0, 1.5, float("nan")):
        assert _call(step, rate=rate) == INV
    assert _call(step, rate=1.5, training=0, wsb=8) == WS                    # the rate is not looked at in evaluation
    assert _call(step, g0=None) == INV and _call(step, g1=None) == INV       # one gradient / accumulator without the other
    assert _call(step, fc1=ctypes.c_void_p(4100)) == INV                     # 16-byte loads
    for kw in (dict(M=129), dict(H=12), dict(H=1032), dict(C=129)):
        assert _call(step, **kw) == UNS
        assert _call(step, wsb=0, **kw) == UNS                               # the order of the seg head: before WORKSPACE
    assert _call(step, M=0, C=129) == INV
    assert _call(step, wsb=8) == WS and _call(step, ws=None) == WS
    assert _call(step, ws=ctypes.c_void_p(4097)) == WS
    if step:
        assert _call(step, dfc1=None) == INV                                 # no gradient to step with
    else:
        assert _call(step, dfc1=None, g0=None, g1=None, wsb=8) == WS         # evaluation is legal: gets as far as the scratch


def test_python_argument_checks():
    f = head.classification_tail
    fc1, W2, b2 = torch.zeros(4, 16), torch.zeros(16, 5), torch.zeros(5)
    lab = torch.zeros(4, dtype=torch.int64)
    bad = [dict(fc1=torch.zeros(4, 8)), dict(fc1=torch.zeros(4, 16, dtype=torch.float64)), dict(b2=torch.zeros(4)),
           dict(labels=torch.zeros(3, dtype=torch.int64)), dict(labels=torch.zeros(4)), dict(rate=1.0), dict(rate=-0.5),
           dict(W2=torch.zeros(16, 1), b2=torch.zeros(1)), dict(fc1=torch.zeros(0, 16), labels=lab[:0]),
           dict(keep_mask=torch.zeros(4, 8)), dict(accum_W2=torch.zeros(16, 5)), dict(seed=-1), dict(step=1 << 64),
           dict(accum_W2=torch.zeros(16, 5), accum_b2=torch.zeros(5)),      # no lr / momentum
           dict(fc1=np.zeros((4, 16), dtype=np.float32)),
           dict()]                                                           # CPU tensors: no CPU path
    for kw in bad:
        a = dict(fc1=fc1, W2=W2, b2=b2, labels=lab)
        a.update(kw)
        with pytest.raises(op.Conv3pInvalidArgument):
            f(a.pop("fc1"), a.pop("W2"), a.pop("b2"), a.pop("labels"), **a)
    hd = head.ClassificationHead(4, num_class=5, hidden=16, device="cpu")
    feat = torch.zeros(3, 4, 36)
    for args in ((torch.zeros(3, 4, 35), lab[:3]), (feat, lab), (feat, torch.zeros(3, 1, dtype=torch.int64)), (feat, [0, 1, 2])):
        with pytest.raises(op.Conv3pInvalidArgument):
            hd.forward_backward(*args)
        with pytest.raises(op.Conv3pInvalidArgument):
            hd.evaluate(*args)
    with pytest.raises(op.Conv3pInvalidArgument):
        hd.forward_backward(feat, lab[:3], global_batch=0)
    with pytest.raises(op.Conv3pRuntimeError):
        hd.counts()
    with pytest.raises(op.Conv3pRuntimeError):
        hd.summary()


def test_philox_known_answers():
    """The known-answer vectors published with the generator (Random123's kat_vectors, philox4x32 10 rounds)."""
    h = lambda s: np.array([int(w, 16) for w in s.split()], dtype=np.uint32)
    ones = "ffffffff ffffffff ffffffff ffffffff"
    for ctr, key, want in (("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           (ones, "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert np.array_equal(philox4x32_10(h(ctr), h(key)), h(want))
    # vectorised over leading axes
    got = philox4x32_10(np.stack([h("0 0 0 0"), h(ones)]), np.stack([h("0 0"), h("ffffffff ffffffff")]))
    assert np.array_equal(got[1], h("408f276d 41c83b0e a20bc7c6 6d5451fd"))


def test_keep_mask_restatement():
    k = keep_mask(1234, 5, 16, 1024, 0.5)
    assert k.dtype == np.uint8 and set(np.unique(k)) == {0, 1}
    assert abs(k.mean() - 0.5) <= 0.02                                        # 16 384 draws
    assert np.array_equal(keep_mask(1234, 5, 1, 1024, 0.5, rows=[7]), k[7:8])  # a function of (seed, step, m, h) only
    assert not np.array_equal(keep_mask(1234, 5 + (1 << 32), 16, 1024, 0.5), k)
    assert not np.array_equal(keep_mask(1234 + (1 << 32), 5, 16, 1024, 0.5), k)
    assert abs(keep_mask(9, 0, 16, 1024, 0.3).mean() - 0.7) <= 0.02


@pytest.mark.parametrize("rate", [0.5, 0.3])
def test_reference_agrees_with_head_numpy(rate):
    rng = np.random.default_rng(3)
    B, K, H, C = 6, 20, 16, 10
    feat, W1, b1 = rng.standard_normal((B, K)), rng.standard_normal((K, H)) / 4, rng.standard_normal(H) / 4
    W2, b2 = rng.standard_normal((H, C)) / 4, rng.standard_normal(C) / 4
    labels = rng.integers(0, C, size=B)
    mask = (rng.random((B, H)) < 1 - rate).astype(np.float64)
    r = head_numpy.head_forward_backward(feat, W1, b1, W2, b2, labels, rate, mask)
    t = cls_tail_ref(r["fc1"], W2, b2, labels, rate, mask)
    a = head_numpy.dropout_selu(r["fc1"], rate, mask)[1]
    # dfc1 = ddrop * a * mask: recovered from head_numpy through the gradient of fc1's pre-activation
    dview, _, _ = head_numpy.fully_connected_grad(feat, W1, r["fc1"], t["dfc1"])
    assert np.abs(t["logits"] - r["logits"]).max() <= 1e-12
    assert abs(t["loss_sum"] / B - r["loss"]) <= 1e-12
    assert np.abs(t["dW2"] - r["dW2"]).max() <= 1e-12 and np.abs(t["db2"] - r["db2"]).max() <= 1e-12
    ddrop = head_numpy.fully_connected_grad(t["drop"], W2, r["logits"], r["dlogits"])[0]
    assert np.abs(t["dfc1"] - ddrop * a * mask).max() <= 1e-12
    assert np.abs(dview.reshape(feat.shape) - r["dfeat"]).max() <= 1e-12
    # ignored rows and the counters
    lab2 = labels.copy()
    lab2[1], lab2[4] = -1, C
    u = cls_tail_ref(r["fc1"], W2, b2, lab2, rate, mask)
    assert u["row_loss"][1] == 0 and u["row_loss"][4] == 0 and not u["dfc1"][[1, 4]].any() and u["counts"][1] == 2
    assert np.array_equal(u["row_loss"][[0, 2, 3, 5]], t["row_loss"][[0, 2, 3, 5]])
    assert u["counts"][2:2 + C].sum() == B - 2 and t["counts"][2 + 2 * C:].sum() == B
    assert np.array_equal(counters([1, 1, 0, 2], [1, 0, 0, 3], 3), [2, 1, 2, 1, 0, 1, 1, 0, 1, 2, 0])


def test_summary_arithmetic():
    hd = head.ClassificationHead(4, num_class=3, hidden=16, device="cpu")
    # two batches: {correct, invalid, seen[3], correct_class[3], predicted[3]}
    for cnt, loss in (([3, 1, 2, 2, 0, 2, 1, 0, 3, 1, 0], 1.5), ([1, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0], 0.5)):
        hd._counts = torch.tensor(cnt, dtype=torch.int64)
        hd._loss = torch.tensor(loss, dtype=torch.float64)
        hd.accumulate()
    assert hd.counts()["seen"].tolist() == [1, 2, 0] and int(hd.counts()["correct"]) == 1
    s = hd.summary()
    assert s["mean_loss"] == 1.0 and s["batches"] == 2 and s["invalid"] == 1 and s["points"] == 7
    assert s["mean_accuracy"] == 4 / 7
    assert s["avg_class_accuracy"] == (2 / 3 + 2 / 4) / 2 and s["unseen_classes"] == [2]
    with pytest.raises(op.Conv3pRuntimeError):
        hd.summary()                                                         # reset
