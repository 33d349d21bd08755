"""The classification model's fused tail (conv3p_cls_tail_f32 / _step_f32, head.classification_tail) on the GPU.

Against the float64 restatement tests/cls_tail_ref.py (oracle/head_numpy.py's layers), rel = max|delta| / max(1, max|ref|)
as tests/test_head.py:
  bound 1  rel <= 2e-4, the head tests' bound;
  bound 2  rel <= max(4 * rel of the parent's composition on the same inputs, 1e-6), where the parent's composition
           (fully_connected / dropout_selu / loss / fully_connected_grad) exists, i.e. num_class % 8 == 0: both are fp32
           sums of at most 1024 terms in different orders.
Everything else is exact: predictions, counters, the Philox mask, bitwise reproducibility, row independence, and the
_step form against the plain call followed by momentum_step."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.cls_tail_ref import cls_tail_ref, counters, keep_mask

TOL = 2e-4
MS, HS, CS = (1, 3, 32, 33, 128), (8, 512, 1024), (2, 10, 13, 40, 128)
OUTS = ("logits", "loss", "dfc1", "dW2", "db2")


def rel(got, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(1.0, np.abs(want).max()))


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def inputs(M, H, C, seed, rate=0.5):
    rng = np.random.default_rng(seed)
    fc1 = rng.standard_normal((M, H)).astype(np.float32)
    W2 = (rng.standard_normal((H, C)) / np.sqrt(H)).astype(np.float32)
    b2 = (rng.standard_normal(C) * 0.1).astype(np.float32)
    labels = rng.integers(0, C, size=M).astype(np.int32)
    mask = (rng.random((M, H)) < 1.0 - rate).astype(np.float32)
    return fc1, W2, b2, labels, mask


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def parent_composition(head, t, fc1, W2, b2, labels, rate, mask):
    """The parent's path through the same stage, on the device: what ClassificationHead.forward's tail, loss() and
    backward()'s tail do."""
    import torch
    drop, m = head.dropout_selu(t(fc1), rate, mask is not None, t(mask) if mask is not None else None)
    fc2 = head.fully_connected(drop, t(W2), t(b2), selu=True)
    logp = torch.log_softmax(fc2, dim=1)
    idx = t(labels).long().unsqueeze(1)
    loss = -(logp.gather(1, idx)).mean()
    dlogits = torch.softmax(fc2, dim=1)
    dlogits.scatter_add_(1, idx, -torch.ones_like(idx, dtype=dlogits.dtype))
    dlogits = dlogits / float(fc2.shape[0])
    ddrop, dW2, db2 = head.fully_connected_grad(drop, t(W2), fc2, dlogits, selu=True)
    dfc1 = ddrop * (head.dropout_selu_constants(rate)[0] * m) if m is not None else ddrop
    return {"logits": fc2, "loss": loss, "dfc1": dfc1, "dW2": dW2, "db2": db2}


@pytest.mark.gpu
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("mode", ["train0.5", "train0.3", "eval"])
def test_matches_float64(dev, mode, H):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    training = mode != "eval"
    rate = float(mode[5:]) if training else 0.5
    worst, worst_ratio, failures = {}, 0.0, []
    for M, C in itertools.product(MS, CS):
        fc1, W2, b2, labels, mask = inputs(M, H, C, 1000 * M + H + C, rate)
        ref = cls_tail_ref(fc1, W2, b2, labels, rate, mask if training else None)
        ref["loss"] = ref["loss_sum"] / M
        out = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), rate=rate, training=training,
                                       keep_mask=t(mask) if training else None, need_grad=training)
        got = {k: out[k] for k in ("logits", "dfc1", "dW2", "db2")}
        got["loss"] = out["loss_sum"] / M
        names = OUTS if training else ("logits", "loss")
        if not training:
            assert out["dfc1"] is None and out["dW2"] is None and out["db2"] is None
        par = parent_composition(head, t, fc1, W2, b2, labels, rate, mask if training else None) if C % 8 == 0 else None
        for k in names:
            e = rel(got[k].cpu().numpy(), ref[k])
            worst[k] = max(worst.get(k, 0.0), e)
            if not e <= TOL:
                failures.append(("bound 1", M, H, C, k, e))
            if par is not None:
                ep = rel(par[k].cpu().numpy(), ref[k])
                worst_ratio = max(worst_ratio, e / max(ep, 2.5e-7))
                if not e <= max(4.0 * ep, 1e-6):
                    failures.append(("bound 2", M, H, C, k, e, ep))
        assert np.array_equal(out["pred"].cpu().numpy(), np.argmax(out["logits"].cpu().numpy(), axis=1))
        assert np.array_equal(out["counts"].cpu().numpy(), counters(out["pred"].cpu().numpy(), labels, C))
    print("cls_tail %s H=%d largest rel distance to float64: %s; largest fused / max(parent, 2.5e-7): %.2f"
          % (mode, H, " ".join("%s %.2e" % kv for kv in sorted(worst.items())), worst_ratio))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("C", [10, 40])
def test_predictions_counters_and_ignored_rows(dev, C):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    M, H = 32, 512
    fc1, W2, b2, labels, mask = inputs(M, H, C, 77 + C)
    labels[[2, 9, 30]] = (-1, C, -5)
    labels[[4, 5]] = labels[3]                                       # a class seen more than once
    out = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), keep_mask=t(mask))
    ref = cls_tail_ref(fc1, W2, b2, labels, 0.5, mask)
    logits, pred = out["logits"].cpu().numpy(), out["pred"].cpu().numpy()
    assert np.array_equal(pred, np.argmax(logits, axis=1))
    want = counters(pred, labels, C)
    assert np.array_equal(out["counts"].cpu().numpy(), want) and want[1] == 3 and want[2:2 + C].sum() == M - 3
    dfc1 = out["dfc1"].cpu().numpy()
    assert not dfc1[[2, 9, 30]].view(np.uint32).any()                # exactly +0
    assert abs(float(out["loss_sum"]) - ref["loss_sum"]) <= TOL * max(1.0, abs(ref["loss_sum"]))
    for k in ("dfc1", "dW2", "db2"):
        assert rel(out[k].cpu().numpy(), ref[k]) <= TOL
    # evaluation on the same batch: the same counters' layout, no dropout
    ev = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), training=False, need_grad=False)
    assert np.array_equal(ev["counts"].cpu().numpy(), counters(ev["pred"].cpu().numpy(), labels, C))
    assert rel(ev["logits"].cpu().numpy(), cls_tail_ref(fc1, W2, b2, labels, 0.5, None)["logits"]) <= TOL


@pytest.mark.gpu
def test_device_drawn_mask_is_the_numpy_philox_mask(dev):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    H, C = 1024, 40
    fc1, W2, b2, labels, _ = inputs(128, H, C, 5)
    for seed, step in itertools.product((1234, (1 << 40) + 77), (3, (1 << 32) + 5)):
        out = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), seed=seed, step=step, need_keep=True)
        keep = out["keep"].cpu().numpy()
        want = keep_mask(seed, step, 128, H, 0.5)
        assert keep.dtype == np.uint8 and np.array_equal(keep, want)
        assert abs(keep.mean() - 0.5) <= 0.02
        one = head.classification_tail(t(fc1[:1]), t(W2), t(b2), t(labels[:1]), seed=seed, step=step, need_keep=True)
        assert np.array_equal(one["keep"].cpu().numpy(), want[:1])                  # not a function of M
    a = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), seed=1234, step=3, need_keep=True)["keep"]
    b = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), seed=1234, step=4, need_keep=True)["keep"]
    assert not torch.equal(a, b)
    k3 = head.classification_tail(t(fc1[:3, :512].copy()), t(W2[:512].copy()), t(b2), t(labels[:3]), rate=0.3, seed=9, step=1,
                                  need_keep=True)["keep"]
    assert np.array_equal(k3.cpu().numpy(), keep_mask(9, 1, 3, 512, 0.3))


@pytest.mark.gpu
@pytest.mark.parametrize("M,H,C", [(32, 512, 40), (33, 1024, 13)])
def test_drawn_run_equals_explicit_mask_run_and_is_reproducible(dev, M, H, C):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    fc1, W2, b2, labels, _ = inputs(M, H, C, 11)
    args = (t(fc1), t(W2), t(b2), t(labels))
    a = head.classification_tail(*args, seed=42, step=7, need_keep=True)
    b = head.classification_tail(*args, keep_mask=a["keep"].to(torch.float32), need_keep=True)
    c = head.classification_tail(*args, seed=42, step=7, need_keep=True)
    for other in (b, c):
        for k in ("logits", "dfc1", "dW2", "db2", "loss_sum"):
            assert same_bits(a[k], other[k]), k
        for k in ("pred", "counts", "keep"):
            assert torch.equal(a[k], other[k]), k


@pytest.mark.gpu
def test_rows_do_not_depend_on_their_batch(dev):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    M, H, C = 32, 512, 40
    fc1, W2, b2, labels, mask = inputs(M, H, C, 13)
    full = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), keep_mask=t(mask), grad_scale=1.0 / M)
    for m in (0, 5, 31):
        one = head.classification_tail(t(fc1[m:m + 1].copy()), t(W2), t(b2), t(labels[m:m + 1].copy()),
                                       keep_mask=t(mask[m:m + 1].copy()), grad_scale=1.0 / M)
        assert same_bits(one["logits"][0], full["logits"][m]) and same_bits(one["dfc1"][0], full["dfc1"][m])
        assert int(one["pred"][0]) == int(full["pred"][m])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [40, 10])
def test_step_form_equals_plain_call_then_momentum_step(dev, C):
    import torch
    from pointwise_amd import head, optim
    t = lambda a: torch.from_numpy(a).to(dev)
    M, H = 32, 512
    lr, mom = 0.01, 0.9
    _, W2, b2, _, _ = inputs(M, H, C, 17)
    Wa, ba, Wb, bb = t(W2), t(b2), t(W2), t(b2)
    acc_a = [torch.zeros_like(Wa), torch.zeros_like(ba)]
    acc_b = [torch.zeros_like(Wb), torch.zeros_like(bb)]
    for step in range(3):
        fc1, _, _, labels, _ = inputs(M, H, C, 100 + step)
        a = head.classification_tail(t(fc1), Wa, ba, t(labels), seed=3, step=step)
        optim.momentum_step([Wa, ba], [a["dW2"], a["db2"]], acc_a, lr, mom)
        b = head.classification_tail(t(fc1), Wb, bb, t(labels), seed=3, step=step, accum_W2=acc_b[0], accum_b2=acc_b[1],
                                     lr=lr, momentum=mom)
        assert b["dW2"] is None and b["db2"] is None
        assert same_bits(a["dfc1"], b["dfc1"]) and same_bits(a["logits"], b["logits"]) and same_bits(a["loss_sum"], b["loss_sum"])
        for x, y in ((Wa, Wb), (ba, bb), (acc_a[0], acc_b[0]), (acc_a[1], acc_b[1])):
            assert same_bits(x, y)
    assert not np.array_equal(Wa.cpu().numpy(), W2) and not np.array_equal(ba.cpu().numpy(), b2)   # it did step


@pytest.mark.gpu
def test_fused_call_adds_no_launch_to_any_profile_kind(dev):
    import torch
    from pointwise_amd import _lib, head
    t = lambda a: torch.from_numpy(a).to(dev)
    lib = _lib.load()
    fc1, W2, b2, labels, _ = inputs(32, 512, 40, 19)
    args = (t(fc1), t(W2), t(b2), t(labels))
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        head.classification_tail(*args, seed=1, step=1)
        head.classification_tail(*args, training=False, need_grad=False)
        torch.cuda.synchronize(dev)
        for k in range(lib.conv3p_profile_kinds()):
            n, ms = ctypes.c_uint64(99), ctypes.c_double(0.0)
            assert lib.conv3p_profile_read(k, ctypes.byref(n), ctypes.byref(ms)) == _lib.OK
            assert n.value == 0, lib.conv3p_profile_name(k)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()


@pytest.mark.gpu
def test_nan_stays_in_its_row(dev):
    import torch
    from pointwise_amd import head
    t = lambda a: torch.from_numpy(a).to(dev)
    M, H, C = 32, 512, 40
    fc1, W2, b2, labels, mask = inputs(M, H, C, 23)
    mask[6, 100] = 1.0
    clean = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), keep_mask=t(mask))
    fc1[6, 100] = np.nan
    out = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), keep_mask=t(mask))
    assert np.isnan(float(out["loss_sum"]))
    dfc1 = out["dfc1"].cpu().numpy()
    assert np.isnan(dfc1[6]).all()
    others = [m for m in range(M) if m != 6]
    assert np.isfinite(dfc1[others]).all()
    assert same_bits(out["dfc1"][others], clean["dfc1"][others]) and same_bits(out["logits"][others], clean["logits"][others])
    assert np.array_equal(out["pred"].cpu().numpy()[others], clean["pred"].cpu().numpy()[others])


@pytest.mark.gpu
def test_ten_class_head_forward_backward_evaluate_and_summary(dev):
    """num_class = 10 (ModelNet10): refused by the fc kernels' N % 8 == 0 on the composed path, served by the tail."""
    import torch
    from oracle import head_numpy
    from pointwise_amd import head, optim
    t = lambda a: torch.from_numpy(a).to(dev)
    B, N, C = 5, 16, 10
    rng = np.random.default_rng(29)
    feat = rng.standard_normal((B, N, 36)).astype(np.float32)
    labels = rng.integers(0, C, size=B)
    mask = (rng.random((B, 512)) < 0.5).astype(np.float32)
    hd = head.ClassificationHead(N, num_class=C, device=dev, seed=31)
    par = [p.cpu().numpy() for p in hd.parameters()]
    loss, dfeat = hd.forward_backward(t(feat), t(labels), keep_mask=t(mask))
    r = head_numpy.head_forward_backward(feat, *par, labels, 0.5, mask.astype(np.float64))
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.device.type == "cuda"
    assert abs(float(loss) - r["loss"]) <= TOL * max(1.0, abs(r["loss"]))
    assert rel(hd.logits.cpu().numpy(), r["logits"]) <= TOL and rel(dfeat.cpu().numpy(), r["dfeat"]) <= TOL
    for g, k in zip(hd.gradients(), ("dW1", "db1", "dW2", "db2")):
        assert rel(g.cpu().numpy(), r[k]) <= TOL
    # global_batch scales the gradient, not the loss
    loss2, dfeat2 = hd.forward_backward(t(feat), t(labels), keep_mask=t(mask), global_batch=4 * B)
    assert same_bits(loss, loss2) and rel(4.0 * dfeat2.cpu().numpy(), r["dfeat"]) <= TOL
    # the default step is a per-head counter: two calls draw different masks, (seed, step) reproduces one
    l0, _ = hd.forward_backward(t(feat), t(labels))
    l1, _ = hd.forward_backward(t(feat), t(labels))
    l0b, _ = hd.forward_backward(t(feat), t(labels), step=2)                   # (two calls came before l0)
    assert same_bits(l0, l0b) and not same_bits(l0, l1)
    # evaluation and the epoch summary
    pred, cnt = hd.evaluate(t(feat), t(labels))
    fc1 = head_numpy.fully_connected(feat.reshape(B, -1), par[0], par[1])
    ev = cls_tail_ref(fc1, par[2], par[3], labels, 0.5, None)
    assert np.array_equal(cnt["all"].cpu().numpy(), counters(pred.cpu().numpy(), labels, C))
    assert rel(hd.logits.cpu().numpy(), ev["logits"]) <= TOL
    hd.accumulate()
    hd.accumulate()
    s = hd.summary()
    assert s["batches"] == 2 and s["points"] == 2 * B and abs(s["mean_loss"] - ev["loss_sum"] / B) <= TOL * max(1.0, ev["loss_sum"] / B)
    assert s["mean_accuracy"] == float((pred.cpu().numpy() == labels).mean())
    # an optimizer that owns everything: both layers are stepped inside the call, gradients() reports None
    opt = optim.MomentumOptimizer(hd.parameters(), 0.01, 0.9)
    before = [p.clone() for p in hd.parameters()]
    hd.forward_backward(t(feat), t(labels), optimizer=opt, keep_mask=t(mask))
    assert hd.gradients() == [None, None, None, None] and opt.global_step == 0
    opt.step(hd.gradients())
    assert opt.global_step == 1 and all(not torch.equal(p, q) for p, q in zip(hd.parameters(), before))
