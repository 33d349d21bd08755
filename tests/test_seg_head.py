"""GPU tests of the fused segmentation loss head (conv3p_seg_head_f32 / _f64, pointwise_amd.seg_head) against the
float64 numpy restatement tests/seg_head_ref.py.

Tolerances (derived, eps = 2^-24):
  |loss - ref|                        fp32 <= 8 eps max(1, max|act| + ln C)   fp64 <= 1e-12 of the same scale
      (one rounding each for the max-subtract, exp, the C-term sum, log and the two adds on a row loss of that
       magnitude; rows are then averaged in double)
  global_points |dact - ref|          fp32 <= 32 eps ~ 1.9e-6                 fp64 <= 1e-12
      (a softmax entry is <= 1: a few ulps of exp plus the sum's)
Predictions and all 2 + 3 C counters are exact."""
import ctypes

import numpy as np
import pytest

from tests.seg_head_ref import seg_head_ref, selu

EPS = 2.0 ** -24
CLASSES = (2, 13, 41, 64, 128)
ROWS = (1, 63, 64, 65, 1000, 65536)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from pointwise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def loss_tol(act, C, fp64):
    scale = max(1.0, float(np.abs(act[np.isfinite(act)]).max()) + np.log(C))
    return (1e-12 if fp64 else 8 * EPS) * scale


DACT_TOL = {False: 32 * EPS, True: 1e-12}


def make(R, C, seed, fp64):
    rng = np.random.default_rng(seed)
    act = selu(2.0 * rng.standard_normal((R, C))).astype(np.float64 if fp64 else np.float32)
    labels = rng.integers(0, C, size=R).astype(np.int32)
    return act, labels


def raw_call(dev, act, labels, C, scale, grad=True, pred=True, ws_bytes=None, dact_fill=None):
    """One call of the C entry point on numpy inputs -> (status, dact, pred, loss_sum, counts) as numpy (None where the
    output was not asked for)."""
    import torch
    from pointwise_amd import _lib
    lib = _lib.load()
    fp64 = act.dtype == np.float64
    R = act.shape[0]
    a = torch.from_numpy(act).to(dev)
    l = torch.from_numpy(labels).to(dev)
    d = torch.empty_like(a) if grad else None
    if d is not None and dact_fill is not None:
        d.fill_(dact_fill)
    p = torch.full((R,), -7, dtype=torch.int32, device=dev) if pred else None
    ls = torch.full((), -1.0, dtype=torch.float64, device=dev)
    cn = torch.full((2 + 3 * C,), -1, dtype=torch.int64, device=dev)
    need = lib.conv3p_seg_head_workspace_bytes(R, C) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    fn = lib.conv3p_seg_head_f64 if fp64 else lib.conv3p_seg_head_f32
    real = ctypes.c_double if fp64 else ctypes.c_float
    with torch.cuda.device(dev):
        rc = fn(a.data_ptr(), l.data_ptr(), R, C, real(scale), d.data_ptr() if d is not None else None,
                p.data_ptr() if p is not None else None, ls.data_ptr(), cn.data_ptr(), ws.data_ptr(), need,
                torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return (rc, d.cpu().numpy() if d is not None else None, p.cpu().numpy() if p is not None else None,
            float(ls.cpu()), cn.cpu().numpy())


def check_against_ref(dev, act, labels, C, compare_loss=True):
    fp64 = act.dtype == np.float64
    R = act.shape[0]
    rc, d, p, ls, cn = raw_call(dev, act, labels, C, 1.0 / R)
    assert rc == 0
    ref = seg_head_ref(act, labels)
    assert np.array_equal(p, ref["pred"]), "pred"
    assert np.array_equal(cn, ref["counts"]), "counts"
    if compare_loss:
        dl, tl = abs(ls / R - ref["loss"]), loss_tol(act, C, fp64)
        dd = float(np.abs(d.astype(np.float64) - ref["dact"]).max() * R)
        print("R=%d C=%d fp64=%d  |dloss| %.3e (bound %.3e)  points*|ddact| %.3e (bound %.3e)" % (R, C, fp64, dl, tl, dd, DACT_TOL[fp64]))
        assert dl <= tl
        assert dd <= DACT_TOL[fp64]
    return d, p, ls, cn


@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("C", CLASSES)
def test_parity_over_the_grid(dev, C, fp64):
    from pointwise_amd import _lib
    for R in ROWS:
        act, labels = make(R, C, 100 * C + R % 97, fp64)
        if fp64 and C == 128:
            rc, d, p, ls, cn = raw_call(dev, act, labels, C, 1.0 / R, dact_fill=3.0)
            assert rc == _lib.ERR_UNSUPPORTED
            assert (d == 3.0).all() and (p == -7).all() and ls == -1.0 and (cn == -1).all()
            continue
        check_against_ref(dev, act, labels, C)


@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_large_activations_do_not_overflow(dev, fp64):
    """Row maximum 80, spread 160: exp(80) overflows fp32 unless the maximum is subtracted first."""
    rng = np.random.default_rng(9)
    R, C = 1000, 13
    act = rng.uniform(-80.0, 80.0, size=(R, C))
    act[np.arange(R), rng.integers(0, C, size=R)] = 80.0
    act = act.astype(np.float64 if fp64 else np.float32)
    labels = rng.integers(0, C, size=R).astype(np.int32)
    d, _, ls, _ = check_against_ref(dev, act, labels, C)
    assert np.isfinite(d).all() and np.isfinite(ls)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 13, 41])
def test_exact_integers_with_ties_and_infinite_maxima(dev, C):
    rng = np.random.default_rng(31 + C)
    R = 5000
    act = (np.round(selu(2.0 * rng.standard_normal((R, C))) * 4) / 4).astype(np.float32)   # multiples of 0.25
    labels = rng.integers(0, C, size=R).astype(np.int32)
    top = act.max(axis=1, keepdims=True)
    assert ((act == top).sum(axis=1) > 1).sum() > R // 50                   # many rows with a repeated maximum
    check_against_ref(dev, act, labels, C)
    inf_rows = rng.choice(R, size=200, replace=False)
    act[inf_rows, rng.integers(0, C, size=200)] = np.inf
    act[inf_rows[:50], rng.integers(0, C, size=50)] = np.inf                 # some rows with two +inf: first one wins
    check_against_ref(dev, act, labels, C, compare_loss=False)


@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_ignored_rows(dev, fp64):
    rng = np.random.default_rng(77)
    R, C = 4133, 13
    act, _ = make(R, C, 78, fp64)
    labels = rng.integers(-2, C + 2, size=R).astype(np.int32)               # uniform over [-2, C + 1]
    bad = (labels < 0) | (labels >= C)
    d, p, ls, cn = check_against_ref(dev, act, labels, C)
    assert cn[1] == bad.sum() > 0
    assert cn[2:2 + C].sum() == R - bad.sum()
    bits = d.view(np.uint64 if fp64 else np.uint32)
    assert (bits[bad] == 0).all()                                           # +0.0, bit for bit
    assert (np.abs(d[~bad]).max(axis=1) > 0).all()
    # int64 labels through the Python class: same numbers
    import torch
    from pointwise_amd.seg_head import SegmentationHead
    hd = SegmentationHead(C, device=dev)
    loss, dact, pred = hd.loss(torch.from_numpy(act.reshape(1, R, C)).to(dev),
                               torch.from_numpy(labels.astype(np.int64).reshape(1, R)).to(dev), need_pred=True)
    assert float(loss) == ls * (1.0 / R)
    assert np.array_equal(dact.cpu().numpy().reshape(R, C).view(bits.dtype), bits)
    assert np.array_equal(pred.cpu().numpy().reshape(R), p)
    assert np.array_equal(hd.counts()["all"].cpu().numpy(), cn) and int(hd.counts()["invalid"]) == bad.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("C", [13, 41])
def test_call_shapes(dev, C, fp64):
    R = 4096
    act, labels = make(R, C, 500 + C, fp64)
    rc, d, p, ls, cn = raw_call(dev, act, labels, C, 1.0 / R)
    assert rc == 0
    # evaluation call: no gradient, no prediction -> the same loss and counters
    rc2, d2, p2, ls2, cn2 = raw_call(dev, act, labels, C, 1.0 / R, grad=False, pred=False)
    assert rc2 == 0 and d2 is None and p2 is None
    ref = seg_head_ref(act, labels)
    assert np.array_equal(cn2, cn)
    assert abs(ls2 / R - ref["loss"]) <= loss_tol(act, C, fp64)
    assert ls2 == ls                                                        # (the row sums are formed in the same order)
    # twice the same call: the same bits
    rc3, d3, p3, ls3, cn3 = raw_call(dev, act, labels, C, 1.0 / R)
    u = np.uint64 if fp64 else np.uint32
    assert np.array_equal(d3.view(u), d.view(u)) and np.array_equal(p3, p) and np.array_equal(cn3, cn)
    assert np.float64(ls3).view(np.uint64) == np.float64(ls).view(np.uint64)
    # the first 1000 rows alone (same grad_scale): the same bits in dact and pred
    rc4, d4, p4, _, _ = raw_call(dev, act[:1000].copy(), labels[:1000].copy(), C, 1.0 / R)
    assert rc4 == 0
    assert np.array_equal(d4.view(u), d[:1000].view(u)) and np.array_equal(p4, p[:1000])


@pytest.mark.gpu
def test_errors_write_nothing(dev):
    from pointwise_amd import _lib
    act, labels = make(1000, 13, 3, False)
    for kw, want in ((dict(C=13, ws_bytes=256), _lib.ERR_WORKSPACE),         # (four records of 176 bytes are needed)
                     (dict(C=1), _lib.ERR_INVALID_ARGUMENT)):
        C = kw.pop("C")
        a = act if C == 13 else act[:, :1].copy()
        rc, d, p, ls, cn = raw_call(dev, a, labels, C, 0.001, dact_fill=3.0, **kw)
        assert rc == want
        assert (d == 3.0).all() and (p == -7).all() and ls == -1.0 and (cn == -1).all()


@pytest.mark.gpu
def test_python_class_accumulates_and_summarises(dev):
    import torch
    from pointwise_amd.seg_head import SegmentationHead, summarize
    B, N, C = 4, 1024, 13
    hd = SegmentationHead(C, device=dev)
    tot, losses = np.zeros(2 + 3 * C, np.int64), []
    for step in range(3):
        act, labels = make(B * N, C, 900 + step, False)
        ref = seg_head_ref(act, labels)
        a = torch.from_numpy(act.reshape(B, N, C)).to(dev)
        l = torch.from_numpy(labels.reshape(B, N)).to(dev)
        if step < 2:
            loss, dact = hd.loss(a, l)
            assert loss.dim() == 0 and loss.device.type == "cuda" and dact.shape == a.shape
            assert np.abs(dact.cpu().numpy().reshape(-1, C) - ref["dact"]).max() * B * N <= DACT_TOL[False]
        else:
            pred, cnt = hd.evaluate(a, l)
            assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy().reshape(-1), ref["pred"])
            assert np.array_equal(cnt["seen"].cpu().numpy(), ref["counts"][2:2 + C])
        assert abs(float(hd.last_loss()) - ref["loss"]) <= loss_tol(act, C, False)
        hd.accumulate()
        tot += ref["counts"]
        losses.append(ref["loss"])
    s = hd.summary()
    want = summarize(tot, sum(losses), 3, C)
    assert abs(s["mean_loss"] - want["mean_loss"]) <= loss_tol(act, C, False)
    for k in ("mean_accuracy", "avg_class_accuracy", "unseen_classes", "iou", "points", "invalid", "batches"):
        assert s[k] == want[k], k
    # global_points: the gradient of the sum over this rank's points / the global count
    loss1, dact1 = hd.loss(a, l, global_points=1)
    r1 = seg_head_ref(act, labels, points=1)
    assert np.abs(dact1.cpu().numpy().reshape(-1, C) - r1["dact"]).max() <= DACT_TOL[False]
    assert abs(float(loss1) - r1["loss"]) <= loss_tol(act, C, False) * B * N


@pytest.mark.gpu
def test_profile_kind_and_code_object(dev):
    import torch
    from pointwise_amd import _lib, build
    lib = _lib.load()
    res = [r for r in build.kernel_resources() if "seg_head" in r[0]]
    assert any("seg_head_kernelIf" in r[0] for r in res) and any("seg_head_kernelId" in r[0] for r in res)
    assert any("seg_head_finish_kernel" in r[0] for r in res)
    for name, _, vgpr_spills, _, private in res:
        assert vgpr_spills == 0 and private == 0, name
    act, labels = make(1000, 13, 4, False)
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    try:
        raw_call(dev, act, labels, 13, 0.001)
        got = {}
        for k in range(lib.conv3p_profile_kinds()):
            n, ms = ctypes.c_uint64(0), ctypes.c_double(0)
            assert lib.conv3p_profile_read(k, ctypes.byref(n), ctypes.byref(ms)) == 0
            if n.value:
                got[lib.conv3p_profile_name(k).decode()] = (n.value, ms.value)
    finally:
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
    assert list(got) == ["seg_head_kernel"] and got["seg_head_kernel"][0] == 1 and got["seg_head_kernel"][1] > 0.0
