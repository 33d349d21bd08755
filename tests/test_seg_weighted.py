"""GPU tests of the weighted segmentation loss head (conv3p_seg_weight_total_*, conv3p_seg_head_weighted_*,
conv3p_seg_confusion; SegmentationHead's class_weights / point_weights / label_smoothing / reduction / confusion)
against the float64 numpy restatement tests/seg_weighted_ref.py, and bit for bit against the plain head.

Tolerances.  tests/test_seg_head.py derives, for the unweighted mean over the call's points (eps = 2^-24):
  |loss - ref|           fp32 <= 8 eps max(1, max|act| + ln C), fp64 <= 1e-12 of the same scale: one rounding each for
                         the max-subtract, exp, the C-term sum, log and the adds of a row loss of that magnitude; the
                         rows are then added in double
  points |dact - ref|    fp32 <= 32 eps, fp64 <= 1e-12: a softmax entry is <= 1, a few ulps of exp plus the sum's
Here a row's loss and gradient carry the factor w_r / D instead of 1 / points, so both bounds are multiplied by
max_r w_r * points / D (D: the denominator of the reduction).  The additional roundings stay inside the same budget:
w_r = class_weight * point_weight and w_r * scale are one rounding each and scale = 1 / D is rounded once (three more
half-ulps on a gradient entry that has 32 eps); under smoothing the row loss is evaluated as
log s + (1 - ls)(m - x_label) + (ls / C) sum_c (m - x_c) -- every term >= 0, nothing cancels -- which adds one C-term sum
scaled by ls / C <= 1 / C, the same kind of term the bound already carries for s.  No bound is wider than derived.
Predictions, the 2 + 3 C counters, the weight totals' non-zero count and the confusion matrix are exact; the sum of
the weights is a double sum of at most 70 000 T-rounded products (<= 1e-12 relative in fp64, 2 eps in fp32: the
products' own rounding)."""
import ctypes

import numpy as np
import pytest

from tests.seg_head_ref import selu
from tests.seg_weighted_ref import confusion_ref, seg_weighted_ref, weight_totals
from tests.test_seg_head import DACT_TOL, EPS, loss_tol, make, raw_call

ROWS = (1, 63, 64, 65, 1000)
GRID = [(False, C) for C in (2, 13, 41, 128)] + [(True, C) for C in (2, 13, 41, 79)]
GRID_IDS = ["%s-C%d" % ("fp64" if f else "fp32", C) for f, C in GRID]
BIG = (70000, 128)        # fp32: one wave per workgroup, the 1024-workgroup grid wraps; past the confusion grid's cap
DATA_DEPENDENT = ("nonzero_weights", "sum_weights")


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from pointwise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def make_weighted(R, C, seed, fp64):
    """act, labels over [-2, C + 1] (out of range on both sides), class and point weights with exact zeros; the weights
    are representable in the element type, so the float64 restatement sees the same numbers."""
    rng = np.random.default_rng(seed)
    dt = np.float64 if fp64 else np.float32
    act = selu(2.0 * rng.standard_normal((R, C))).astype(dt)
    labels = rng.integers(0, C, size=R).astype(np.int32)
    bad = rng.random(R) < 0.1
    labels[bad] = rng.choice(np.array([-2, -1, C, C + 1], np.int32), size=int(bad.sum()))
    cw = rng.uniform(0.25, 4.0, size=C).astype(dt)
    cw[rng.integers(0, C)] = 0.0
    pw = rng.uniform(0.0, 2.0, size=R).astype(dt)
    pw[rng.random(R) < 0.15] = 0.0
    return act, labels, cw, pw


def raw_weighted(dev, act, labels, C, cw=None, pw=None, ls=0.0, scale=1.0, den=None, grad=True):
    """One call of conv3p_seg_head_weighted_* on numpy inputs -> (status, dact, pred, loss_sum, counts)."""
    import torch
    from pointwise_amd import _lib
    lib = _lib.load()
    fp64 = act.dtype == np.float64
    R = act.shape[0]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda a: None if a is None else a.data_ptr()
    a, l, w1, w2 = t(act), t(labels), t(cw), t(pw)
    dn = None if den is None else torch.tensor([den], dtype=torch.float64, device=dev)
    d = torch.empty_like(a) if grad else None
    p = torch.full((R,), -7, dtype=torch.int32, device=dev)
    lsum = torch.full((), -1.0, dtype=torch.float64, device=dev)
    cn = torch.full((2 + 3 * C,), -1, dtype=torch.int64, device=dev)
    need = lib.conv3p_seg_head_weighted_workspace_bytes(R, C)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    fn = lib.conv3p_seg_head_weighted_f64 if fp64 else lib.conv3p_seg_head_weighted_f32
    real = ctypes.c_double if fp64 else ctypes.c_float
    with torch.cuda.device(dev):
        rc = fn(a.data_ptr(), l.data_ptr(), R, C, ptr(w1), ptr(w2), ls, real(scale), ptr(dn), ptr(d), p.data_ptr(),
                lsum.data_ptr(), cn.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, d.cpu().numpy() if d is not None else None, p.cpu().numpy(), float(lsum.cpu()), cn.cpu().numpy()


def head_call(dev, C, act, labels, cw=None, pw=None, ls=0.0, reduction="points", **kw):
    """SegmentationHead.loss on numpy inputs (one batch of R points) -> (head, loss, dact (R, C), pred (R,))."""
    import torch
    from pointwise_amd.seg_head import SegmentationHead
    R = act.shape[0]
    hd = SegmentationHead(C, device=dev, class_weights=cw, label_smoothing=ls, reduction=reduction)
    pwt = None if pw is None else torch.from_numpy(pw.reshape(1, R)).to(dev)
    loss, dact, pred = hd.loss(torch.from_numpy(act.reshape(1, R, C)).to(dev), torch.from_numpy(labels.reshape(1, R)).to(dev),
                               need_pred=True, point_weights=pwt, **kw)
    return hd, float(loss), dact.cpu().numpy().reshape(R, C), pred.cpu().numpy().reshape(R)


def check_against_ref(dev, C, act, labels, cw, pw, ls, reduction, what=""):
    fp64 = act.dtype == np.float64
    R = act.shape[0]
    hd, loss, dact, pred = head_call(dev, C, act, labels, cw, pw, ls, reduction)
    ref = seg_weighted_ref(act, labels, cw, pw, ls, reduction)
    assert np.array_equal(pred, ref["pred"]), "pred"
    assert np.array_equal(hd.counts()["all"].cpu().numpy(), ref["counts"]), "counts"
    D = ref["denominator"]
    if D == 0:
        assert loss == 0.0 and not bits(dact).any(), "zero denominator"
        return
    factor = float(ref["weights"].max()) * R / D
    dl, tl = abs(loss - ref["loss"]), loss_tol(act, C, fp64) * factor
    dd, td = float(np.abs(dact.astype(np.float64) - ref["dact"]).max() * R), DACT_TOL[fp64] * factor
    print("%s R=%d C=%d fp64=%d ls=%g %s  |dloss| %.3e (bound %.3e)  points*|ddact| %.3e (bound %.3e)"
          % (what, R, C, fp64, ls, reduction, dl, tl, dd, td))
    assert dl <= tl, "loss"
    assert dd <= td, "dact"
    zero_w = ref["weights"] == 0
    assert not bits(dact)[zero_w].any()                                      # +0.0, bit for bit


# ---------------------------------------------------------------------------------------------- 1. the plain head
def check_bit_equal(dev, R, C, fp64):
    act, labels = make(R, C, 7 * C + R % 89, fp64)
    labels[::17] = C                                                        # some ignored rows
    rc0, d0, p0, ls0, cn0 = raw_call(dev, act, labels, C, 1.0 / R)
    rc1, d1, p1, ls1, cn1 = raw_weighted(dev, act, labels, C, scale=1.0 / R)
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(bits(d1), bits(d0)) and np.array_equal(p1, p0) and np.array_equal(cn1, cn0)
    assert np.float64(ls1).view(np.uint64) == np.float64(ls0).view(np.uint64)
    hd, loss, dact, pred = head_call(dev, C, act, labels)                   # all defaults: reduction "points"
    assert np.array_equal(bits(dact), bits(d0)) and np.array_equal(pred, p0)
    assert np.array_equal(hd.counts()["all"].cpu().numpy(), cn0) and loss == ls0 * (1.0 / R)


@pytest.mark.gpu
@pytest.mark.parametrize("fp64,C", GRID, ids=GRID_IDS)
def test_defaults_are_bit_equal_to_the_plain_head(dev, fp64, C):
    for R in ROWS:
        check_bit_equal(dev, R, C, fp64)


@pytest.mark.gpu
def test_defaults_are_bit_equal_to_the_plain_head_when_the_grid_wraps(dev):
    check_bit_equal(dev, BIG[0], BIG[1], False)


# ---------------------------------------------------------------------------------------------- 2. the restatement
MODES = (("class", True, False, 0.0), ("point", False, True, 0.0), ("both", True, True, 0.0),
         ("smooth.1", False, False, 0.1), ("both+smooth.5", True, True, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("fp64,C", GRID, ids=GRID_IDS)
def test_weights_smoothing_and_reductions_against_the_restatement(dev, fp64, C):
    for R in ROWS:
        act, labels, cw, pw = make_weighted(R, C, 1000 * C + R, fp64)
        for what, use_cw, use_pw, ls in MODES:
            for reduction in ("points",) + DATA_DEPENDENT:
                check_against_ref(dev, C, act, labels, cw if use_cw else None, pw if use_pw else None, ls, reduction, what)


@pytest.mark.gpu
def test_against_the_restatement_when_the_grid_wraps(dev):
    R, C = BIG
    act, labels, cw, pw = make_weighted(R, C, 4242, False)
    check_against_ref(dev, C, act, labels, cw, pw, 0.1, "sum_weights", "big")
    # the kernel without smoothing and the other two reductions, where a workgroup takes a second tile
    check_against_ref(dev, C, act, labels, None, pw, 0.0, "nonzero_weights", "big")
    check_against_ref(dev, C, act, labels, cw, None, 0.0, "points", "big")


@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_weight_total(dev, fp64):
    """The pre-pass alone, through weight_total(): the non-zero count exactly, the sum to the products' rounding."""
    import torch
    from pointwise_amd.seg_head import SegmentationHead
    for R in ROWS + (BIG[0],):                                              # 70 000 rows: 69 workgroups
        C = 13
        _, labels, cw, pw = make_weighted(R, C, 55 + R, fp64)
        want_sum, want_nz = weight_totals(labels, C, cw, pw)
        l = torch.from_numpy(labels.reshape(1, R)).to(dev)
        p = torch.from_numpy(pw.reshape(1, R)).to(dev)
        got = []
        for reduction in DATA_DEPENDENT:
            hd = SegmentationHead(C, device=dev, class_weights=cw, reduction=reduction)
            a, b = hd.weight_total(l, p), hd.weight_total(l.long(), p)
            assert a.dim() == 0 and a.dtype == torch.float64 and a.device.type == "cuda"
            assert np.float64(float(a)).view(np.uint64) == np.float64(float(b)).view(np.uint64)   # same inputs, same bits
            got.append(float(a))
        assert got[0] == want_nz
        assert abs(got[1] - want_sum) <= (1e-12 if fp64 else 2 * EPS) * max(want_sum, 1.0)
        # class weights alone (dtype= names the element type), and no weights at all: the valid rows
        valid = int(((labels >= 0) & (labels < C)).sum())
        hd = SegmentationHead(C, device=dev, reduction="sum_weights")
        assert float(hd.weight_total(l, dtype=torch.float64 if fp64 else torch.float32)) == valid


# ---------------------------------------------------------------------------------------------- 3. zero denominators
@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_zero_denominator_gives_zero_loss_and_positive_zero_gradient(dev, fp64):
    R, C = 1000, 13
    act, labels, cw, pw = make_weighted(R, C, 31, fp64)
    for reduction in DATA_DEPENDENT:
        for what, lab, c, p in (("all rows ignored", np.full(R, C, np.int32), cw, pw),
                                ("all point weights zero", labels, cw, np.zeros_like(pw)),
                                ("all class weights zero", labels, np.zeros_like(cw), None)):
            hd, loss, dact, pred = head_call(dev, C, act, lab, c, p, 0.1, reduction)
            assert loss == 0.0 and np.float64(loss).view(np.uint64) == 0, what
            assert not bits(dact).any(), what                               # +0.0 everywhere, bit for bit
            ref = seg_weighted_ref(act, lab, c, p, 0.1, reduction)
            assert ref["denominator"] == 0
            assert np.array_equal(hd.counts()["all"].cpu().numpy(), ref["counts"]) and np.array_equal(pred, ref["pred"])
    # a zero denominator handed in from outside, with weights that are not zero: still loss 0 and gradient +0
    import torch
    hd, loss, dact, _ = head_call(dev, C, act, labels, cw, pw, 0.1, "sum_weights",
                                  denominator=torch.zeros((), dtype=torch.float64, device=dev))
    assert loss == 0.0 and not bits(dact).any()


# ---------------------------------------------------------------------------------------------- 4. the data-parallel contract
@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("reduction", DATA_DEPENDENT)
def test_external_denominator(dev, reduction, fp64):
    import torch
    from pointwise_amd.seg_head import SegmentationHead
    R, C = 1000, 13
    act, labels, cw, pw = make_weighted(R, C, 77, fp64)
    _, loss1, d1, _ = head_call(dev, C, act, labels, cw, pw, 0.1, reduction)
    hd = SegmentationHead(C, device=dev, class_weights=cw, reduction=reduction)
    total = hd.weight_total(torch.from_numpy(labels.reshape(1, R)).to(dev), torch.from_numpy(pw.reshape(1, R)).to(dev))
    ref1 = seg_weighted_ref(act, labels, cw, pw, 0.1, reduction)
    assert abs(float(total) - ref1["denominator"]) <= 1e-6 * ref1["denominator"]
    twice = total * 2                                                       # "two ranks with the same batch": all-reduced
    _, loss2, d2, _ = head_call(dev, C, act, labels, cw, pw, 0.1, reduction, denominator=twice)
    u = 2.0 ** -53 if fp64 else EPS
    assert (np.abs(2.0 * d2.astype(np.float64) - d1) <= u * np.abs(d1)).all()   # halved, within one rounding
    assert np.abs(d1).max() > 0
    ref2 = seg_weighted_ref(act, labels, cw, pw, 0.1, reduction, denominator=2.0 * float(total))
    factor = float(ref2["weights"].max()) * R / ref2["denominator"]
    assert abs(loss2 - ref2["loss"]) <= loss_tol(act, C, fp64) * factor
    assert np.abs(d2 - ref2["dact"]).max() * R <= DACT_TOL[fp64] * factor
    assert abs(2.0 * loss2 - loss1) <= 2.0 ** -52 * loss1


# ---------------------------------------------------------------------------------------------- 5. reproducibility
@pytest.mark.gpu
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("C", [13, 41])
def test_reproducible_and_rows_independent(dev, C, fp64):
    import torch
    R, R1 = 1064, 1000
    act, labels, cw, pw = make_weighted(R, C, 300 + C, fp64)
    for reduction in ("points",) + DATA_DEPENDENT:
        kw = dict(global_points=R) if reduction == "points" else \
            dict(denominator=torch.tensor(123.5, dtype=torch.float64, device=dev))
        hd_a, loss_a, d_a, p_a = head_call(dev, C, act, labels, cw, pw, 0.1, reduction, **kw)
        hd_b, loss_b, d_b, p_b = head_call(dev, C, act, labels, cw, pw, 0.1, reduction, **kw)
        assert np.array_equal(bits(d_a), bits(d_b)) and np.array_equal(p_a, p_b)
        assert np.float64(loss_a).view(np.uint64) == np.float64(loss_b).view(np.uint64)
        assert np.array_equal(hd_a.counts()["all"].cpu().numpy(), hd_b.counts()["all"].cpu().numpy())
        _, _, d_c, p_c = head_call(dev, C, act[:R1].copy(), labels[:R1].copy(), cw, pw[:R1].copy(), 0.1, reduction, **kw)
        assert np.array_equal(bits(d_c), bits(d_a[:R1])) and np.array_equal(p_c, p_a[:R1])
        if reduction != "points":                                           # ... and with the head's own pre-pass, twice
            _, loss_d, d_d, _ = head_call(dev, C, act, labels, cw, pw, 0.1, reduction)
            _, loss_e, d_e, _ = head_call(dev, C, act, labels, cw, pw, 0.1, reduction)
            assert np.array_equal(bits(d_d), bits(d_e)) and np.float64(loss_d).view(np.uint64) == np.float64(loss_e).view(np.uint64)


# ---------------------------------------------------------------------------------------------- 6. the confusion matrix
@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 13, 128])
def test_confusion_kernel_on_arbitrary_rows(dev, C):
    """conv3p_seg_confusion alone: any labels / predictions (out-of-range ones are not counted), up to rows past the
    grid cap (64 workgroups of 1024 rows)."""
    import torch
    from pointwise_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(C)
    for R in ROWS + (BIG[0],):
        labels = rng.integers(-1, C + 1, size=R).astype(np.int32)
        pred = rng.integers(-1, C + 1, size=R).astype(np.int32)
        l, p = torch.from_numpy(labels).to(dev), torch.from_numpy(pred).to(dev)
        conf = torch.full((C, C), -1, dtype=torch.int64, device=dev)
        need = lib.conv3p_seg_confusion_workspace_bytes(R, C)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.conv3p_seg_confusion(l.data_ptr(), p.data_ptr(), R, C, conf.data_ptr(), ws.data_ptr(), need,
                                          torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        assert np.array_equal(conf.cpu().numpy(), confusion_ref(labels, pred, C)), R


@pytest.mark.gpu
def test_confusion_through_evaluate_accumulate_and_summary(dev):
    import torch
    from pointwise_amd.seg_head import SegmentationHead
    B, N, C = 2, 500, 13
    hd = SegmentationHead(C, device=dev)
    total = np.zeros((C, C), np.int64)
    for step in range(3):
        act, labels, _, _ = make_weighted(B * N, C, 600 + step, False)
        a = torch.from_numpy(act.reshape(B, N, C)).to(dev)
        l = torch.from_numpy(labels.reshape(B, N)).to(dev)
        pred, cnt = hd.evaluate(a, l, confusion=True)
        ref = seg_weighted_ref(act, labels)
        conf = cnt["confusion"]
        assert conf.dtype == torch.int64 and tuple(conf.shape) == (C, C) and conf.device.type == "cuda"
        conf = conf.cpu().numpy()
        assert np.array_equal(conf, ref["confusion"]) and np.array_equal(pred.cpu().numpy().reshape(-1), ref["pred"])
        assert np.array_equal(conf.sum(axis=1), cnt["seen"].cpu().numpy())
        assert np.array_equal(np.diag(conf), cnt["correct_class"].cpu().numpy())
        assert np.array_equal(conf.sum(axis=0), cnt["predicted"].cpu().numpy())
        valid = int(((labels >= 0) & (labels < C)).sum())
        assert conf.sum() == valid < B * N and int(cnt["invalid"]) == B * N - valid
        hd.accumulate()
        total += ref["confusion"]
    s = hd.summary()
    assert np.array_equal(np.array(s["confusion"]), total) and s["batches"] == 3 and s["points"] == total.sum()
    # a call without confusion=True has none, and neither has a summary of such calls
    _, cnt = hd.evaluate(a, l)
    assert "confusion" not in cnt
    hd.accumulate()
    assert "confusion" not in hd.summary()


# ---------------------------------------------------------------------------------------------- 7. a model step
@pytest.mark.gpu
def test_segmentation_model_step_with_a_weighted_smoothed_loss(dev):
    """tests/test_seg_model_step.py's graph (stack -> head -> stack backward against oracle conv3p + numpy SELU + the
    restatement) with class weights, ls = 0.1 and reduction "sum_weights", at B = 2, N = 1024, within that file's
    tolerances.  Its rel() is a true relative error, so the small scale of a mean's gradients loosens nothing.  Loss
    bound: the head's own (times max w * points / D, as above) plus the activation tolerance per point times the same
    factor -- the activations feeding the loss already differ by up to that much."""
    import torch
    from oracle import oracle
    from pointwise_amd import stack, synth
    from pointwise_amd.seg_head import SegmentationHead
    from tests.test_seg_model_step import TOL, VOX, rel
    dt = np.float32
    B, N, CIN, NCLS = 2, 1024, 9, 13
    R = B * N
    tol_a, tol_g, head_factor = TOL[dt]
    P = synth.room_like(B, N, seed=2700).astype(dt)
    X = synth.features(B, N, CIN, 2701, points=P, dtype=dt)
    rng = np.random.default_rng(2702)
    labels = rng.integers(-1, NCLS, size=(B, N))                            # -1: ignored points
    cw = rng.uniform(0.5, 2.0, size=NCLS).astype(dt)
    cw[3] = 0.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    st = stack.Conv3pStack(CIN, NCLS, device=dev, dtype=torch.float32, seed=2703)
    acts = st.forward(t(P), t(X))
    hd = SegmentationHead(NCLS, device=dev, class_weights=cw, label_smoothing=0.1, reduction="sum_weights")
    loss, dact = hd.loss(acts[4], t(labels))
    dx, fused = st.backward([dact])

    filters = [f.cpu().numpy() for f in st.filters]
    x, ref_acts = X, []
    for li in range(4):
        s = st.layers[li][2]
        x = stack.selu_numpy(oracle.forward(P, x, filters[li], (s, s, s), VOX))
        ref_acts.append(x)
    concat = np.concatenate(ref_acts, axis=2)
    head = stack.selu_numpy(oracle.forward(P, concat, filters[4], (1, 1, 1), VOX))
    r = seg_weighted_ref(head, labels, class_weights=cw, label_smoothing=0.1, reduction="sum_weights")
    g = stack.selu_grad_numpy(head, np.ascontiguousarray(r["dact"].astype(dt)))
    dconcat, dw4 = oracle.backward(g, P, concat, filters[4], (1, 1, 1), VOX)
    carry, dws = None, [None] * 4 + [dw4]
    for li in (3, 2, 1, 0):
        s = st.layers[li][2]
        up = dconcat[:, :, 9 * li:9 * li + 9]
        gi = stack.selu_grad_numpy(ref_acts[li], np.ascontiguousarray(up if carry is None else up + carry))
        carry, dws[li] = oracle.backward(gi, P, ref_acts[li - 1] if li > 0 else X, filters[li], (s, s, s), VOX)
    ref_fused = np.concatenate([d.reshape(-1) for d in dws])

    for li, (a, ra) in enumerate(zip(acts, ref_acts + [head])):
        e = rel(a.cpu().numpy(), ra) * min(1.0, float(np.abs(ra).max()))
        assert e <= tol_a, ("activation", li, e)
    factor = float(r["weights"].max()) * R / r["denominator"]
    loss_bound = (head_factor * max(1.0, float(np.abs(head).max()) + np.log(NCLS)) + tol_a) * factor
    print("loss", float(loss), r["loss"], abs(float(loss) - r["loss"]), loss_bound)
    assert abs(float(loss) - r["loss"]) <= loss_bound
    e_d, e_x, e_w = rel(dact.cpu().numpy(), r["dact"]), rel(dx.cpu().numpy(), carry), rel(fused.cpu().numpy(), ref_fused)
    print("dact %.3e dx %.3e dW %.3e" % (e_d, e_x, e_w))
    assert e_d <= tol_g and e_x <= tol_g and e_w <= tol_g
    cnt = hd.counts()
    assert int(cnt["invalid"]) == int((labels < 0).sum()) > 0 and int(cnt["seen"].sum()) == R - int((labels < 0).sum())
