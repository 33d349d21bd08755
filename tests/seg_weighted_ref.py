"""float64 numpy restatement of the weighted segmentation loss head (the CPU side of test_seg_weighted.py and
test_seg_weighted_host.py; csrc/conv3p_seg_head_weighted.hpp is the device side).

    tf.losses.softmax_cross_entropy(onehot_labels, logits, weights, label_smoothing, reduction)
                                                                          (pointcnn_scene_seg_acsd.py:66-67)

Per point r with logits x, label l, class weights cw, point weights pw, smoothing ls, C classes:
    valid_r  = 0 <= l < C                          (any other label: an ignored point, weight 0, counted under `invalid`)
    w_r      = valid_r * cw[l] * pw[r]             (a missing table is all ones)
    q        = (1 - ls) * onehot(l) + ls / C       (TensorFlow's smoothed target)
    loss_r   = w_r * -sum_c q_c log softmax(x)_c
    dact_r   = w_r * (softmax(x) - q) / D
    loss     = sum_r loss_r / D
with the denominator D chosen by `reduction`:
    "points"           the number of points of the call (or the caller's `points`)
    "nonzero_weights"  #{r : w_r != 0}
    "sum_weights"      sum_r w_r
or given by the caller (`denominator`).  D == 0: loss 0, dact 0.  pred / counts are those of tests/seg_head_ref.py (they
do not look at the weights); the confusion matrix counts valid points at [label][pred]."""
import numpy as np

from tests.seg_head_ref import seg_head_ref

REDUCTIONS = ("points", "nonzero_weights", "sum_weights")


def row_weights(labels, C, class_weights=None, point_weights=None):
    """(R,) float64: valid * cw[label] * pw."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    valid = (lab >= 0) & (lab < C)
    w = valid.astype(np.float64)
    if class_weights is not None:
        w = w * np.asarray(class_weights, dtype=np.float64)[np.where(valid, lab, 0)]
    if point_weights is not None:
        w = w * np.asarray(point_weights, dtype=np.float64).reshape(-1)
    return np.where(valid, w, 0.0)


def weight_totals(labels, C, class_weights=None, point_weights=None):
    """{sum of the row weights, rows with a non-zero weight}."""
    w = row_weights(labels, C, class_weights, point_weights)
    return float(w.sum()), int(np.count_nonzero(w))


def confusion_ref(labels, pred, C):
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    keep = (lab >= 0) & (lab < C) & (p >= 0) & (p < C)
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (lab[keep], p[keep]), 1)
    return conf


def seg_weighted_ref(act, labels, class_weights=None, point_weights=None, label_smoothing=0.0, reduction="points",
                     points=None, denominator=None):
    """-> dict(loss, dact, pred, counts, confusion, loss_sum, weights, denominator, weight_sum, nonzero)."""
    assert reduction in REDUCTIONS
    C = act.shape[-1]
    x = np.asarray(act, dtype=np.float64).reshape(-1, C)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    R = x.shape[0]
    w = row_weights(lab, C, class_weights, point_weights)
    wsum, nonzero = float(w.sum()), int(np.count_nonzero(w))
    if denominator is not None:
        D = float(denominator)
    elif reduction == "points":
        D = float(R if points is None else points)
    else:
        D = wsum if reduction == "sum_weights" else float(nonzero)
    valid = (lab >= 0) & (lab < C)
    q = np.full((R, C), label_smoothing / C)
    q[np.arange(R)[valid], lab[valid]] += 1.0 - label_smoothing
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = x - x.max(axis=1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        ce = -(q * logp).sum(axis=1)
        use = w != 0                                        # a zero-weight row contributes nothing, whatever it holds
        row_loss = np.where(use, w * np.where(use, ce, 0.0), 0.0)
        g = np.where(use[:, None], w[:, None] * (np.exp(logp) - q), 0.0)
    loss_sum = float(row_loss.sum())
    if D == 0.0:
        loss, dact = 0.0, np.zeros_like(g)
    else:
        loss, dact = loss_sum / D, g / D
    plain = seg_head_ref(act, labels)
    return {"loss": loss, "dact": dact.reshape(act.shape), "pred": plain["pred"], "counts": plain["counts"],
            "confusion": confusion_ref(lab, plain["pred"], C), "loss_sum": loss_sum, "weights": w, "denominator": D,
            "weight_sum": wsum, "nonzero": nonzero}
