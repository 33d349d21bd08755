"""float64 numpy restatement of the segmentation model's loss head and batch statistics (the CPU side of
test_seg_head.py / test_seg_model_step.py; pointwise_amd.seg_head is the device side).

    loss    pointcnn_scene_seg_acsd.py:60-71   softmax cross-entropy per point, mean over all B*N points
    counts  train_scene_seg_s3dis.py:134-145   argmax, correct points, per-class seen / correct -- the reference's
                                               double loop over B x N, vectorised with np.bincount

A label outside [0, C) is an ignored point: loss 0, gradient row 0 (tf.one_hot of such a label is a zero row), counted
under `invalid` only; the denominator stays `points` (default B*N)."""
import numpy as np


def seg_head_ref(act, labels, points=None):
    """act (..., C), labels (...) -> dict(loss, dact, pred, counts, row_loss), everything in float64 / int64.
    loss = sum of row losses / points, dact = (softmax - onehot) / points; counts = {correct, invalid, seen[C],
    correct_class[C], predicted[C]}."""
    C = act.shape[-1]
    x = np.asarray(act, dtype=np.float64).reshape(-1, C)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    R = x.shape[0]
    assert lab.shape[0] == R
    points = float(R if points is None else points)
    valid = (lab >= 0) & (lab < C)
    safe = np.where(valid, lab, 0)
    m = x.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - m[:, None])
        s = e.sum(axis=1)
        row_loss = np.where(valid, np.log(s) + m - x[np.arange(R), safe], 0.0)
        p = e / s[:, None]
    onehot = np.zeros_like(p)
    onehot[np.arange(R), safe] = 1.0
    dact = np.where(valid[:, None], (p - onehot) / points, 0.0)
    pred = np.argmax(x, axis=1).astype(np.int64)
    lv, pv = lab[valid], pred[valid]
    seen = np.bincount(lv, minlength=C)
    correct_class = np.bincount(lv[pv == lv], minlength=C)
    predicted = np.bincount(pv, minlength=C)
    counts = np.concatenate([[int((pv == lv).sum()), int((~valid).sum())], seen, correct_class, predicted]).astype(np.int64)
    return {"loss": float(row_loss.sum() / points), "dact": dact.reshape(act.shape), "pred": pred.reshape(act.shape[:-1]),
            "counts": counts, "row_loss": row_loss}


def selu(x):
    """The range layer 5 produces (selu.py:22-26)."""
    alpha, scale = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
    return scale * np.where(x >= 0, x, alpha * np.expm1(np.minimum(x, 0)))
