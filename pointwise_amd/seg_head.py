"""The per-point loss head of the reference's segmentation model, on one fused HIP pass.

/root/reference/scene_seg/pointcnn_scene_seg_acsd.py:57-71
    fc2  = selu(conv3p(concat, 36 -> num_class))            (B, N, num_class)  -- stack.Conv3pStack(c, num_class)
    loss = mean over all B*N points of sparse softmax cross-entropy(fc2, labels)
/root/reference/scene_seg/train_scene_seg_s3dis.py:134-145 (eval_scene_seg_s3dis.py:88-98), after every batch:
    pred = argmax(fc2, 2); correct points; per class: points seen, points correct -- a Python double loop over B x N.

conv3p_seg_head_f32 / _f64 (include/conv3p.h, csrc/conv3p_seg_head.hpp) compute the loss, its gradient with respect to
the activation, the predictions and the counters in one read and one write of the (B*N, num_class) tensor, stream
ordered, bitwise reproducible.  Nothing here synchronises except summary().

A label outside [0, num_class) marks an ignored point: no loss, zero gradient, counted under `invalid` only; the
mean still divides by B*N (what the reference's one-hot of such a label gives).

The loss call of the reference, tf.losses.softmax_cross_entropy (pointcnn_scene_seg_acsd.py:66-67), also takes
`weights`, `label_smoothing` and a `reduction`; SegmentationHead takes them as class_weights / point_weights,
label_smoothing and reduction (conv3p_seg_head_weighted_*, csrc/conv3p_seg_head_weighted.hpp), and evaluate() can
return the confusion matrix (conv3p_seg_confusion).  With the defaults every call is the plain head above, bit for bit.
"""
import torch

from . import _lib
from ._host import _HEADS, _SFX, Conv3pInvalidArgument, Conv3pRuntimeError, _call, _check_device, _require, _workspace

REDUCTIONS = ("points", "nonzero_weights", "sum_weights")


def split_counts(counts, num_class):
    """Views of a {correct, invalid, seen[C], correct_class[C], predicted[C]} vector (tensor or array)."""
    C = num_class
    return {"correct": counts[0], "invalid": counts[1], "seen": counts[2:2 + C], "correct_class": counts[2 + C:2 + 2 * C],
            "predicted": counts[2 + 2 * C:2 + 3 * C]}


def summarize(counts, loss_total, batches, num_class, confusion=None):
    """The epoch numbers from accumulated counters (an int64 CPU tensor / sequence of 2 + 3 C entries), the sum of the
    batches' mean losses and the number of batches.  Pure host arithmetic.

    mean_loss, mean_accuracy, avg_class_accuracy as printed by train_scene_seg_s3dis.py:157-159: loss_sum / batches,
    correct / seen points, mean over classes of correct_class / seen.  The reference divides 0 / 0 for a class that never
    occurred; here such classes are left out of the mean and listed under `unseen_classes`.  Ignored points
    (`invalid`) are in no ratio.  iou[c] = correct_class / (seen + predicted - correct_class), None where that is 0 / 0;
    mean_iou is over the classes that have one.

    confusion (optional, C x C counts, [label][pred]): returned under "confusion" as a list of integer rows."""
    c = [int(v) for v in counts]
    if len(c) != 2 + 3 * num_class:
        raise Conv3pInvalidArgument("SegmentationHead: counts must have 2 + 3 * num_class entries")
    v = split_counts(c, num_class)
    seen_total = sum(v["seen"])
    acc = [v["correct_class"][k] / v["seen"][k] for k in range(num_class) if v["seen"][k] > 0]
    iou = []
    for k in range(num_class):
        union = v["seen"][k] + v["predicted"][k] - v["correct_class"][k]
        iou.append(v["correct_class"][k] / union if union > 0 else None)
    have = [x for x in iou if x is not None]
    out = {"mean_loss": float(loss_total) / batches if batches else float("nan"),
           "mean_accuracy": v["correct"] / seen_total if seen_total else float("nan"),
           "avg_class_accuracy": sum(acc) / len(acc) if acc else float("nan"),
           "unseen_classes": [k for k in range(num_class) if v["seen"][k] == 0],
           "iou": iou, "mean_iou": sum(have) / len(have) if have else float("nan"),
           "points": seen_total, "invalid": v["invalid"], "batches": int(batches)}
    if confusion is not None:
        rows = [[int(x) for x in row] for row in confusion]
        if len(rows) != num_class or any(len(r) != num_class for r in rows):
            raise Conv3pInvalidArgument("SegmentationHead: confusion must be num_class x num_class")
        out["confusion"] = rows
    return out


def class_weights_from_counts(seen, kind="inverse"):
    """Per-class loss weights from per-class point counts (e.g. summary()'s / counts()'s `seen` over a training set)
    -> float64 CPU tensor, what SegmentationHead(class_weights=...) takes.  Pure host arithmetic.

    "inverse"           w_c = total / (K * seen_c), K = classes that occur: inverse frequency, scaled so that
                        sum_c w_c * seen_c = total (the weighted and the unweighted point counts agree)
    "median_frequency"  w_c = median(f) / f_c with f_c = seen_c / total, the median over the classes that occur
    A class that never occurs gets weight 0 under both."""
    n = [int(v) for v in seen]
    _require(len(n) >= 2 and all(v >= 0 for v in n), "class_weights_from_counts: at least two non-negative counts expected")
    _require(kind in ("inverse", "median_frequency"), "class_weights_from_counts: kind must be 'inverse' or 'median_frequency'")
    total = sum(n)
    present = sorted(v for v in n if v > 0)
    _require(total > 0, "class_weights_from_counts: all counts are zero")
    if kind == "inverse":
        w = [total / (len(present) * v) if v > 0 else 0.0 for v in n]
    else:
        h = len(present) // 2
        median = present[h] if len(present) % 2 else (present[h - 1] + present[h]) / 2      # of the counts: total cancels
        w = [median / v if v > 0 else 0.0 for v in n]
    return torch.tensor(w, dtype=torch.float64)


class SegmentationHead:
    """Loss, gradient and batch statistics of the segmentation model's (B, N, num_class) activation.

    class_weights (num_class floats: a sequence, an array or a tensor), label_smoothing in [0, 1) and reduction are
    those of tf.losses.softmax_cross_entropy (pointcnn_scene_seg_acsd.py:66-67); per-point weights are an argument of
    loss() / evaluate().  A point's weight is class_weights[label] * point_weights[point]; the target under smoothing
    is TensorFlow's, (1 - ls) onehot + ls / num_class.  reduction: what the sum of the weighted point losses is divided by
        "points"            global_points, default B*N (the plain head's rule)
        "nonzero_weights"   the number of points with a non-zero weight (TensorFlow's default, SUM_BY_NONZERO_WEIGHTS)
        "sum_weights"       the sum of the weights (torch's CrossEntropyLoss(weight=..., ignore_index=...) mean)
    The last two are known only on the device: a pre-pass over the labels and weights leaves them there and the main
    pass reads them there (no synchronisation); a zero denominator gives loss 0 and a zero gradient.  Weights are not
    validated: negative or non-finite ones propagate.
    The constructor keeps class_weights as a float64 host copy (the device copies are made per element type at first
    use): given as a device tensor, that copy synchronises once, at construction -- no call afterwards does."""

    def __init__(self, num_class, device="cuda:0", class_weights=None, label_smoothing=0.0, reduction="points"):
        _require(isinstance(num_class, int) and num_class >= 2, "SegmentationHead: num_class must be an integer >= 2")
        self.num_class = num_class
        self.device = torch.device(device)
        _require(reduction in REDUCTIONS, "SegmentationHead: reduction must be one of %s" % ", ".join(REDUCTIONS))
        self.reduction = reduction
        _require(isinstance(label_smoothing, (int, float)) and 0.0 <= float(label_smoothing) < 1.0,
                 "SegmentationHead: label_smoothing must be in [0, 1)")
        self.label_smoothing = float(label_smoothing)
        self.class_weights = None     # float64 CPU tensor (num_class)
        self._cw = {}                 # dtype -> the device copy the kernels read
        if class_weights is not None:
            try:
                cw = torch.as_tensor(class_weights)
            except (TypeError, ValueError, RuntimeError):
                raise Conv3pInvalidArgument("SegmentationHead: class_weights must be num_class numbers")
            _require(cw.dtype in (torch.float32, torch.float64), "SegmentationHead: class_weights must be float32 or float64")
            _require(tuple(cw.shape) == (num_class,), "SegmentationHead: class_weights must have num_class entries")
            _require(cw.device.type == "cpu" or cw.device == self.device,
                     "SegmentationHead: class_weights must be on the host or on the head's device")
            self.class_weights = cw.detach().to("cpu", torch.float64).clone()
        self._counts = None           # int64[2 + 3 C] of the last call
        self._loss = None             # 0-d double: the last call's mean loss
        self._confusion = None        # int64 (C, C) of the last call, if it was evaluate(confusion=True)
        self._tot_counts = None
        self._tot_loss = None
        self._tot_confusion = None
        self._batches = 0

    # ------------------------------------------------------------------ checks
    def _check(self, act, labels, point_weights=None, denominator=None):
        """-> (device, contiguous point weights or None, 0-d denominator or None)"""
        C = self.num_class
        _require(isinstance(act, torch.Tensor) and isinstance(labels, torch.Tensor),
                 "SegmentationHead: act and labels must be tensors")
        _require(act.dim() == 3 and act.shape[2] == C,
                 "SegmentationHead expects (batch_size, num_points, num_class) activations")
        _require(labels.dim() == 2, "SegmentationHead expects (batch_size, num_points) labels")
        _require(tuple(labels.shape) == tuple(act.shape[:2]),
                 "SegmentationHead expects activations and labels to have the same batch size and number of points")
        if act.dtype not in _SFX:
            raise Conv3pInvalidArgument("SegmentationHead: activations must be float32 or float64")
        _require(labels.dtype in (torch.int32, torch.int64), "SegmentationHead: labels must be int32 or int64")
        _require(act.shape[0] * act.shape[1] > 0, "SegmentationHead: empty batch")
        pw = self._check_point_weights(point_weights, labels, act.dtype)
        den = self._check_denominator(denominator, act.device)
        _require(act.device.type == "cuda" and labels.device.type == "cuda",
                 "SegmentationHead: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        try:
            return _check_device(act, labels), pw, den
        except Conv3pRuntimeError as e:
            raise Conv3pInvalidArgument(str(e))

    def _check_point_weights(self, point_weights, labels, dtype):
        if point_weights is None:
            return None
        _require(isinstance(point_weights, torch.Tensor), "SegmentationHead: point_weights must be a tensor")
        _require(tuple(point_weights.shape) == tuple(labels.shape),
                 "SegmentationHead expects (batch_size, num_points) point_weights")
        _require(point_weights.dtype == dtype, "SegmentationHead: point_weights must have the activations' dtype")
        _require(point_weights.device == labels.device, "SegmentationHead: point_weights must be on the labels' device")
        return point_weights.contiguous()

    def _check_denominator(self, denominator, dev):
        if denominator is None:
            return None
        _require(self.reduction != "points", "SegmentationHead: denominator= goes with reduction 'nonzero_weights' or "
                                             "'sum_weights' (use global_points with 'points')")
        _require(isinstance(denominator, torch.Tensor) and denominator.numel() == 1 and denominator.dtype == torch.float64,
                 "SegmentationHead: denominator must be a float64 tensor of one element (see weight_total())")
        _require(denominator.device == dev, "SegmentationHead: denominator must be on the activations' device")
        return denominator.reshape(())

    def _class_weights_on(self, dev, dtype):
        if self.class_weights is None:
            return None
        key = (dev, dtype)
        if key not in self._cw:
            self._cw[key] = self.class_weights.to(dev, dtype)
        return self._cw[key]

    @staticmethod
    def _int32(labels):
        labels = labels.contiguous()
        return labels if labels.dtype == torch.int32 else labels.to(torch.int32)   # once; the kernels read int32

    def _weight_total(self, labels32, pw, dtype, dev):
        """{sum of the point weights, points with a non-zero weight}: float64[2] on the device."""
        lib = _lib.load()
        rows, C = labels32.numel(), self.num_class
        cw = self._class_weights_on(dev, dtype)
        total = torch.empty(2, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            ws = _workspace(dev, lib.conv3p_seg_head_weighted_workspace_bytes(rows, C), _HEADS)
            _call(getattr(lib, "conv3p_seg_weight_total_" + _SFX[dtype][0]), labels32.data_ptr(), rows, C,
                  cw.data_ptr() if cw is not None else None, pw.data_ptr() if pw is not None else None,
                  total.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        return total

    def _run(self, act, labels, points, need_grad, need_pred, point_weights=None, denominator=None, confusion=False):
        _require(self.reduction == "points" or points is None,
                 "SegmentationHead: global_points goes with reduction 'points' (pass the all-reduced weight_total() as "
                 "denominator= instead)")
        dev, pw, den = self._check(act, labels, point_weights, denominator)
        lib = _lib.load()
        B, N, C = act.shape
        rows = B * N
        act = act.contiguous()
        labels = self._int32(labels)
        sfx, real, _ = _SFX[act.dtype]
        if self.reduction == "points":
            scale = 1.0 / float(points if points is not None else rows)
        else:
            scale = 1.0
            if den is None:
                den = self._weight_total(labels, pw, act.dtype, dev)[0 if self.reduction == "sum_weights" else 1]
        cw = self._class_weights_on(dev, act.dtype)
        dact = torch.empty_like(act) if need_grad else None
        pred = torch.empty((B, N), dtype=torch.int32, device=dev) if need_pred else None
        loss_sum = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(2 + 3 * C, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            ws = _workspace(dev, lib.conv3p_seg_head_weighted_workspace_bytes(rows, C), _HEADS)
            _call(getattr(lib, "conv3p_seg_head_weighted_" + sfx), act.data_ptr(), labels.data_ptr(), rows, C,
                  cw.data_ptr() if cw is not None else None, pw.data_ptr() if pw is not None else None,
                  self.label_smoothing, real(scale), den.data_ptr() if den is not None else None,
                  dact.data_ptr() if dact is not None else None, pred.data_ptr() if pred is not None else None,
                  loss_sum.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            conf = None
            if confusion:
                conf = torch.empty((C, C), dtype=torch.int64, device=dev)
                ws = _workspace(dev, lib.conv3p_seg_confusion_workspace_bytes(rows, C), _HEADS)
                _call(lib.conv3p_seg_confusion, labels.data_ptr(), pred.data_ptr(), rows, C, conf.data_ptr(), ws.data_ptr(),
                      ws.numel(), stream)
        self._counts = counts
        self._confusion = conf
        if den is None:
            self._loss = loss_sum * scale
        else:
            self._loss = torch.where(den != 0, loss_sum / den, torch.zeros_like(loss_sum))
        return dact, pred

    # ------------------------------------------------------------------ public
    def loss(self, act, labels, global_points=None, need_pred=False, point_weights=None, denominator=None):
        """act (B, N, C) float32/float64, labels (B, N) int32/int64 -> (loss, dact), or (loss, dact, pred) with need_pred.

        loss: 0-d device tensor (float64, no synchronisation): sum of the point losses / global_points (default B*N);
        dact: dL/dact, what Conv3pStack.backward([dact]) takes.
        point_weights: (B, N) tensor of the activations' dtype on their device, or None (= 1).
        Data parallel: pass global_points = the points of ALL ranks, as ClassificationHead.loss(global_batch=...):
        distributed.py sums gradients across ranks, so each rank's gradient is scaled by the global count.
        Under reduction "nonzero_weights" / "sum_weights" the count is data dependent: each rank calls
        weight_total(labels, point_weights), all-reduces (sums) that device tensor and passes it as denominator=; without
        denominator= the head computes the local total itself (single-rank training)."""
        _require(global_points is None or global_points > 0, "SegmentationHead: global_points must be positive")
        dact, pred = self._run(act, labels, global_points, True, need_pred, point_weights, denominator)
        return (self._loss, dact, pred) if need_pred else (self._loss, dact)

    def weight_total(self, labels, point_weights=None, dtype=torch.float32):
        """The denominator of this head's reduction for one batch: a 0-d float64 device tensor (no synchronisation) --
        the number of points with a non-zero weight ("nonzero_weights") or the sum of the weights ("sum_weights"), with
        weight = class_weights[label] * point_weights[point] and 0 for an ignored point.  dtype: the activations'
        element type (the weights are multiplied in it; taken from point_weights when those are given)."""
        _require(self.reduction != "points", "SegmentationHead.weight_total(): reduction 'points' has no weight total")
        _require(isinstance(labels, torch.Tensor) and labels.dim() == 2 and labels.numel() > 0,
                 "SegmentationHead expects (batch_size, num_points) labels")
        _require(labels.dtype in (torch.int32, torch.int64), "SegmentationHead: labels must be int32 or int64")
        _require(labels.device.type == "cuda",
                 "SegmentationHead: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        if point_weights is not None:
            dtype = point_weights.dtype
        if dtype not in _SFX:
            raise Conv3pInvalidArgument("SegmentationHead: weights must be float32 or float64")
        pw = self._check_point_weights(point_weights, labels, dtype)
        total = self._weight_total(self._int32(labels), pw, dtype, labels.device)
        return total[0 if self.reduction == "sum_weights" else 1]

    def evaluate(self, act, labels, point_weights=None, confusion=False):
        """No gradient: -> (pred (B, N) int32, counts).  The mean loss of the call (this head's weights, smoothing and
        reduction, the local denominator) is kept for accumulate().  confusion=True: counts["confusion"] is the
        (C, C) int64 device matrix [label][pred] over the valid points of the call."""
        _, pred = self._run(act, labels, None, False, True, point_weights, None, confusion)
        return pred, self.counts()

    def counts(self):
        """The last call's counters: the device int64 tensor under "all" and its views correct, invalid, seen,
        correct_class, predicted; after evaluate(..., confusion=True) also "confusion".  A caller in a data-parallel
        run all-reduces "all" (and "confusion") as is."""
        if self._counts is None:
            raise Conv3pRuntimeError("SegmentationHead.counts(): no call yet")
        out = split_counts(self._counts, self.num_class)
        out["all"] = self._counts
        if self._confusion is not None:
            out["confusion"] = self._confusion
        return out

    def last_loss(self):
        """The last call's mean loss (0-d float64 device tensor)."""
        return self._loss

    def accumulate(self):
        """Add the last call's counters, mean loss and (if it has one) confusion matrix to the epoch totals: on the
        device, no synchronisation."""
        if self._counts is None:
            raise Conv3pRuntimeError("SegmentationHead.accumulate(): no call yet")
        if self._tot_counts is None:
            self._tot_counts = self._counts.clone()
            self._tot_loss = self._loss.clone()
        else:
            self._tot_counts += self._counts
            self._tot_loss += self._loss
        if self._confusion is not None:
            if self._tot_confusion is None:
                self._tot_confusion = self._confusion.clone()
            else:
                self._tot_confusion += self._confusion
        self._batches += 1

    def summary(self, reset=True):
        """Synchronises.  The epoch numbers of train_scene_seg_s3dis.py:157-159 -- mean_loss (mean of the batches' mean
        losses), mean_accuracy, avg_class_accuracy -- plus per-class IoU = correct_class / (seen + predicted -
        correct_class), from everything accumulate() has added.  The reference divides 0 / 0 for a class it never saw;
        here such classes are left out of avg_class_accuracy and listed under unseen_classes (see summarize()).
        "confusion": the sum of the matrices of the accumulated evaluate(..., confusion=True) calls, if there were any."""
        if self._tot_counts is None:
            raise Conv3pRuntimeError("SegmentationHead.summary(): nothing accumulated")
        conf = self._tot_confusion.cpu().tolist() if self._tot_confusion is not None else None
        out = summarize(self._tot_counts.cpu().tolist(), float(self._tot_loss.cpu()), self._batches, self.num_class, conf)
        if reset:
            self._tot_counts = self._tot_loss = self._tot_confusion = None
            self._batches = 0
        return out
