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
"""
import torch

from . import _lib
from .conv3p_op import Conv3pInvalidArgument, Conv3pRuntimeError, _SFX, _call, _check_device, _require
from .head import _workspace


def split_counts(counts, num_class):
    """Views of a {correct, invalid, seen[C], correct_class[C], predicted[C]} vector (tensor or array)."""
    C = num_class
    return {"correct": counts[0], "invalid": counts[1], "seen": counts[2:2 + C], "correct_class": counts[2 + C:2 + 2 * C],
            "predicted": counts[2 + 2 * C:2 + 3 * C]}


def summarize(counts, loss_total, batches, num_class):
    """The epoch numbers from accumulated counters (an int64 CPU tensor / sequence of 2 + 3 C entries), the sum of the
    batches' mean losses and the number of batches.  Pure host arithmetic.

    mean_loss, mean_accuracy, avg_class_accuracy as printed by train_scene_seg_s3dis.py:157-159: loss_sum / batches,
    correct / seen points, mean over classes of correct_class / seen.  The reference divides 0 / 0 for a class that never
    occurred; here such classes are left out of the mean and listed under `unseen_classes`.  Ignored points
    (`invalid`) are in no ratio.  iou[c] = correct_class / (seen + predicted - correct_class), None where that is 0 / 0;
    mean_iou is over the classes that have one."""
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
    return {"mean_loss": float(loss_total) / batches if batches else float("nan"),
            "mean_accuracy": v["correct"] / seen_total if seen_total else float("nan"),
            "avg_class_accuracy": sum(acc) / len(acc) if acc else float("nan"),
            "unseen_classes": [k for k in range(num_class) if v["seen"][k] == 0],
            "iou": iou, "mean_iou": sum(have) / len(have) if have else float("nan"),
            "points": seen_total, "invalid": v["invalid"], "batches": int(batches)}


class SegmentationHead:
    """Loss, gradient and batch statistics of the segmentation model's (B, N, num_class) activation."""

    def __init__(self, num_class, device="cuda:0"):
        _require(isinstance(num_class, int) and num_class >= 2, "SegmentationHead: num_class must be an integer >= 2")
        self.num_class = num_class
        self.device = torch.device(device)
        self._counts = None           # int64[2 + 3 C] of the last call
        self._loss = None             # 0-d double: the last call's mean loss
        self._tot_counts = None
        self._tot_loss = None
        self._batches = 0

    # ------------------------------------------------------------------ checks
    def _check(self, act, labels):
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
        _require(act.device.type == "cuda" and labels.device.type == "cuda",
                 "SegmentationHead: tensors must live on a HIP device (no CPU path in pointwise_amd)")
        try:
            return _check_device(act, labels)
        except Conv3pRuntimeError as e:
            raise Conv3pInvalidArgument(str(e))

    def _run(self, act, labels, points, need_grad, need_pred):
        dev = self._check(act, labels)
        lib = _lib.load()
        B, N, C = act.shape
        rows = B * N
        scale = 1.0 / float(points if points is not None else rows)
        act = act.contiguous()
        labels = labels.contiguous()
        if labels.dtype != torch.int32:
            labels = labels.to(torch.int32)          # once; the kernel reads int32
        sfx, real, _ = _SFX[act.dtype]
        dact = torch.empty_like(act) if need_grad else None
        pred = torch.empty((B, N), dtype=torch.int32, device=dev) if need_pred else None
        loss_sum = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(2 + 3 * C, dtype=torch.int64, device=dev)
        need = lib.conv3p_seg_head_workspace_bytes(rows, C)
        with torch.cuda.device(dev):
            ws = _workspace(dev, need)
            _call(getattr(lib, "conv3p_seg_head_" + sfx), act.data_ptr(), labels.data_ptr(), rows, C, real(scale),
                  dact.data_ptr() if dact is not None else None, pred.data_ptr() if pred is not None else None,
                  loss_sum.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream(dev).cuda_stream)
        self._counts = counts
        self._loss = loss_sum * scale
        return dact, pred

    # ------------------------------------------------------------------ public
    def loss(self, act, labels, global_points=None, need_pred=False):
        """act (B, N, C) float32/float64, labels (B, N) int32/int64 -> (loss, dact), or (loss, dact, pred) with need_pred.

        loss: 0-d device tensor (float64, no synchronisation): sum of the point losses / global_points (default B*N);
        dact: dL/dact, what Conv3pStack.backward([dact]) takes.
        Data parallel: pass global_points = the points of ALL ranks, as ClassificationHead.loss(global_batch=...):
        distributed.py sums gradients across ranks, so each rank's gradient is scaled by the global count."""
        _require(global_points is None or global_points > 0, "SegmentationHead: global_points must be positive")
        dact, pred = self._run(act, labels, global_points, True, need_pred)
        return (self._loss, dact, pred) if need_pred else (self._loss, dact)

    def evaluate(self, act, labels):
        """No gradient: -> (pred (B, N) int32, counts).  The mean loss of the call is kept for accumulate()."""
        _, pred = self._run(act, labels, None, False, True)
        return pred, self.counts()

    def counts(self):
        """The last call's counters: the device int64 tensor under "all" and its views correct, invalid, seen,
        correct_class, predicted.  A caller in a data-parallel run all-reduces "all" as is."""
        if self._counts is None:
            raise Conv3pRuntimeError("SegmentationHead.counts(): no call yet")
        out = split_counts(self._counts, self.num_class)
        out["all"] = self._counts
        return out

    def last_loss(self):
        """The last call's mean loss (0-d float64 device tensor)."""
        return self._loss

    def accumulate(self):
        """Add the last call's counters and mean loss to the epoch totals: on the device, no synchronisation."""
        if self._counts is None:
            raise Conv3pRuntimeError("SegmentationHead.accumulate(): no call yet")
        if self._tot_counts is None:
            self._tot_counts = self._counts.clone()
            self._tot_loss = self._loss.clone()
        else:
            self._tot_counts += self._counts
            self._tot_loss += self._loss
        self._batches += 1

    def summary(self, reset=True):
        """Synchronises.  The epoch numbers of train_scene_seg_s3dis.py:157-159 -- mean_loss (mean of the batches' mean
        losses), mean_accuracy, avg_class_accuracy -- plus per-class IoU = correct_class / (seen + predicted -
        correct_class), from everything accumulate() has added.  The reference divides 0 / 0 for a class it never saw;
        here such classes are left out of avg_class_accuracy and listed under unseen_classes (see summarize())."""
        if self._tot_counts is None:
            raise Conv3pRuntimeError("SegmentationHead.summary(): nothing accumulated")
        out = summarize(self._tot_counts.cpu().tolist(), float(self._tot_loss.cpu()), self._batches, self.num_class)
        if reset:
            self._tot_counts = self._tot_loss = None
            self._batches = 0
        return out
