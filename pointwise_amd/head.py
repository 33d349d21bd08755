"""The dense head of the reference's classification model, on the hand-written FC kernels.

/root/reference/pointcnn2_acsd.py:68-77
    feat = concat(relu1..relu4)                 (B, N, 36)       -- the conv3p stack's output (stack.Conv3pStack)
    view = reshape(feat, [-1, n * 36])          (B, N*36)
    fc1  = fully_connected(view, 512, selu)     W1: (N*36, 512)  -- 151 MB for N = 2048: the model's big object
    drop = dropout_selu(fc1, rate 0.5, training)                 -- selu.py:35-70
    fc2  = fully_connected(drop, num_class, selu)
loss: mean sparse softmax cross-entropy (pointcnn2_acsd.py:79-90).

tf.contrib.layers.fully_connected(x, n, activation_fn) is activation(x . W + b).  Both layers run through
conv3p_fc_forward_f32 / conv3p_fc_backward_f32 (include/conv3p.h): W streamed once per pass, exact fp32 products on
v_mfma_f32_32x32x2_f32, bitwise reproducible.

Everything between fc1's output and fc1's backward -- dropout_selu, fc2, the loss, the batch statistics of
train_modelnet40_acsd.py:136-146, fc2's backward and (with an optimizer) the update of W2 / b2 -- is ONE call of two
launches, conv3p_cls_tail_f32 / _step_f32 (csrc/conv3p_cls_tail.hpp): ClassificationHead.forward_backward / evaluate
and the functional classification_tail.  Its dropout mask is a function of (seed, step, row, column) (Philox4x32-10
on the device), so a step is reproducible from (seed, step).  forward / loss / backward remain as the composition of
the fc kernels and elementwise torch ops (about 27 launches for the same work; fc2 there needs num_class % 8 == 0).

Data parallelism (one process per GPU): the gradient of W1 is 151 MB per rank -- four orders of magnitude more than
the conv3p filters' 29 KB.  `sharded_gradient_step` reduce-scatters it (every rank receives the SUM of one 1/world
slice: half the traffic of an all-reduce), lets the caller update only that slice (optimizer state is sharded the
same way) and all-gathers the updated weights; launched right after the head's backward on its own stream it runs
under the whole conv3p backward.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._host import (_HEADS, Conv3pInvalidArgument, Conv3pRuntimeError, _call, _check_device, _ptr, _require, _stream,
                    _workspace)

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946

def _check_fc(x, W, b):
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[0]:
        raise Conv3pInvalidArgument("fully_connected: x (M, K) and W (K, N) expected")
    if b is not None and tuple(b.shape) != (W.shape[1],):
        raise Conv3pInvalidArgument("fully_connected: bias must have N entries")
    for t in (x, W) + ((b,) if b is not None else ()):
        if t.dtype != torch.float32:
            raise Conv3pInvalidArgument("fully_connected: float32 only")


def fully_connected(x, W, b=None, selu=True):
    """activation(x . W + b), activation = SELU or identity (tf.contrib.layers.fully_connected)."""
    lib = _lib.load()
    _check_fc(x, W, b)
    dev = _check_device(x, W)
    M, K = x.shape
    N = W.shape[1]
    x, W = x.contiguous(), W.contiguous()
    y = torch.empty((M, N), dtype=torch.float32, device=dev)
    need = lib.conv3p_fc_workspace_bytes(M, K, N)
    with torch.cuda.device(dev):
        ws = _workspace(dev, need, _HEADS)
        _call(lib.conv3p_fc_forward_f32, x.data_ptr(), W.data_ptr(), _ptr(b), M, K, N, 1 if selu else 0, y.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream(dev))
    return y


def fully_connected_grad(x, W, y, dy, selu=True, need_dx=True, dW_out=None, db_out=None):
    """Gradients of fully_connected given its OUTPUT y and dL/dy -> (dx or None, dW, db).

    Narrower than the forward (N % 8 == 0, N <= 1024, M <= 128): the dW pass keeps all of dz in LDS, so batches of
    33 .. 64 rows need N <= 632 and batches of 65 .. 128 rows N <= 312 (Conv3pRuntimeError "unsupported" otherwise,
    before anything is launched; conv3p_fc_workspace_bytes does not reflect this).  A ClassificationHead with
    hidden = 512 therefore runs forward at a batch of 65 .. 128 clouds and fails in backward; MomentumOptimizer.
    fused_fc_step has the same limits.  An empty batch (M = 0) gives dW = 0 and db = 0."""
    lib = _lib.load()
    _check_fc(x, W, None)
    dev = _check_device(x, W, y, dy)
    M, K = x.shape
    N = W.shape[1]
    x, W, y, dy = x.contiguous(), W.contiguous(), y.contiguous(), dy.contiguous()
    dx = torch.empty_like(x) if need_dx else None
    dW = dW_out if dW_out is not None else torch.empty_like(W)
    db = db_out if db_out is not None else torch.empty((N,), dtype=torch.float32, device=dev)
    if not dW.is_contiguous() or tuple(dW.shape) != (K, N):
        raise Conv3pInvalidArgument("dW_out must be a contiguous (K, N) tensor")
    need = lib.conv3p_fc_workspace_bytes(M, K, N)
    with torch.cuda.device(dev):
        ws = _workspace(dev, need, _HEADS)
        _call(lib.conv3p_fc_backward_f32, x.data_ptr(), W.data_ptr(), y.data_ptr(), dy.data_ptr(), M, K, N,
              1 if selu else 0, _ptr(dx), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    return dx, dW, db


def dropout_selu_constants(rate, alpha=-1.7580993408473766, fixed_mean=0.0, fixed_var=1.0):
    """a, b of selu.py:59-61 for keep_prob = 1 - rate."""
    keep = 1.0 - rate
    a = np.sqrt(fixed_var / (keep * ((1 - keep) * (alpha - fixed_mean) ** 2 + fixed_var)))
    b = fixed_mean - a * (keep * fixed_mean + (1 - keep) * alpha)
    return float(a), float(b), float(alpha)


def dropout_selu(x, rate, training, keep_mask=None):
    """selu.py:35-70: ret = a * (x * keep + alpha' * (1 - keep)) + b in training, identity otherwise.
    keep_mask (0/1 tensor like x): the Bernoulli(keep_prob) draw; None draws floor(keep_prob + U[0,1))."""
    if not training or rate == 0.0:
        return x, None
    a, b, alpha = dropout_selu_constants(rate)
    if keep_mask is None:
        keep_mask = torch.floor((1.0 - rate) + torch.rand_like(x))            # selu.py:53-55
    return a * (x * keep_mask + alpha * (1 - keep_mask)) + b, keep_mask        # :56, :62


def classification_tail(fc1, W2, b2, labels, rate=0.5, training=True, keep_mask=None, seed=0, step=0, grad_scale=None,
                        need_grad=True, need_keep=False, accum_W2=None, accum_b2=None, lr=None, momentum=None,
                        dW2_out=None, db2_out=None):
    """conv3p_cls_tail_f32 / _step_f32 (include/conv3p.h) on the current stream: everything between fc1's output
    fc1 (M, H) and fc1's backward.  Returns a dict: logits (M, C), pred int32 (M), loss_sum (0-d float64, the UNSCALED
    sum of the row losses), counts int64 (2 + 3 C: the layout of seg_head.split_counts), and with need_grad dfc1 (M, H),
    dW2 (H, C), db2 (C); keep (uint8 (M, H)) with need_keep when dropout applies (training and rate > 0).

    keep_mask: float 0 / 1 (M, H); None draws it on the device from (seed, step).  grad_scale: default 1 / M.
    accum_W2 / accum_b2 (both or neither, with lr and momentum): W2, b2 and the accumulators are stepped in place
    (ApplyMomentum), dW2 / db2 are not produced (None); dfc1 comes from the W2 of before the call."""
    for t, what in ((fc1, "fc1"), (W2, "W2"), (b2, "b2"), (labels, "labels")):
        _require(isinstance(t, torch.Tensor), "classification_tail: %s must be a tensor" % what)
    _require(fc1.dim() == 2 and W2.dim() == 2 and fc1.shape[1] == W2.shape[0],
             "classification_tail: fc1 (M, H) and W2 (H, C) expected")
    M, H = fc1.shape
    C = W2.shape[1]
    _require(tuple(b2.shape) == (C,), "classification_tail: b2 must have C entries")
    _require(tuple(labels.shape) == (M,), "classification_tail: labels must have M entries")
    _require(M > 0, "classification_tail: empty batch")
    _require(C >= 2, "classification_tail: at least two classes")
    for t in (fc1, W2, b2):
        if t.dtype != torch.float32:
            raise Conv3pInvalidArgument("classification_tail: float32 only")
    _require(labels.dtype in (torch.int32, torch.int64), "classification_tail: labels must be int32 or int64")
    _require(not training or 0.0 <= rate < 1.0, "classification_tail: rate must be in [0, 1)")
    _require((accum_W2 is None) == (accum_b2 is None), "classification_tail: accum_W2 and accum_b2 go together")
    stepping = accum_W2 is not None
    if stepping:
        _require(need_grad, "classification_tail: the update needs the gradient pass")
        _require(lr is not None and momentum is not None, "classification_tail: the update needs lr and momentum")
        for t, ref in ((accum_W2, W2), (accum_b2, b2)):
            _require(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == ref.numel() and
                     t.is_contiguous(), "classification_tail: an accumulator must match its parameter")
        _require(W2.is_contiguous() and b2.is_contiguous(), "classification_tail: W2 and b2 are updated in place: contiguous")
    if keep_mask is not None:
        _require(isinstance(keep_mask, torch.Tensor) and tuple(keep_mask.shape) == (M, H) and
                 keep_mask.dtype == torch.float32, "classification_tail: keep_mask must be a float32 (M, H) tensor")
    _require(0 <= int(seed) < 1 << 64 and 0 <= int(step) < 1 << 64, "classification_tail: seed and step are uint64")
    for t in (fc1, W2, b2, labels) + ((keep_mask,) if keep_mask is not None else ()) + \
            ((accum_W2, accum_b2) if stepping else ()):
        _require(t.device.type == "cuda", "classification_tail: tensors must live on a HIP device (no CPU path in pointwise_amd)")
    dev = _check_device(fc1, W2, b2, labels)
    fc1, W2, b2, labels = fc1.contiguous(), W2.contiguous(), b2.contiguous(), labels.contiguous()
    if labels.dtype != torch.int32:
        labels = labels.to(torch.int32)
    if keep_mask is not None:
        keep_mask = keep_mask.contiguous()
    dropout = bool(training) and rate > 0.0
    f32 = dict(dtype=torch.float32, device=dev)
    logits = torch.empty((M, C), **f32)
    pred = torch.empty((M,), dtype=torch.int32, device=dev)
    loss_sum = torch.empty((), dtype=torch.float64, device=dev)
    counts = torch.empty(2 + 3 * C, dtype=torch.int64, device=dev)
    dfc1 = torch.empty((M, H), **f32) if need_grad else None
    dW2 = db2 = None
    if need_grad and not stepping:
        dW2 = dW2_out if dW2_out is not None else torch.empty((H, C), **f32)
        db2 = db2_out if db2_out is not None else torch.empty((C,), **f32)
        _require(dW2.is_contiguous() and tuple(dW2.shape) == (H, C) and db2.is_contiguous() and tuple(db2.shape) == (C,)
                 and dW2.dtype == torch.float32 and db2.dtype == torch.float32,
                 "classification_tail: dW2_out / db2_out must be contiguous float32 (H, C) / (C)")
    keep = torch.empty((M, H), dtype=torch.uint8, device=dev) if need_keep and dropout else None
    scale = float(grad_scale) if grad_scale is not None else 1.0 / M
    lib = _lib.load()
    need = lib.conv3p_cls_tail_workspace_bytes(M, H, C)
    with torch.cuda.device(dev):
        ws = _workspace(dev, need, _HEADS)
        head = (fc1.data_ptr(), W2.data_ptr(), b2.data_ptr(), labels.data_ptr(), M, H, C, 1 if training else 0, float(rate),
                _ptr(keep_mask), int(seed), int(step), scale, logits.data_ptr(), pred.data_ptr(), _ptr(dfc1))
        tail = (_ptr(keep), loss_sum.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        if stepping:
            _call(lib.conv3p_cls_tail_step_f32, *head, accum_W2.data_ptr(), accum_b2.data_ptr(), float(lr), float(momentum),
                  *tail)
        else:
            _call(lib.conv3p_cls_tail_f32, *head, _ptr(dW2), _ptr(db2), *tail)
    return {"logits": logits, "pred": pred, "loss_sum": loss_sum, "counts": counts, "dfc1": dfc1, "dW2": dW2, "db2": db2,
            "keep": keep}


class ClassificationHead:
    """fc1 (N*36 -> 512, selu) -> dropout_selu -> fc2 (512 -> num_class, selu); parameters live on `device`."""

    def __init__(self, n_points, num_class=40, feat_channels=36, hidden=512, device="cuda:0", seed=0, rate=0.5):
        g = torch.Generator().manual_seed(seed)
        K = n_points * feat_channels
        # variance-scaling (FAN_IN) initialisation as recommended next to selu (selu.py:29-31); zero biases
        self.W1 = (torch.randn((K, hidden), generator=g) * (1.0 / np.sqrt(K))).to(device)
        self.b1 = torch.zeros(hidden, device=device)
        self.W2 = (torch.randn((hidden, num_class), generator=g) * (1.0 / np.sqrt(hidden))).to(device)
        self.b2 = torch.zeros(num_class, device=device)
        self.rate = rate
        self.dW1 = torch.empty_like(self.W1)           # 151 MB for N = 2048: allocated once
        self.db1 = torch.empty_like(self.b1)
        self.dW2 = torch.empty_like(self.W2)
        self.db2 = torch.empty_like(self.b2)
        self._saved = None
        self._fc1_stepped = False                      # the last backward() updated W1 / b1 itself: dW1 / db1 not written
        self._fc2_stepped = False                      # the last forward_backward() updated W2 / b2 itself
        self.num_class = num_class
        self.seed = int(seed)
        self._calls = 0                                # forward_backward()'s default `step`
        self._counts = None                            # int64[2 + 3 C] of the last fused call
        self._loss = None                              # 0-d double: its mean loss
        self._tot_counts = None
        self._tot_loss = None
        self._batches = 0

    def forward(self, feat, training=True, keep_mask=None):
        B = feat.shape[0]
        view = feat.reshape(B, -1)                                              # pointcnn2_acsd.py:70
        fc1 = fully_connected(view, self.W1, self.b1, selu=True)                # :71
        drop, mask = dropout_selu(fc1, self.rate, training, keep_mask)          # :73
        fc2 = fully_connected(drop, self.W2, self.b2, selu=True)                # :75
        self._saved = (view, fc1, drop, mask, fc2, feat.shape)
        return fc2

    def loss(self, logits, labels, global_batch=None):
        """mean sparse softmax cross-entropy (pointcnn2_acsd.py:79-90) and its gradient w.r.t. the logits.

        Data parallel: pass global_batch = the batch over ALL ranks.  distributed.py reduces gradients with SUM, so the
        gradient of the reference's mean over the global batch is each rank's dlogits / global_batch (dividing by
        the local batch would scale every gradient by the world size).  The returned loss is the local shard's mean."""
        logp = torch.log_softmax(logits, dim=1)
        idx = labels.long().unsqueeze(1)
        e = -(logp.gather(1, idx)).mean()
        dlogits = torch.softmax(logits, dim=1)
        dlogits.scatter_add_(1, idx, -torch.ones_like(idx, dtype=dlogits.dtype))
        return e, dlogits / float(global_batch if global_batch is not None else logits.shape[0])

    def backward(self, dlogits, optimizer=None):
        """-> dL/dfeat (B, N, 36); parameter gradients in self.dW1, db1, dW2, db2.

        optimizer (an optim.MomentumOptimizer that owns W1 and b1; single-GPU runs): fc1's gradient pass applies the
        update itself (optimizer.fused_fc_step) -- W1 and b1 are stepped on return, dW1 / db1 are NOT written and
        gradients() reports None for them; W2, b2 and everything else are the caller's optimizer.step().  Data-parallel
        runs keep the default: the gradient has to cross ranks before anything is updated.  So does an optimizer that
        is not `fusable` (use_nesterov, clip_norm, skip_nonfinite: its step needs every gradient first): dW1 / db1 are
        written and optimizer.step(gradients) updates everything."""
        view, fc1, drop, mask, fc2, shape = self._saved
        ddrop, _, _ = fully_connected_grad(drop, self.W2, fc2, dlogits, selu=True, dW_out=self.dW2, db_out=self.db2)
        if mask is not None:
            a, _, _ = dropout_selu_constants(self.rate)
            dfc1 = ddrop * (a * mask)
        else:
            dfc1 = ddrop
        self._fc2_stepped = False
        return self._fc1_backward(view, fc1, dfc1, optimizer).reshape(shape)

    def _fc1_backward(self, view, fc1, dfc1, optimizer):
        self._fc1_stepped = optimizer is not None and optimizer.fusable and optimizer.owns(self.W1, self.b1)
        if self._fc1_stepped:
            return optimizer.fused_fc_step(view.contiguous(), self.W1, self.b1, fc1, dfc1.contiguous(), selu=True)
        dview, _, _ = fully_connected_grad(view, self.W1, fc1, dfc1, selu=True, dW_out=self.dW1, db_out=self.db1)
        return dview

    # ------------------------------------------------------------------ the fused tail
    def _check_batch(self, feat, labels):
        _require(isinstance(feat, torch.Tensor) and isinstance(labels, torch.Tensor),
                 "ClassificationHead: feat and labels must be tensors")
        _require(feat.dim() >= 2 and feat.shape[0] > 0, "ClassificationHead: feat must be a non-empty (B, ...) batch")
        _require(feat[0].numel() == self.W1.shape[0], "ClassificationHead: feat must have %d values per cloud" % self.W1.shape[0])
        _require(labels.dim() == 1 and labels.shape[0] == feat.shape[0], "ClassificationHead: labels must have B entries")

    def forward_backward(self, feat, labels, optimizer=None, keep_mask=None, seed=None, step=None, global_batch=None,
                         training=True):
        """One training step of the head: fc1, the fused tail (conv3p_cls_tail_*: dropout_selu, fc2, loss, statistics,
        fc2's backward), fc1's backward -> (loss, dL/dfeat).

        loss: 0-d float64 device tensor, the local batch's mean (not synchronised).  global_batch scales the gradient as
        loss() documents.  keep_mask (B, hidden) float 0 / 1 fixes the dropout draw; otherwise it is drawn on the
        device from (seed, step): seed defaults to the constructor's, step to the number of forward_backward() calls
        before this one that were not given a step.  Gradients land in dW1, db1, dW2, db2 -- except what `optimizer` (an
        optim.MomentumOptimizer) owns: W1 / b1 are stepped by fc1's gradient pass as in backward(), W2 / b2 by the
        tail's second launch, and gradients() reports None for them (an optimizer that is not `fusable` owns nothing in
        this sense: all four gradients are written for its step()).  The global step is the caller's
        optimizer.step(gradients...) to advance.  counts() / accumulate() / summary() refer to this call; its logits
        and predictions stay in .logits / .pred."""
        self._check_batch(feat, labels)
        _require(global_batch is None or global_batch > 0, "ClassificationHead: global_batch must be positive")
        B = feat.shape[0]
        if step is None:
            step = self._calls
            self._calls += 1
        view = feat.reshape(B, -1)
        fc1 = fully_connected(view, self.W1, self.b1, selu=True)
        own2 = optimizer is not None and optimizer.fusable and optimizer.owns(self.W2, self.b2)
        kw = {}
        if own2:
            _require(optimizer.accums[optimizer._index(self.W2, "W2")].numel() == self.W2.numel(),
                     "MomentumOptimizer: W2's accumulator is sharded")
            kw = dict(accum_W2=optimizer.accums[optimizer._index(self.W2, "W2")],
                      accum_b2=optimizer.accums[optimizer._index(self.b2, "b2")], lr=optimizer.learning_rate(),
                      momentum=optimizer.momentum)
        else:
            kw = dict(dW2_out=self.dW2, db2_out=self.db2)
        out = classification_tail(fc1, self.W2, self.b2, labels, rate=self.rate, training=training, keep_mask=keep_mask,
                                  seed=self.seed if seed is None else seed, step=step,
                                  grad_scale=1.0 / float(global_batch if global_batch is not None else B), **kw)
        self._fc2_stepped = own2
        self._counts = out["counts"]
        self._loss = out["loss_sum"] * (1.0 / B)
        self._saved = None
        self.logits, self.pred = out["logits"], out["pred"]
        return self._loss, self._fc1_backward(view, fc1, out["dfc1"], optimizer).reshape(feat.shape)

    def evaluate(self, feat, labels):
        """No dropout, no gradient: -> (pred (B) int32, counts).  The call's mean loss is kept for accumulate()."""
        self._check_batch(feat, labels)
        B = feat.shape[0]
        fc1 = fully_connected(feat.reshape(B, -1), self.W1, self.b1, selu=True)
        out = classification_tail(fc1, self.W2, self.b2, labels, rate=self.rate, training=False, need_grad=False)
        self._counts = out["counts"]
        self._loss = out["loss_sum"] * (1.0 / B)
        self.logits, self.pred = out["logits"], out["pred"]
        return out["pred"], self.counts()

    def counts(self):
        """The last fused call's counters, as SegmentationHead.counts(): the device int64 tensor under "all" and its
        views correct, invalid, seen, correct_class, predicted (units: clouds)."""
        from . import seg_head
        if self._counts is None:
            raise Conv3pRuntimeError("ClassificationHead.counts(): no forward_backward() / evaluate() yet")
        out = seg_head.split_counts(self._counts, self.num_class)
        out["all"] = self._counts
        return out

    def last_loss(self):
        """The last fused call's mean loss (0-d float64 device tensor)."""
        return self._loss

    def accumulate(self):
        """Add the last fused call's counters and mean loss to the epoch totals: on the device, no synchronisation."""
        if self._counts is None:
            raise Conv3pRuntimeError("ClassificationHead.accumulate(): no forward_backward() / evaluate() yet")
        if self._tot_counts is None:
            self._tot_counts = self._counts.clone()
            self._tot_loss = self._loss.clone()
        else:
            self._tot_counts += self._counts
            self._tot_loss += self._loss
        self._batches += 1

    def summary(self, reset=True):
        """Synchronises.  mean_loss (mean of the batches' mean losses), mean_accuracy, avg_class_accuracy as printed by
        train_modelnet40_acsd.py:158-160, from everything accumulate() has added (seg_head.summarize: classes never
        seen are left out of avg_class_accuracy and listed under unseen_classes)."""
        from . import seg_head
        if self._tot_counts is None:
            raise Conv3pRuntimeError("ClassificationHead.summary(): nothing accumulated")
        out = seg_head.summarize(self._tot_counts.cpu().tolist(), float(self._tot_loss.cpu()), self._batches, self.num_class)
        if reset:
            self._tot_counts = self._tot_loss = None
            self._batches = 0
        return out

    def parameters(self):
        return [self.W1, self.b1, self.W2, self.b2]

    def gradients(self):
        """In parameters() order; None for W1 and b1 when the last backward() / forward_backward() stepped them itself,
        and for W2 and b2 when the last forward_backward() did (what MomentumOptimizer.step skips)."""
        g1 = [None, None] if self._fc1_stepped else [self.dW1, self.db1]
        return g1 + ([None, None] if self._fc2_stepped else [self.dW2, self.db2])
