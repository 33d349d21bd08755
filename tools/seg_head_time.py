"""developer: time the fused segmentation loss head (SegmentationHead.loss with predictions) against the torch
composition a user would write without it -- the op list of ClassificationHead.loss (log_softmax, gather, mean,
softmax, scatter_add, scale) plus argmax, compare and three bincounts -- at the three sizes of DESIGN.md section 5f.

Both in one process, alternated: 3 rounds x 20 calls each, a round timed with one pair of HIP events; every shape is
warmed up first.  Neither side synchronises inside a round.  Output: profiles/seg_head_time.txt (--out).

    python tools/seg_head_time.py [--out profiles/seg_head_time.txt]

--weighted: the same comparison for the weighted head (class and point weights, label smoothing 0.1, reduction
"sum_weights": the pre-pass over the labels is part of the call) at 65 536 x 13 and 131 072 x 41 -- the unweighted
head, the weighted head, the weighted head without the pre-pass (reduction "points"), the confusion kernel, and the
two torch compositions, each + backward + argmax + bincounts: F.cross_entropy(label_smoothing=) times the weights
(TensorFlow's rule: compared with the head, then timed) and F.cross_entropy(weight=, label_smoothing=) (torch's own
rule: timed only).  Output: profiles/seg_head_weighted_time.txt.

    python tools/seg_head_time.py --weighted [--out profiles/seg_head_weighted_time.txt]
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from pointwise_amd import _lib
from pointwise_amd.seg_head import SegmentationHead

SIZES = ((65536, 13, "cfg4: 16 x 4096 points, S3DIS"), (524288, 13, "param.json's batch: 128 x 4096"),
         (131072, 41, "SceneNN-like: 41 classes"))
ROUNDS, CALLS = 3, 20


def torch_composition(logits, labels, C):
    """(R, C) logits, (R,) int64 labels -> loss, dlogits, pred, correct, seen[C], correct_class[C], predicted[C]."""
    R = logits.shape[0]
    logp = torch.log_softmax(logits, dim=1)
    idx = labels.unsqueeze(1)
    e = -(logp.gather(1, idx)).mean()
    d = torch.softmax(logits, dim=1)
    d.scatter_add_(1, idx, -torch.ones_like(idx, dtype=d.dtype))
    d = d / float(R)
    pred = torch.argmax(logits, dim=1)
    hit = pred == labels
    return (e, d, pred, hit.sum(), torch.bincount(labels, minlength=C), torch.bincount(labels[hit], minlength=C),
            torch.bincount(pred, minlength=C))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS      # us per call


def event_bracket(lib, fn):
    """us per call of fn inside the library's own event brackets (all of them are accounted to seg_head_kernel)."""
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    total = 0.0
    for k in range(lib.conv3p_profile_kinds()):
        n, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
        lib.conv3p_profile_read(k, ctypes.byref(n), ctypes.byref(ms))
        if n.value and lib.conv3p_profile_name(k).decode() == "seg_head_kernel":
            total += ms.value
    lib.conv3p_profile_enable(0)
    lib.conv3p_profile_reset()
    return total * 1e3 / CALLS


def torch_weighted_composition(logits, labels, C, cw, pw, smoothing):
    """What a user writes without the head: the weighted, smoothed mean (divided by the sum of the weights), its
    gradient through autograd, argmax, and the counters by bincount.  The point's weight multiplies
    F.cross_entropy(label_smoothing=)'s per-point loss -- TensorFlow's rule, the one the head implements;
    F.cross_entropy(weight=, label_smoothing=) would weight the smoothing part class by class -- at the same op count."""
    x = logits.detach().requires_grad_(True)
    w = cw[labels] * pw
    rows = torch.nn.functional.cross_entropy(x, labels, label_smoothing=smoothing, reduction="none")
    loss = (rows * w).sum() / w.sum()
    loss.backward()
    pred = torch.argmax(logits, dim=1)
    hit = pred == labels
    return (loss.detach(), x.grad, pred, hit.sum(), torch.bincount(labels, minlength=C),
            torch.bincount(labels[hit], minlength=C), torch.bincount(pred, minlength=C),
            torch.bincount(labels * C + pred, minlength=C * C).view(C, C))


def torch_class_weighted_composition(logits, labels, C, cw, smoothing):
    """F.cross_entropy(weight=, label_smoothing=) + backward + argmax + bincounts: torch's own rule (the smoothing part
    weighted class by class, no per-point weights), so its numbers are not the head's -- timed, not compared."""
    x = logits.detach().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, labels, weight=cw, label_smoothing=smoothing)
    loss.backward()
    pred = torch.argmax(logits, dim=1)
    hit = pred == labels
    return (loss.detach(), x.grad, pred, hit.sum(), torch.bincount(labels, minlength=C),
            torch.bincount(labels[hit], minlength=C), torch.bincount(pred, minlength=C))


def main_weighted(out):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = ["weighted segmentation loss head (class + point weights, label smoothing 0.1), fp32, %s"
             % torch.cuda.get_device_name(dev),
             "us per call; %d rounds x %d calls, alternated, HIP events; 'kernels' = the library's event brackets" % (ROUNDS, CALLS),
             "unweighted = conv3p_seg_head_f32 through SegmentationHead's defaults: the parent commit's kernels, unchanged",
             "torch, TF rule = F.cross_entropy(label_smoothing=, reduction='none') x class and point weights / their sum,",
             "  backward, argmax, three bincounts and the C x C one: what the head computes, compared with it before timing",
             "torch, own rule = F.cross_entropy(weight=, label_smoothing=), backward, argmax, three bincounts: torch weights",
             "  the smoothing part class by class and has no point weights, so it is timed only"]
    for R, C, what in (SIZES[0], SIZES[2]):
        g = torch.Generator(device="cpu").manual_seed(R + C)
        act = torch.selu(2.0 * torch.randn(R, C, generator=g)).to(dev)
        lab64 = torch.randint(0, C, (R,), generator=g).to(dev)
        cw = (0.25 + 3.75 * torch.rand(C, generator=g)).to(dev)
        pw = (2.0 * torch.rand(R, generator=g)).to(dev)
        a3, l3, p3 = act.view(1, R, C), lab64.to(torch.int32).view(1, R), pw.view(1, R)
        plain = SegmentationHead(C, device=dev)
        full = SegmentationHead(C, device=dev, class_weights=cw, label_smoothing=0.1, reduction="sum_weights")
        nopre = SegmentationHead(C, device=dev, class_weights=cw, label_smoothing=0.1, reduction="points")
        pred = plain.loss(a3, l3, need_pred=True)[2]
        conf = torch.empty((C, C), dtype=torch.int64, device=dev)
        need = lib.conv3p_seg_confusion_workspace_bytes(R, C)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def confusion():
            rc = lib.conv3p_seg_confusion(l3.data_ptr(), pred.data_ptr(), R, C, conf.data_ptr(), ws.data_ptr(), need, stream)
            assert rc == 0
        fns = (("unweighted head (2 launches)", lambda: plain.loss(a3, l3, need_pred=True)),
               ("weighted head + pre-pass (4)", lambda: full.loss(a3, l3, need_pred=True, point_weights=p3)),
               ("weighted head, 'points' (2) ", lambda: nopre.loss(a3, l3, need_pred=True, point_weights=p3)),
               ("confusion kernel (2)        ", confusion),
               ("torch, TF rule              ", lambda: torch_weighted_composition(act, lab64, C, cw, pw, 0.1)),
               ("torch, own rule             ", lambda: torch_class_weighted_composition(act, lab64, C, cw, 0.1)))
        # agreement at the timed size
        loss, dact, wpred = fns[1][1]()
        confusion()
        ref = fns[4][1]()
        cnt = full.counts()
        torch.cuda.synchronize()
        assert torch.equal(wpred.view(-1).long(), ref[2]) and torch.equal(cnt["seen"], ref[4]) and torch.equal(conf, ref[7])
        assert abs(float(loss) - float(ref[0])) < 1e-5 * max(1.0, float(ref[0]))
        assert float((dact.view(R, C) - ref[1]).abs().max()) * R < 1e-4
        for _ in range(5):
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(ROUNDS):
            for t, (_, fn) in zip(times, fns):
                t.append(timed(fn))
        kern = [event_bracket(lib, fn) for _, fn in fns[:4]]
        lines.append("")
        lines.append("R x C = %d x %d  (%s)" % (R, C, what))
        for (name, _), t in zip(fns, times):
            lines.append("  %s  " % name + "  ".join("%8.1f" % v for v in t))
        lines.append("  ratio weighted + pre-pass / unweighted   " + "  ".join("%8.2f" % (w / u) for u, w in zip(times[0], times[1])))
        lines.append("  ratio weighted 'points' / unweighted     " + "  ".join("%8.2f" % (w / u) for u, w in zip(times[0], times[2])))
        lines.append("  ratio torch TF rule / weighted + pre-pass" + "  ".join("%8.2f" % (c / w) for w, c in zip(times[1], times[4])))
        lines.append("  ratio torch own rule / weighted + pre-pass" + "  ".join("%7.2f" % (c / w) for w, c in zip(times[1], times[5])))
        lines.append("  kernels: unweighted %.1f us, weighted + pre-pass %.1f us (ratio %.2f), weighted 'points' %.1f us "
                     "(ratio %.2f), confusion %.1f us" % (kern[0], kern[1], kern[1] / kern[0], kern[2], kern[2] / kern[0], kern[3]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--weighted", action="store_true", help="time the weighted head (see the module docstring)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                "seg_head_weighted_time.txt" if args.weighted else "seg_head_time.txt")
    if not torch.cuda.is_available():
        raise SystemExit("seg_head_time: needs a HIP device")
    if args.weighted:
        return main_weighted(args.out)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = ["fused segmentation loss head vs the torch composition, fp32, %s" % torch.cuda.get_device_name(dev),
             "us per call; %d rounds x %d calls, alternated, HIP events; ratio = torch / fused per round" % (ROUNDS, CALLS)]
    for R, C, what in SIZES:
        g = torch.Generator(device="cpu").manual_seed(R + C)
        act = torch.selu(2.0 * torch.randn(R, C, generator=g)).to(dev)
        lab64 = torch.randint(0, C, (R,), generator=g).to(dev)
        lab32 = lab64.to(torch.int32)
        hd = SegmentationHead(C, device=dev)
        a3, l3 = act.view(1, R, C), lab32.view(1, R)
        fused = lambda: hd.loss(a3, l3, need_pred=True)
        comp = lambda: torch_composition(act, lab64, C)
        # agreement at the timed size (the counters exactly; the loss to fp32 rounding)
        loss, dact, pred = fused()
        ref = comp()
        cnt = hd.counts()
        torch.cuda.synchronize()
        assert torch.equal(pred.view(-1).long(), ref[2]) and int(cnt["correct"]) == int(ref[3])
        assert torch.equal(cnt["seen"], ref[4]) and torch.equal(cnt["correct_class"], ref[5])
        assert torch.equal(cnt["predicted"], ref[6])
        assert abs(float(loss) - float(ref[0])) < 1e-5 and float((dact.view(R, C) - ref[1]).abs().max()) * R < 1e-5
        for _ in range(5):
            fused(), comp()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(fused))
            tc.append(timed(comp))
        # the two kernels alone, from the library's own event brackets
        lib.conv3p_profile_reset()
        lib.conv3p_profile_enable(1)
        for _ in range(CALLS):
            fused()
        torch.cuda.synchronize()
        kern = None
        for k in range(lib.conv3p_profile_kinds()):
            n, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
            lib.conv3p_profile_read(k, ctypes.byref(n), ctypes.byref(ms))
            if n.value and lib.conv3p_profile_name(k).decode() == "seg_head_kernel":
                kern = ms.value / n.value * 1e3
        lib.conv3p_profile_enable(0)
        lib.conv3p_profile_reset()
        traffic = R * (8 * C + 8)
        lines.append("")
        lines.append("R x C = %d x %d  (%s; %.1f MB of traffic at 8 C + 8 bytes per row)" % (R, C, what, traffic / 1e6))
        lines.append("  fused  (2 launches)   " + "  ".join("%8.1f" % v for v in tf))
        lines.append("  torch composition     " + "  ".join("%8.1f" % v for v in tc))
        lines.append("  ratio torch / fused   " + "  ".join("%8.2f" % (c / f) for f, c in zip(tf, tc)))
        if kern is not None:
            lines.append("  seg_head_kernel + finish, event bracket: %.1f us -> %.0f GB/s" % (kern, traffic / kern / 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
