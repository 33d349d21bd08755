"""developer: time the fused segmentation loss head (SegmentationHead.loss with predictions) against the torch
composition a user would write without it -- the op list of ClassificationHead.loss (log_softmax, gather, mean,
softmax, scatter_add, scale) plus argmax, compare and three bincounts -- at the three sizes of DESIGN.md section 5f.

Both in one process, alternated: 3 rounds x 20 calls each, a round timed with one pair of HIP events; every shape is
warmed up first.  Neither side synchronises inside a round.  Output: profiles/seg_head_time.txt (--out).

    python tools/seg_head_time.py [--out profiles/seg_head_time.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "seg_head_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_head_time: needs a HIP device")
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
