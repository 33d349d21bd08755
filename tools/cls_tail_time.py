"""developer: time the classification model's fused tail (head.classification_tail with the W2 / b2 update:
conv3p_cls_tail_step_f32, two launches) against the composition it replaces -- the lines of
ClassificationHead.forward's tail (dropout_selu with torch's generator, fc2), loss(), the statistics a training loop
adds (argmax, compare, three bincounts), backward()'s tail (fc2's gradient, dropout backward) and momentum_step on
W2 / b2 -- at M x H x C = 32 x 512 x 40 (the model), 128 x 512 x 40 and 32 x 512 x 10.

The fc kernels need num_class % 8 == 0, so the composition does not exist for 10 classes; there it is timed on W2 / b2
padded to 16 columns (what a user would have had to do), and the line says so.

Both in one process, alternated: 5 rounds x 20 calls each, us per call INCLUDING Python, a round timed with one pair
of HIP events; every shape is warmed up first; nothing synchronises inside a round.  Then the C entry point alone,
200 back-to-back calls between one event pair: the device time of the two kernels (or the host's enqueue time, should
that be the longer).  Last, the largest distances to the float64 restatement over the sizes of tests/test_cls_tail.py,
for the fused call and for the composition.  Output: profiles/cls_tail_time.txt (--out).

    python tools/cls_tail_time.py [--out profiles/cls_tail_time.txt]
"""
import argparse
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, head, optim

SIZES = ((32, 512, 40, "the model: 32 clouds per GPU, ModelNet40"), (128, 512, 40, "the largest batch of the fc kernels"),
         (32, 512, 10, "ModelNet10"))
ROUNDS, CALLS, BARE = 5, 20, 200
RATE, LR, MOM = 0.5, 0.001, 0.9


def composition(fc1, W2, b2, labels, accums, C, keep_mask=None):
    """What the parent does between fc1's output and fc1's backward.  labels int64."""
    M = fc1.shape[0]
    drop, mask = head.dropout_selu(fc1, RATE, True, keep_mask)                      # forward(): :73
    fc2 = head.fully_connected(drop, W2, b2, selu=True)                            # :75
    logp = torch.log_softmax(fc2, dim=1)                                           # loss()
    idx = labels.unsqueeze(1)
    e = -(logp.gather(1, idx)).mean()
    dlogits = torch.softmax(fc2, dim=1)
    dlogits.scatter_add_(1, idx, -torch.ones_like(idx, dtype=dlogits.dtype))
    dlogits = dlogits / float(M)
    pred = torch.argmax(fc2[:, :C], dim=1)                                         # train_modelnet40_acsd.py:136-146
    hit = pred == labels
    stats = (hit.sum(), torch.bincount(labels, minlength=C), torch.bincount(labels[hit], minlength=C),
             torch.bincount(pred, minlength=C))
    ddrop, dW2, db2 = head.fully_connected_grad(drop, W2, fc2, dlogits, selu=True)  # backward()
    a, _, _ = head.dropout_selu_constants(RATE)
    dfc1 = ddrop * (a * mask)
    optim.momentum_step([W2, b2], [dW2, db2], accums, LR, MOM)
    return e, dfc1, pred, stats, fc2


def timed(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def rel(got, want):
    want = np.asarray(want)
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))


def accuracy(dev):
    """Largest rel distance to float64 over the sizes of tests/test_cls_tail.py (explicit mask, rate 0.5)."""
    from tests.cls_tail_ref import cls_tail_ref
    t = lambda a: torch.from_numpy(a).to(dev)
    worst = {"fused": {}, "composition (C % 8 == 0)": {}}
    for M, H, C in itertools.product((1, 3, 32, 33, 128), (8, 512, 1024), (2, 10, 13, 40, 128)):
        rng = np.random.default_rng(1000 * M + H + C)
        fc1 = rng.standard_normal((M, H)).astype(np.float32)
        W2 = (rng.standard_normal((H, C)) / np.sqrt(H)).astype(np.float32)
        b2 = (rng.standard_normal(C) * 0.1).astype(np.float32)
        labels = rng.integers(0, C, size=M)
        mask = (rng.random((M, H)) < 0.5).astype(np.float32)
        ref = cls_tail_ref(fc1, W2, b2, labels, RATE, mask)
        out = head.classification_tail(t(fc1), t(W2), t(b2), t(labels), rate=RATE, keep_mask=t(mask))
        got = {"fused": {"logits": out["logits"], "loss": out["loss_sum"] / M, "dfc1": out["dfc1"], "dW2": out["dW2"],
                         "db2": out["db2"]}}
        if C % 8 == 0:
            W, b = t(W2), t(b2)
            e, dfc1, _, _, fc2 = composition(t(fc1), W, b, t(labels), [torch.zeros_like(W), torch.zeros_like(b)], C, t(mask))
            got["composition (C % 8 == 0)"] = {"logits": fc2, "loss": e, "dfc1": dfc1}
        ref["loss"] = ref["loss_sum"] / M
        for arm, outs in got.items():
            for k, v in outs.items():
                worst[arm][k] = max(worst[arm].get(k, 0.0), rel(v, ref[k]))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "cls_tail_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_tail_time: needs a HIP device")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = ["fused classification tail (with the W2 / b2 update) vs the composition it replaces, fp32, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds x %d calls, alternated, HIP events; ratio = composition / fused per round"
             % (ROUNDS, CALLS)]
    for M, H, C, what in SIZES:
        g = torch.Generator(device="cpu").manual_seed(M + H + C)
        fc1 = torch.selu(torch.randn(M, H, generator=g)).to(dev)
        W2 = (torch.randn(H, C, generator=g) / H ** 0.5).to(dev)
        b2 = torch.zeros(C, device=dev)
        lab64 = torch.randint(0, C, (M,), generator=g).to(dev)
        lab32 = lab64.to(torch.int32)
        Cp = (C + 7) // 8 * 8                      # the fc kernels' N % 8 == 0
        Wc = torch.zeros(H, Cp, device=dev)
        Wc[:, :C] = W2
        bc = torch.zeros(Cp, device=dev)           # (the padded classes take part in the softmax: this arm is timed only)
        acc_c = [torch.zeros_like(Wc), torch.zeros_like(bc)]
        Wf, bf = W2.clone(), b2.clone()
        acc_f = [torch.zeros_like(Wf), torch.zeros_like(bf)]
        step = [0]

        def fused():
            step[0] += 1
            return head.classification_tail(fc1, Wf, bf, lab32, rate=RATE, seed=1, step=step[0], accum_W2=acc_f[0],
                                            accum_b2=acc_f[1], lr=LR, momentum=MOM)
        comp = lambda: composition(fc1, Wc, bc, lab64, acc_c, C)
        for _ in range(5):
            fused(), comp()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(fused))
            tc.append(timed(comp))
        # the C entry point alone
        logits = torch.empty(M, C, device=dev)
        pred = torch.empty(M, dtype=torch.int32, device=dev)
        dfc1 = torch.empty(M, H, device=dev)
        loss = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(2 + 3 * C, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.conv3p_cls_tail_workspace_bytes(M, H, C), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        a = (fc1.data_ptr(), Wf.data_ptr(), bf.data_ptr(), lab32.data_ptr(), M, H, C, 1, RATE, None, 1, 7, 1.0 / M,
             logits.data_ptr(), pred.data_ptr(), dfc1.data_ptr(), acc_f[0].data_ptr(), acc_f[1].data_ptr(), LR, MOM, None,
             loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)

        def bare():
            if lib.conv3p_cls_tail_step_f32(*a) != _lib.OK:
                raise SystemExit("cls_tail_time: conv3p_cls_tail_step_f32 failed")
        bare()
        torch.cuda.synchronize()
        tb = [timed(bare, BARE) for _ in range(3)]
        lines.append("")
        lines.append("M x H x C = %d x %d x %d  (%s)" % (M, H, C, what))
        lines.append("  fused  (2 launches)        " + "  ".join("%8.1f" % v for v in tf))
        lines.append("  composition%s " % (" (C -> %d) " % Cp if Cp != C else "           ") + "  ".join("%8.1f" % v for v in tc))
        lines.append("  ratio composition / fused  " + "  ".join("%8.2f" % (c / f) for f, c in zip(tf, tc)))
        lines.append("  the C call alone, %d back to back, 3 rounds: " % BARE + "  ".join("%.1f" % v for v in tb) + " us")
    lines.append("")
    lines.append("largest max|delta| / max(1, max|ref|) against float64 over M in {1, 3, 32, 33, 128}, H in {8, 512, 1024},")
    lines.append("C in {2, 10, 13, 40, 128}, explicit mask, rate 0.5:")
    for arm, w in accuracy(dev).items():
        lines.append("  %-26s " % arm + "  ".join("%s %.2e" % kv for kv in sorted(w.items())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
