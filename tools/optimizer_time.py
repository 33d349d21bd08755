"""developer: time the momentum optimizer step at the three sizes of DESIGN.md section 5g.

Variants, all in one process, rounds alternated between them, a round of CALLS calls timed with one pair of HIP events:
  (a) the path before optim.py: head.fully_connected_grad + the three torch lines of distributed.sharded_momentum_step
  (b) head.fully_connected_grad + optim.momentum_step (one launch)
  (c) MomentumOptimizer.fused_fc_step (the update in the epilogue of the dW pass; fc1 only)
  (d) for reference: torch.optim.SGD(momentum=0.9) in the installed torch's default (foreach) mode
At fc1's size the variants include the gradient pass (that is what (c) replaces) and the update is also timed alone;
the parameter sets are timed as updates alone.  Output: profiles/optimizer_time.txt (--out).

    python tools/optimizer_time.py [--out profiles/optimizer_time.txt]

--guarded (DESIGN.md section 5g'): the step that clips by the global norm and skips a non-finite batch, same protocol,
same three sizes, output profiles/optimizer_guarded_time.txt:
  (a) the plain optim.momentum_step (one launch)
  (b) MomentumOptimizer.step with clip_norm and skip_nonfinite: grad_sumsq (two launches per 16 tensors), the guarded
      step, the skipped_steps counter; (b') the same without the optimizer object's counter
  (c) what a torch user writes: torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum, nesterov=True), foreach
and fc1's gradient + update as the classification step runs it with and without the guard (fused epilogue against
fully_connected_grad + guarded step).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from pointwise_amd import distributed, head, stack
from pointwise_amd.optim import MomentumOptimizer, grad_sumsq, momentum_step

ROUNDS, CALLS = 5, 20
LR, MOM = 0.001, 0.9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS      # us per call


def race(variants):
    """{name: fn} -> {name: [us per call of every round]}, rounds alternated between the variants."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            out[k].append(timed(fn))
    return out


def report(lines, res, nbytes=None):
    base = statistics.median(res["(a)"]) if "(a)" in res else None
    for k, v in res.items():
        med = statistics.median(v)
        s = "  %-46s %s   median %8.1f  spread %4.1f %%" % (k, " ".join("%8.1f" % x for x in v), med,
                                                           100.0 * (max(v) - min(v)) / med)
        if base is not None and k != "(a)":
            s += "  (a)/this %.2f" % (base / med)
        if nbytes and k in nbytes:
            s += "  %.2f TB/s of %.0f MB" % (nbytes[k] / med / 1e6, nbytes[k] / 1e6)
        lines.append(s)


def torch_lines(params, grads, accs):
    for p, g, a in zip(params, grads, accs):
        distributed.sharded_momentum_step(p, g, a.reshape(-1), LR, MOM)


def update_only(lines, title, params):
    grads = [torch.randn_like(p) for p in params]
    acc_a = [torch.zeros_like(p) for p in params]
    acc_b = [torch.zeros_like(p) for p in params]
    pa, pb, pd = ([p.clone() for p in params] for _ in range(3))
    for p, g in zip(pd, grads):
        p.grad = g
    sgd = torch.optim.SGD(pd, lr=LR, momentum=MOM)
    res = race({"(a)": lambda: torch_lines(pa, grads, acc_a),
                "(b) momentum_step": lambda: momentum_step(pb, grads, acc_b, LR, MOM),
                "(d) torch.optim.SGD": sgd.step})
    n = sum(p.numel() for p in params) * 4
    lines.append("")
    lines.append("%s: %d tensors, %.3f MB (update alone; 5 x that in traffic for one fused pass)" % (title, len(params), n / 1e6))
    report(lines, res, {"(b) momentum_step": 5 * n})


def ratio(lines, res, num, den, what):
    a, b = statistics.median(res[num]), statistics.median(res[den])
    lines.append("  %s: %.1f / %.1f = %.2f" % (what, a, b, a / b))


def guarded_update(lines, title, params):
    """(a) / (b) / (b') / (c) on clones of `params` with one fixed set of gradients; clip_norm = half their norm, so
    the clipping multiplies for real."""
    grads = [torch.randn_like(p) for p in params]
    n = sum(p.numel() for p in params)
    clip = 0.5 * float(n) ** 0.5
    pa, pb, pf, pc = ([p.clone() for p in params] for _ in range(4))
    acc_a, acc_f = ([torch.zeros_like(p) for p in params] for _ in range(2))
    opt = MomentumOptimizer(pb, LR, MOM, clip_norm=clip, skip_nonfinite=True)
    for p, g in zip(pc, grads):
        p.grad = g.clone()                        # clip_grad_norm_ rescales .grad in place: its own copy
    sgd = torch.optim.SGD(pc, lr=LR, momentum=MOM, nesterov=True, foreach=True)

    def vc():
        torch.nn.utils.clip_grad_norm_(pc, clip, foreach=True)
        sgd.step()
    res = race({"(a) momentum_step": lambda: momentum_step(pa, grads, acc_a, LR, MOM),
                "(b) MomentumOptimizer.step, clip + skip": lambda: opt.step(grads),
                "(b') momentum_step, clip + skip": lambda: momentum_step(pf, grads, acc_f, LR, MOM, clip_norm=clip,
                                                                         skip_nonfinite=True),
                "(c) clip_grad_norm_ + SGD(nesterov), foreach": vc,
                "    grad_sumsq alone": lambda: grad_sumsq(grads)})
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 0 and opt.last_grad_norm()[0] > clip
    lines.append("")
    lines.append("%s: %d tensors, %.3f MB (traffic: plain step 5 x that, norm pass 1 x)" % (title, len(params), 4 * n / 1e6))
    report(lines, res, {"(a) momentum_step": 20 * n, "(b') momentum_step, clip + skip": 24 * n, "    grad_sumsq alone": 4 * n})
    ratio(lines, res, "(b) MomentumOptimizer.step, clip + skip", "(a) momentum_step", "(b) / (a)")
    ratio(lines, res, "(b') momentum_step, clip + skip", "(a) momentum_step", "(b') / (a)")
    ratio(lines, res, "(c) clip_grad_norm_ + SGD(nesterov), foreach", "(b) MomentumOptimizer.step, clip + skip", "(c) / (b)")


def guarded(lines, dev):
    M, K, N = 32, 73728, 512
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(dev)
    W0 = (torch.randn(K, N, generator=g) * K ** -0.5).to(dev)
    b0 = torch.zeros(N, device=dev)
    dy = (torch.randn(M, N, generator=g) / M).to(dev)
    y = head.fully_connected(x, W0, b0, selu=True)
    guarded_update(lines, "fc1 %d x %d: the update alone" % (K, N), [W0, b0])
    # fc1's gradient + update as the classification step runs it: fused epilogue (plain optimizer) against
    # fully_connected_grad + guarded step (what ClassificationHead does for an optimizer that is not fusable)
    dW, db = torch.empty_like(W0), torch.empty_like(b0)
    Wf, bf, Wg, bg = W0.clone(), b0.clone(), W0.clone(), b0.clone()
    opt_f = MomentumOptimizer([Wf, bf], LR, MOM)
    grad = lambda W: head.fully_connected_grad(x, W, y, dy, selu=True, dW_out=dW, db_out=db)
    grad(Wg)
    torch.cuda.synchronize()
    clip = 0.5 * float(grad_sumsq([dW, db]).cpu()[0]) ** 0.5
    opt_g = MomentumOptimizer([Wg, bg], LR, MOM, clip_norm=clip, skip_nonfinite=True)

    def vg():
        grad(Wg)
        opt_g.step([dW, db])
    res = race({"fused_fc_step (plain optimizer)": lambda: opt_f.fused_fc_step(x, Wf, bf, y, dy, selu=True),
                "fully_connected_grad + guarded step": vg,
                "    fully_connected_grad alone": lambda: grad(Wg)})
    lines.append("")
    lines.append("fc1 %d x %d, M = %d: gradient pass + update, without and with the guard" % (K, N, M))
    report(lines, res)
    ratio(lines, res, "fully_connected_grad + guarded step", "fused_fc_step (plain optimizer)", "guarded / fused")
    del Wf, Wg, opt_f, opt_g, dW, W0, x
    torch.cuda.empty_cache()
    st = stack.Conv3pStack(3, None, device=dev)
    hd = head.ClassificationHead(2048, num_class=40, device=dev)
    guarded_update(lines, "classification model, all parameters", list(st.filters) + hd.parameters())
    guarded_update(lines, "cfg2 stack's filters alone (launch latency)", list(st.filters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guarded", action="store_true", help="time the clipping / skipping step (section 5g')")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                "optimizer_guarded_time.txt" if args.guarded else "optimizer_time.txt")
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_time: needs a HIP device")
    dev = torch.device("cuda:0")
    if args.guarded:
        lines = ["guarded momentum optimizer step (clip_norm + skip_nonfinite), fp32, %s" % torch.cuda.get_device_name(dev),
                 "us per call incl. Python; %d rounds x %d calls, alternated, HIP events; spread = (max - min) / median of a "
                 "variant's rounds" % (ROUNDS, CALLS)]
        guarded(lines, dev)
        text = "\n".join(lines) + "\n"
        print(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
    lines = ["momentum optimizer step, fp32, %s" % torch.cuda.get_device_name(dev),
             "us per call; %d rounds x %d calls, alternated, HIP events; spread = (max - min) / median of a variant's rounds"
             % (ROUNDS, CALLS)]
    # ---- fc1 of the model: 73 728 x 512, M = 32, with its gradient pass
    M, K, N = 32, 73728, 512
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(dev)
    W0 = (torch.randn(K, N, generator=g) * K ** -0.5).to(dev)
    b0 = torch.zeros(N, device=dev)
    dy = (torch.randn(M, N, generator=g) / M).to(dev)
    y = head.fully_connected(x, W0, b0, selu=True)
    dW, db = torch.empty_like(W0), torch.empty_like(b0)
    Wa, ba, Wb, bb, Wc, bc, Wd, bd = (t.clone() for _ in range(4) for t in (W0, b0))
    acc_a = [torch.zeros_like(W0), torch.zeros_like(b0)]
    acc_b = [torch.zeros_like(W0), torch.zeros_like(b0)]
    opt_c = MomentumOptimizer([Wc, bc], LR, MOM)
    Wd.grad, bd.grad = dW, db
    sgd = torch.optim.SGD([Wd, bd], lr=LR, momentum=MOM)
    grad = lambda W: head.fully_connected_grad(x, W, y, dy, selu=True, dW_out=dW, db_out=db)

    def va():
        grad(Wa)
        torch_lines([Wa, ba], [dW, db], acc_a)

    def vb():
        grad(Wb)
        momentum_step([Wb, bb], [dW, db], acc_b, LR, MOM)

    def vd():
        grad(Wd)
        sgd.step()
    # (b) and (c) agree bit for bit from the same state before anything is timed
    vb()
    opt_c.fused_fc_step(x, Wc, bc, y, dy, selu=True)
    torch.cuda.synchronize()
    assert torch.equal(Wb, Wc) and torch.equal(bb, bc) and torch.equal(acc_b[0], opt_c.accums[0])
    res = race({"(a)": va, "(b) fully_connected_grad + momentum_step": vb,
                "(c) fused_fc_step": lambda: opt_c.fused_fc_step(x, Wc, bc, y, dy, selu=True),
                "(d) fully_connected_grad + torch.optim.SGD": vd,
                "    fully_connected_grad alone": lambda: grad(Wa)})
    wb = K * N * 4
    lines.append("")
    lines.append("fc1 %d x %d, M = %d: gradient pass + update (W = %.0f MB; bytes: dx 1 W, dW 1 W, fused update 5 W | dW+update 4 W)"
                 % (K, N, M, wb / 1e6))
    report(lines, res, {"(b) fully_connected_grad + momentum_step": 7 * wb, "(c) fused_fc_step": 5 * wb})
    res = race({"(a)": lambda: torch_lines([Wa, ba], [dW, db], acc_a),
                "(b) momentum_step": lambda: momentum_step([Wb, bb], [dW, db], acc_b, LR, MOM),
                "(d) torch.optim.SGD": sgd.step})
    lines.append("")
    lines.append("fc1 %d x %d: the update alone" % (K, N))
    report(lines, res, {"(b) momentum_step": 5 * wb})
    del Wa, Wb, Wc, Wd, acc_a, acc_b, opt_c, sgd, dW
    torch.cuda.empty_cache()
    # ---- the whole classification parameter set, and the cfg2 stack's filters alone
    st = stack.Conv3pStack(3, None, device=dev)
    hd = head.ClassificationHead(2048, num_class=40, device=dev)
    update_only(lines, "classification model, all parameters", list(st.filters) + hd.parameters())
    update_only(lines, "cfg2 stack's filters alone (launch latency)", list(st.filters))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
