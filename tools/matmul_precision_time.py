"""Forward and backward time of the cfg5 shard (B=16, N=8192, 128 -> 256) in each matmul precision of the matrix-core
path (NeighborCache(matmul_precision=...): "highest", "medium"), the per-kernel times from the library's profile, and
each mode's deviation from "highest" on y, dX and dW.

    python tools/matmul_precision_time.py [--calls 10] [--rounds 3] [--out FILE]

Every mode is warmed up first; then `rounds` rounds alternate highest / medium, each timing `calls` forward calls
and `calls` backward calls (device-synchronised means).  The reported time of a mode is the median over the rounds."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pointwise_amd import _lib, conv3p_op as op, synth  # noqa: E402

MODES = ("highest", "medium")


def kinds(lib):
    out = {}
    for k in range(lib.conv3p_profile_kinds()):
        n, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
        lib.conv3p_profile_read(k, ctypes.byref(n), ctypes.byref(ms))
        if n.value:
            out[lib.conv3p_profile_name(k).decode()] = {"calls": n.value, "ms_per_call": round(ms.value / n.value, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, N, ci, co, s, vox = 16, 8192, 128, 256, (1, 1, 1), 0.1
    t = lambda x: torch.from_numpy(x).to(dev)
    P = synth.room_like(B, N, 7, extent=(2.4, 2.4, 3.0))
    tp, tx = t(P), t(synth.features(B, N, ci, 8, points=P))
    tw, tdy = t(synth.filter_weights(3, 3, 3, ci, co, 5)), t(synth.upstream_grad(B, N, co, 9))
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    fwd = lambda: op.conv3p(tp, tx, tw, s, vox, cache=cache)
    bwd = lambda: op.conv3p_grad(tdy, tp, tx, tw, s, vox, cache=cache)

    outs = {}
    for mode in MODES:                                   # warm-up, and the outputs the deviations are taken from
        cache.matmul_precision = mode
        for _ in range(2):
            y = fwd()
            dx, dw = bwd()
        torch.cuda.synchronize()
        outs[mode] = (y.double(), dx.double(), dw.double())

    times = {m: {"forward": [], "backward": []} for m in MODES}
    for _ in range(a.rounds):
        for mode in MODES:
            cache.matmul_precision = mode
            for name, fn in (("forward", fwd), ("backward", bwd)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                times[mode][name].append((time.perf_counter() - t0) / a.calls * 1e3)

    prof = {}
    for mode in MODES:                                   # per-kernel times in a separate, profiled pass
        cache.matmul_precision = mode
        prof[mode] = {}
        for name, fn in (("forward", fwd), ("backward", bwd)):
            lib.conv3p_profile_reset()
            lib.conv3p_profile_enable(1)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            lib.conv3p_profile_enable(0)
            prof[mode][name] = kinds(lib)
            lib.conv3p_profile_reset()

    res = {"shape": {"B": B, "N": N, "Cin": ci, "Cout": co, "calls": a.calls, "rounds": a.rounds},
           "device": torch.cuda.get_device_name(0), "modes": {}}
    base = None
    for mode in MODES:
        f, b = float(np.median(times[mode]["forward"])), float(np.median(times[mode]["backward"]))
        if mode == "highest":
            base = f + b
        dev_ = {}
        for name, u, v in zip(("y", "dX", "dW"), outs[mode], outs["highest"]):
            d = (u - v)
            dev_[name] = {"max_abs": float(d.abs().max()), "fro_rel": float(d.norm() / v.norm())}
        res["modes"][mode] = {"forward_ms": round(f, 4), "backward_ms": round(b, 4), "fwd_bwd_ms": round(f + b, 4),
                              "vs_highest": round((f + b) / base, 4), "rounds_ms": times[mode],
                              "deviation_from_highest": dev_, "kernels": prof[mode]}
    for mode in MODES:
        m = res["modes"][mode]
        print("%-8s fwd %.3f ms  bwd %.3f ms  fwd+bwd %.3f ms  (%.3fx highest)  dev y %.2e/%.2e dX %.2e/%.2e dW %.2e/%.2e" % (
            mode, m["forward_ms"], m["backward_ms"], m["fwd_bwd_ms"], m["vs_highest"],
            *[m["deviation_from_highest"][k][q] for k in ("y", "dX", "dW") for q in ("max_abs", "fro_rel")]))
        for name in ("forward", "backward"):
            print("    %s kernels: %s" % (name, {k: v["ms_per_call"] for k, v in m["kernels"][name].items()}))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
