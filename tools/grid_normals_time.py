"""developer: time the per-voxel normals (grid.GridSubsample.normals: conv3p_grid_normals_f32, one launch behind a 16-byte
memset) against (a) the composition a caller writes in torch today and (b) the neighbors() launch on the same voxels, the
cheapest call that touches the same table, on the same device:

    u = neigh (M, 27);  q = xyz[u.clamp_min(0)] - xyz[:, None]        (M, 27, 3)
    ok = u >= 0;  n = ok.sum(1);  m = (q * ok).sum(1) / n;  e = (q - m[:, None]) * ok
    C = e^T e / n                                                     (M, 3, 3)
    lam, vec = torch.linalg.eigh(C);  normal = vec[:, :, 0], turned towards the viewpoint;  curvature = lam0 / lam.sum

The composition is GIVEN this call's own neighbour table, which favours it; it materialises (M, 27, 3) tensors, the
order of its sums is not defined, and it has no flags.  If the batched eigh fails on the device the tool says so and times
the moments alone.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube whose side leaves about 4 and about 40 rows a voxel; K = 6,
voxel 0.05.  All sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one
pair of HIP events around back-to-back calls; every shape is warmed up first.  The spread of the rounds is printed next
to their median.  Per shape the kernel's achieved bytes/s against its own traffic floor: 108 B of the table, 12 B of the
voxel's own row (every row is somebody's neighbour: the 27 gathers hit the cache) and 24 B out a voxel, plus 36 B with
the moments.  The kernel's registers, spills and private segment are printed first.  Output: profiles/grid_normals_time.txt.

    python tools/grid_normals_time.py [--out profiles/grid_normals_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, build, grid

ROWS = (65536, 1048576, 1 << 24)
PER_VOXEL = (4, 40)
K, VOXEL = 6, 0.05
ROUNDS = 5


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def alternated(fns, calls):
    """-> per fn the rounds' us per call; two warm-up calls each first.  The last fn, the composition, takes a third
    of the calls a round (it is an order of magnitude slower)."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(ROUNDS):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, calls if k + 1 < len(fns) else max(1, calls // 3)))
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / float(np.median(v))


def show(name, v, extra=""):
    return "  %-46s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%%s" % (
        float(np.median(v)), spread(v), extra)


def rate(M, with_moments, v):
    b = 108 + 12 + 24 + (36 if with_moments else 0)
    return "   %6.0f GB/s of the floor's %d B a voxel" % (M * b / (float(np.median(v)) * 1e-6) / 1e9, b)


def verdict(ours, other, what):
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    word = "SLOWER than" if mo > mc * (1.0 + slack) else "faster than" if mc > mo * (1.0 + slack) else "within the spread of"
    return "%s %s (ratio %s / call %.2f)" % (word, what, what, mc / mo)


def make_cloud(N, per_voxel, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * (N / float(per_voxel)) ** (1.0 / 3.0)
    data = torch.rand((N, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    return data.contiguous(), side


def torch_moments(xyz, neigh, chunk=1 << 20):
    """-> n (M), C (M, 3, 3), in chunks of voxels."""
    ns, Cs = [], []
    for a in range(0, xyz.shape[0], chunk):
        u = neigh[a:a + chunk].long()
        ok = (u >= 0).to(torch.float32)[:, :, None]
        q = (xyz[u.clamp_min(0)] - xyz[a:a + chunk, None, :]) * ok
        n = ok.sum(1).clamp_min(1.0)
        e = (q - q.sum(1, keepdim=True) / n[:, None]) * ok
        ns.append(n[:, 0])
        Cs.append(e.transpose(1, 2) @ e / n[:, None])
    return torch.cat(ns), torch.cat(Cs)


def torch_composition(xyz, neigh, viewpoint, with_eigh=True):
    n, C = torch_moments(xyz, neigh)
    if not with_eigh:
        return n, C
    lam, vec = torch.linalg.eigh(C)
    nrm = vec[:, :, 0]
    s = ((viewpoint - xyz) * nrm).sum(1, keepdim=True)
    return torch.where(s < 0, -nrm, nrm), lam[:, 0] / lam.sum(1).clamp_min(1e-30)


def measure(lines, title, g, calls):
    dev = g.data.device
    M = g.num_voxels()
    g = g.trim()
    xyz = g.data[:, :3].contiguous()
    neigh = g.neighbors()
    vp = torch.tensor([[0.5, 0.5, 100.0]], dtype=torch.float32, device=dev)
    out, out_m = grid.GridNormals(M, False, dev), grid.GridNormals(M, True, dev)

    def table():
        g._neigh = None
        g.neighbors()

    ours = g.normals(viewpoint=vp, out=out)
    st = ours.stats.tolist()
    eigh_ok, why = True, ""
    try:
        theirs, _ = torch_composition(xyz, neigh, vp)
        torch.cuda.synchronize()
        good = ours.flags == 0
        agree = float(((ours.normals[good] * theirs[good]).sum(1).abs() > 0.999).float().mean())
    except Exception as e:                               # the batched eigh is unusable here: the moments alone
        eigh_ok, why, agree = False, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:120]), float("nan")
    t = alternated((table,
                    lambda: g.normals(viewpoint=vp, out=out),
                    lambda: g.normals(viewpoint=vp, return_moments=True, out=out_m),
                    lambda: g.normals(out=out),
                    lambda: torch_composition(xyz, neigh, vp, eigh_ok)), calls)
    lines.append("")
    lines.append("%s: %d voxels, %.1f of 27 neighbours a voxel; normal_stats %s; |cos| > 0.999 against the composition's "
                 "normal on %.4f of the flags-0 voxels" % (title, M, float((neigh >= 0).sum()) / max(M, 1), st, agree))
    lines.append("  %d calls a round" % calls)
    if not eigh_ok:
        lines.append("  torch.linalg.eigh on (M, 3, 3) is unusable here (%s): the composition below is the moments alone" % why)
    lines.append(show("neighbors (the table alone, 1 launch)", t[0]))
    lines.append(show("normals, one viewpoint", t[1], rate(M, False, t[1])))
    lines.append(show("normals, one viewpoint, with the moments", t[2], rate(M, True, t[2])))
    lines.append(show("normals, no viewpoint", t[3], rate(M, False, t[3])))
    lines.append(show("torch composition" + ("" if eigh_ok else " (moments alone)"), t[4]))
    lines.append("  normals is %s" % verdict(t[1], t[4], "the composition"))
    lines.append("  normals costs %.2f x neighbors (%.1f us more a call)" % (
        float(np.median(t[1])) / float(np.median(t[0])), float(np.median(t[1])) - float(np.median(t[0]))))
    print("\n".join(lines[-11:]), flush=True)            # as it goes: a long run is seen to move


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_normals_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_normals_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["per-voxel normals against gather + masked moments + batched eigh in torch and against neighbors(), %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes" % (ROUNDS, K, VOXEL),
             "the composition is given the call's own neighbour table and works in chunks of 2^20 voxels"]
    if args.note:
        lines.insert(2, args.note)
    for name, v, vs, ss, scr in build.kernel_resources():
        if "grid_normals_kernel" in name:
            lines.append("grid_normals_kernel: vgprs %d, vgpr spills %d, sgpr spills %d (to vector registers), private segment %d B"
                         % (v, vs, ss, scr))
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 3
        for per_voxel in PER_VOXEL:
            data, side = make_cloud(N, per_voxel, 7000 + per_voxel, dev)
            g = grid.grid_subsample(data, None, VOXEL, "mean")
            del data
            measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), g, calls)
            del g
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
