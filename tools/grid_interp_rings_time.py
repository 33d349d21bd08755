"""developer: time the ring fallback of the interpolated projection (grid.GridSubsample.interpolate(rings=):
conv3p_grid_interpolate_rings_f32 -- the plain call's launch, a list kernel and, with rings > 1, the ring kernel on a
fixed grid) against the plain call of the same build and against what a caller writes in torch for the rows the plain
call leaves at -1, on the same device:

    d = torch.cdist(p_leftover, q_voted)              (rows, voted voxels), in chunks of rows of at most 2^28 distances
    d2k, j = (d * d).topk(k, largest=False);  u = voted[j]
    w = 1 / d2k.clamp_min(1e-10);  out = (w[..., None] * scores[u]).sum(1) / w.sum(1, keepdim=True);  label = out.argmax(1)

That baseline is a TRUE k-NN over all voted voxels: more work than the ring search, which stops at the first ring with a
candidate and never looks past `rings` cells, and another result (it labels every row, from the nearest voxels wherever
they are).  It is timed on the first 65 536 leftover rows at most and given per leftover row, next to the ring search's
cost per leftover row, (the rings call - the plain call) / leftover rows: its chunks are independent, so its time is
proportional to the rows.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube with about 4 rows a voxel; K = 6, voxel 0.05, C = 13, k = 3,
labels only.  (a) every voxel voted: rings = 8 against the plain call -- the price of the list kernel and an idle ring
launch.  (b) a random 50 %, 10 % and 1 % of the voxels voted: the plain call, rings = 4 and rings = 8, alternated, with
the rows labelled per ring.  us per call INCLUDING Python, 5 rounds, a round timed with one pair of HIP events around
back-to-back calls, every shape warmed up first; the spread of the rounds next to their median.  Output:
profiles/grid_interp_rings_time.txt.

    python tools/grid_interp_rings_time.py [--out profiles/grid_interp_rings_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, grid

ROWS = (65536, 1048576, 1 << 24)
SHARES = (0.5, 0.1, 0.01)
K, VOXEL, NCLS, KNN = 6, 0.05, 13, 3
ROUNDS = 5
BASELINE_ROWS = 65536
BASELINE_DISTANCES = 1 << 28


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def alternated(fns, calls, rounds=ROUNDS, warm=2):
    """-> per fn the rounds' us per call; warm-up calls each first."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, calls))
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / float(np.median(v))


def show(name, v, extra=""):
    return "  %-46s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%%s" % (
        float(np.median(v)), spread(v), extra)


def make_cloud(N, per_voxel, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * (N / float(per_voxel)) ** (1.0 / 3.0)
    data = torch.rand((N, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    return data.contiguous(), side


def torch_knn(p, q, voted, scores):
    """The baseline on the rows p (n, 3) against the voted voxels' representatives q (v, 3) -> labels (n) int64."""
    out = []
    k = min(KNN, q.shape[0])
    chunk = max(1, BASELINE_DISTANCES // max(1, q.shape[0]))
    for a in range(0, p.shape[0], chunk):
        d = torch.cdist(p[a:a + chunk], q)
        d2k, j = (d * d).topk(k, dim=1, largest=False)
        u = voted[j]
        w = 1.0 / d2k.clamp_min(1e-10)
        out.append(((w[:, :, None] * scores[u]).sum(1) / w.sum(1, keepdim=True)).argmax(1))
    return torch.cat(out)


def measure(lines, title, data, g, calls):
    dev = data.device
    N = data.shape[0]
    V = g.num_voxels()
    g = g.trim()
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    scores = torch.rand((V, NCLS), generator=gen, device=dev, dtype=torch.float32)
    lab = torch.empty((N,), dtype=torch.int32, device=dev)
    g.neighbors()
    lines.append("")
    lines.append("%s: %d voxels (%.1f rows a voxel); %d calls a round" % (title, V, N / float(max(V, 1)), calls))
    # (a) every voxel voted: no row enters the fallback
    t = alternated((lambda: g.interpolate(data, scores, k=KNN, out=lab),
                    lambda: g.interpolate(data, scores, k=KNN, rings=8, out=lab)), calls)
    assert int(g.ring_stats[0]) == 0
    more = float(np.median(t[1])) - float(np.median(t[0]))
    lines.append(" (a) every voxel voted")
    lines.append(show("interpolate, the plain call", t[0]))
    lines.append(show("interpolate rings = 8 (nothing to search)", t[1]))
    lines.append("  the list kernel and an idle ring launch cost %.1f us a call, %.2f x the plain call's own time" % (
        more, more / float(np.median(t[0]))))
    # (b) a share of the voxels voted
    for share in SHARES:
        valid = torch.where(torch.rand((V,), generator=gen, device=dev) < share, 1, -1).to(torch.int32)
        counts = {}

        def ringed(r):
            def fn():
                g.interpolate(data, scores, k=KNN, valid_labels=valid, rings=r, out=lab)
            return fn

        t = alternated((lambda: g.interpolate(data, scores, k=KNN, valid_labels=valid, out=lab), ringed(4), ringed(8)), calls)
        for r in (4, 8):
            ringed(r)()
            counts[r] = (g.interp_stats.tolist(), g.ring_stats.tolist())
        plain = g.interpolate(data, scores, k=KNN, valid_labels=valid)
        left = torch.nonzero((plain < 0) & (g.inverse >= 0))[:, 0]
        L = int(left.numel())
        lines.append(" (b) %g %% of the voxels voted (%d of %d); %d of %d rows enter the fallback" % (
            100 * share, int((valid >= 0).sum()), V, L, N))
        lines.append(show("interpolate, the plain call", t[0]))
        for n, r in ((1, 4), (2, 8)):
            st, rs = counts[r]
            lines.append(show("interpolate rings = %d" % r, t[n]))
            lines.append("      rows labelled per ring 1 .. 8: %s; left at -1: %d" % (rs[1:], st[2]))
        if L == 0:
            lines.append("  no row is left over: no baseline")
            continue
        voted = torch.nonzero(valid >= 0)[:, 0]
        rows = left[:BASELINE_ROWS]
        p, q = data[rows, :3].contiguous(), g.data[voted, :3].contiguous()
        big = q.shape[0] * rows.numel() > (1 << 34)
        tb = alternated((lambda: torch_knn(p, q, voted, scores),), 1, rounds=2 if big else ROUNDS, warm=1)[0]
        lines.append(show("torch cdist + topk + gather-sum, %d rows" % rows.numel(), tb))
        base = float(np.median(tb)) / rows.numel()
        for n, r in ((1, 4), (2, 8)):
            ours = (float(np.median(t[n])) - float(np.median(t[0]))) / L
            lines.append("  per leftover row: rings = %d %.4f us (rings call - plain call), the baseline %.4f us: ratio %.1f "
                         "(the baseline is a true k-NN over all %d voted voxels: more work, and it labels every row)" % (
                             r, ours, base, base / ours if ours > 0 else float("nan"), q.shape[0]))
        del p, q, rows, left, voted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "grid_interp_rings_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_interp_rings_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["ring fallback of the interpolated projection against the plain call and against cdist + topk in torch, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g, C = %d, k = %d, labels only; "
             "uniform cubes" % (ROUNDS, K, VOXEL, NCLS, KNN),
             "the baseline is timed on at most %d leftover rows, in chunks of at most 2^28 distances" % BASELINE_ROWS]
    if args.note:
        lines.insert(2, args.note)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 2
        data, side = make_cloud(N, 4, 6004, dev)
        g = grid.grid_subsample(data, None, VOXEL, "mean")
        measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), data, g, calls)
        del data, g
        torch.cuda.empty_cache()
        with open(args.out + ".part", "w") as f:         # what is measured so far survives a later shape that does not
            f.write("\n".join(lines) + "\n")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    os.remove(args.out + ".part")


if __name__ == "__main__":
    main()
