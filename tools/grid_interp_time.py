"""developer: time the interpolated projection (grid.GridSubsample.neighbors / interpolate: conv3p_grid_neighbors, one
launch; conv3p_grid_interpolate_f32, one launch) against project(scores.labels()) and against the composition a caller
writes in torch today, on the same device:

    q = voxel_data[neigh[inverse]]                    (N, 27, 3)     the 27 representatives around every row
    d2 = ((p - q) ** 2).sum(-1), inf where there is no voxel
    d2k, j = d2.topk(k, largest=False);  u = neigh[inverse].gather(1, j)
    w = 1 / d2k.clamp_min(1e-10);  out = (w[..., None] * scores[u]).sum(1) / w.sum(1, keepdim=True);  label = out.argmax(1)

The composition is GIVEN this call's own neighbour table, which favours it (torch has no such structure), it
materialises (N, 27, 3) and (N, k, C) tensors, and neither its selection on ties nor the order of its sums is defined.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube whose side leaves about 4 and about 40 rows a voxel; K = 6,
voxel 0.05, C = 13; and the many-clouds result of 64 rooms x 65 536 rows.  All sides in one process, alternated over 5
rounds, us per call INCLUDING Python, a round timed with one pair of HIP events around back-to-back calls; every shape is
warmed up first.  The spread of the rounds is printed next to their median.  Per shape the row kernel's achieved bytes/s
against its own traffic floor, 4K + 4 + 108 + k(12 + 4C) + 4 bytes a row, plus 4C with scores.  Output:
profiles/grid_interp_time.txt.

    python tools/grid_interp_time.py [--out profiles/grid_interp_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, grid

ROWS = (65536, 1048576, 1 << 24)
PER_VOXEL = (4, 40)
K, VOXEL, NCLS = 6, 0.05, 13
ROOMS, ROOM_ROWS = 64, 65536
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
    """-> per fn the rounds' us per call; two warm-up calls each first."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(ROUNDS):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, calls))
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / float(np.median(v))


def show(name, v, extra=""):
    return "  %-46s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%%s" % (
        float(np.median(v)), spread(v), extra)


def floor_bytes(N, k, with_scores):
    return N * (4 * K + 4 + 108 + k * (12 + 4 * NCLS) + 4 + (4 * NCLS if with_scores else 0))


def rate(N, k, with_scores, v):
    return "   %6.0f GB/s of the floor's %d B a row" % (floor_bytes(N, k, with_scores) / (float(np.median(v)) * 1e-6) / 1e9,
                                                          floor_bytes(1, k, with_scores))


def verdict(ours, other, what):
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    word = "SLOWER than" if mo > mc * (1.0 + slack) else "faster than" if mc > mo * (1.0 + slack) else "within the spread of"
    return "%s %s (ratio %s / call %.2f)" % (word, what, what, mc / mo)


def make_cloud(N, per_voxel, seed, dev, rows_of_a_cube=None):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * ((rows_of_a_cube or N) / float(per_voxel)) ** (1.0 / 3.0)
    data = torch.rand((N, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    return data.contiguous(), side


def torch_composition(data, g, neigh, scores, k, chunk=1 << 21):
    """The composition in chunks of rows (the (N, 27, 3) gather of 2^24 rows alone is 5.4 GB) -> labels (N) int64."""
    out = []
    for a in range(0, data.shape[0], chunk):
        p, inv = data[a:a + chunk, :3], g.inverse[a:a + chunk].long().clamp_min(0)
        nb = neigh[inv].long()                                         # (n, 27)
        q = g.data[nb.clamp_min(0)][:, :, :3]                          # (n, 27, 3)
        d2 = ((p[:, None, :] - q) ** 2).sum(-1)
        d2 = torch.where(nb >= 0, d2, torch.full_like(d2, float("inf")))
        d2k, j = d2.topk(k, dim=1, largest=False)
        u = nb.gather(1, j).clamp_min(0)
        w = torch.where(torch.isfinite(d2k), 1.0 / d2k.clamp_min(1e-10), torch.zeros_like(d2k))
        blend = (w[:, :, None] * scores[u]).sum(1) / w.sum(1, keepdim=True)
        out.append(blend.argmax(1))
    return torch.cat(out)


def measure(lines, title, data, g, calls):
    dev = data.device
    N = data.shape[0]
    V = g.num_voxels()
    g = g.trim()
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    scores = torch.rand((V, NCLS), generator=gen, device=dev, dtype=torch.float32)
    voxel_labels = scores.argmax(1).to(torch.int32)
    neigh = g.neighbors()
    lab = torch.empty((N,), dtype=torch.int32, device=dev)
    both = (lab, torch.empty((N, NCLS), dtype=torch.float32, device=dev))

    def table():
        g._neigh = None
        g.neighbors()

    ours3 = g.interpolate(data, scores, k=3)
    theirs3 = torch_composition(data, g, neigh, scores, 3)
    agree = float((ours3.long() == theirs3).float().mean())
    st = g.interp_stats.tolist()
    t = alternated((table,
                    lambda: g.interpolate(data, scores, k=1, out=lab),
                    lambda: g.interpolate(data, scores, k=1, return_scores=True, out=both),
                    lambda: g.interpolate(data, scores, k=3, out=lab),
                    lambda: g.interpolate(data, scores, k=3, return_scores=True, out=both),
                    lambda: g.project(voxel_labels, out=lab),
                    lambda: torch_composition(data, g, neigh, scores, 1),
                    lambda: torch_composition(data, g, neigh, scores, 3)), calls)
    lines.append("")
    lines.append("%s: %d voxels (%.1f rows a voxel), %.1f of 27 neighbours a voxel; interp_stats %s; labels equal to the "
                 "composition's on %.4f of the rows (k = 3)" % (title, V, N / float(max(V, 1)),
                                                                 float((neigh >= 0).sum()) / max(V, 1), st, agree))
    lines.append("  %d calls a round" % calls)
    lines.append(show("neighbors (the table alone, 1 launch)", t[0]))
    lines.append(show("interpolate k = 1, labels", t[1], rate(N, 1, False, t[1])))
    lines.append(show("interpolate k = 1, labels and scores", t[2], rate(N, 1, True, t[2])))
    lines.append(show("interpolate k = 3, labels", t[3], rate(N, 3, False, t[3])))
    lines.append(show("interpolate k = 3, labels and scores", t[4], rate(N, 3, True, t[4])))
    lines.append(show("project(voxel labels)", t[5]))
    lines.append(show("torch composition k = 1, labels", t[6]))
    lines.append(show("torch composition k = 3, labels", t[7]))
    lines.append("  interpolate k = 1 is %s" % verdict(t[1], t[6], "the composition"))
    lines.append("  interpolate k = 3 is %s" % verdict(t[3], t[7], "the composition"))
    lines.append("  interpolate k = 3 costs %.1f x project (%.1f us more a call)" % (
        float(np.median(t[3])) / float(np.median(t[5])), float(np.median(t[3])) - float(np.median(t[5]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_interp_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    ap.add_argument("--no-rooms", action="store_true", help="skip the many-clouds shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_interp_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["interpolated projection against project and against gather + topk + weighted gather-sum in torch, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g, C = %d; uniform cubes"
             % (ROUNDS, K, VOXEL, NCLS),
             "the composition is given the call's own neighbour table and works in chunks of 2^21 rows"]
    if args.note:
        lines.insert(2, args.note)
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 3
        for per_voxel in PER_VOXEL:
            data, side = make_cloud(N, per_voxel, 6000 + per_voxel, dev)
            g = grid.grid_subsample(data, None, VOXEL, "mean")
            measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), data, g, calls)
            del data, g
            torch.cuda.empty_cache()
    if not args.no_rooms:
        data, side = make_cloud(ROOMS * ROOM_ROWS, 4, 6100, dev, rows_of_a_cube=ROOM_ROWS)   # every room fills the same cube
        start = torch.arange(0, (ROOMS + 1) * ROOM_ROWS, ROOM_ROWS, dtype=torch.int32, device=dev)
        g = grid.grid_subsample_rooms(data, start, None, VOXEL, "mean")
        measure(lines, "%d rooms x %d rows x %d, each in a cube of %.3f (many clouds)" % (ROOMS, ROOM_ROWS, K, side), data, g, 3)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
