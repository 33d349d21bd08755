"""developer: time the voxel-grid subsampling (grid.grid_subsample: conv3p_grid_subsample_f32, 24 launches in the mean
mode, 23 in the centre mode, whatever the data) against the composition a caller writes in torch today, on the same
device:

    lo = xyz.min(0); ijk = floor((xyz - lo) / voxel); c = (i_x n_y + i_y) n_z + i_z
    cells, inverse, counts = torch.unique(c, return_inverse=True, return_counts=True)
    mean = zeros(V, K).index_add_(0, inverse, data) / counts

That composition does LESS than the call: no labels, no voxel_row, no voxel_cell, its sums come from float atomics (so
neither their order nor their bits are defined) and torch.unique synchronises on the number of voxels.  The call is
timed with and without labels, and in the centre mode.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube whose side leaves about 4 and about 40 rows a voxel;
K = 6, voxel 0.05, 13 classes.  Both sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round
timed with one pair of HIP events around back-to-back calls; every shape is warmed up first.  The spread of the rounds is
printed next to their median, and a shape slower than the composition beyond that spread is called so.  Output:
profiles/grid_time.txt.

    python tools/grid_time.py [--out profiles/grid_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
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


def show(name, v):
    return "  %-52s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%" % (
        float(np.median(v)), spread(v))


def verdict(ours, other):
    """ours slower than the other side beyond the rounds' spread?"""
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    word = "SLOWER than the composition beyond the spread" if mo > mc * (1.0 + slack) else "not slower beyond the spread"
    return "%s (ratio composition / call %.2f)" % (word, mc / mo)


def make_cloud(N, per_voxel, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * (N / float(per_voxel)) ** (1.0 / 3.0)
    data = torch.rand((N, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    labels = torch.randint(0, NCLS, (N,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
    return data.contiguous(), labels, side


def torch_composition(data):
    xyz = data[:, :3]
    lo = xyz.min(dim=0).values
    ijk = torch.floor((xyz - lo) / torch.tensor(VOXEL, dtype=torch.float32, device=data.device)).to(torch.int64)   # a true division
    n = ijk.max(dim=0).values + 1
    c = (ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2]
    cells, inverse, counts = torch.unique(c, return_inverse=True, return_counts=True)
    sums = torch.zeros((cells.numel(), data.shape[1]), dtype=torch.float32, device=data.device).index_add_(0, inverse, data)
    return sums / counts[:, None].to(torch.float32), inverse, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["voxel-grid subsampling against torch.unique(return_inverse) + index_add_, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g, %d classes; uniform cubes"
             % (ROUNDS, K, VOXEL, NCLS),
             "the composition computes no labels, voxel_row or voxel_cell, sums with float atomics and synchronises once"]
    if args.note:
        lines.insert(2, args.note)
    for N in [int(x) for x in args.rows.split(",")]:
        calls = 10 if N <= (1 << 20) else 3
        for per_voxel in PER_VOXEL:
            data, labels, side = make_cloud(N, per_voxel, 6000 + per_voxel, dev)
            a = grid.grid_subsample(data, labels, VOXEL, "mean", NCLS)
            b = grid.grid_subsample(data, None, VOXEL, "mean")
            c = grid.grid_subsample(data, None, VOXEL, "center")
            mean_t, inv_t, cnt_t = torch_composition(data)
            V = a.num_voxels()
            same = bool(V == mean_t.shape[0] and torch.equal(inv_t.to(torch.int32), a.inverse)
                        and torch.equal(cnt_t.to(torch.int32), a.voxel_count[:V]))
            diff = float((a.data[:V] - mean_t).abs().max()) if same else float("nan")
            st = a.stats.tolist()
            t = alternated((lambda: grid.grid_subsample(data, labels, VOXEL, "mean", NCLS, out=a),
                            lambda: grid.grid_subsample(data, None, VOXEL, "mean", out=b),
                            lambda: grid.grid_subsample(data, None, VOXEL, "center", out=c),
                            lambda: torch_composition(data)), calls)
            lines.append("")
            lines.append("%d rows x %d in a cube of %.3f: %d voxels (%.1f rows a voxel, the largest %d), lattice %d x %d x %d; "
                         "voxels, inverse and counts equal the composition's: %s; largest |mean - composition's| %.3g"
                         % (N, K, side, V, N / float(max(V, 1)), st[6], st[2], st[3], st[4], same, diff))
            lines.append("  %d calls a round" % calls)
            lines.append(show("grid_subsample mean, labels (24 launches)", t[0]))
            lines.append(show("grid_subsample mean, no labels (24 launches)", t[1]))
            lines.append(show("grid_subsample center, no labels (23 launches)", t[2]))
            lines.append(show("torch.unique + index_add_ (no labels)", t[3]))
            lines.append("  the mean call with labels is %s" % verdict(t[0], t[3]))
            lines.append("  the mean call without labels is %s" % verdict(t[1], t[3]))
            del a, b, c, data, labels, mean_t, inv_t, cnt_t
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
