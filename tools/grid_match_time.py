"""developer: time the segment matching (grid.GridSegments.match: c3p_grid_match_segments, 8 + 9 b launches) against the
torch composition that computes the same table, best partners and matches on the same device:

    p = segment[inverse];  key = p * T + truth over the units with p >= 0 and truth >= 0
    keys, inter = torch.unique(key, return_counts=True);  pp, tt = keys // T, keys % T
    union = bincount(p)[pp] + bincount(truth)[tt] - inter;  iou = inter / union            (float64)
    best_iou per segment and per instance by scatter_reduce(amax);  pred_match by a scatter of the rows with iou > 1/2

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube with about 4 rows a voxel (16 850 / 257 265 / 4 148 504
voxels with this generator), voxel 0.05.  The instances are planted boxes of 8 x 8 x 8 voxels; the segments are
segments(labels) of a labelling in boxes of the same size shifted by half a box, so a segment overlaps up to 8
instances.  Two inputs per size:
    (a) the rows in scan order -- sorted by their voxel, so consecutive rows share a pair: long runs;
    (b) the same rows shuffled -- every unit ends a run: the worst case of the walk.
weight "rows" and "voxels", max_pairs = M.  us per call INCLUDING Python, 5 rounds, alternated, a round timed with one pair
of HIP events around back-to-back calls, every shape warmed up first; the spread of the rounds next to their median.
Output: profiles/grid_match_time.txt.

    python tools/grid_match_time.py [--out profiles/grid_match_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import torch

from grid_interp_rings_time import K, ROUNDS, VOXEL, alternated, make_cloud, show
from pointwise_amd import _lib, grid

ROWS = (65536, 1048576, 1 << 24)
BOX = 8                                                  # voxels along a side of an instance
NCLS = 13


def boxes(xyz, shift, n):
    """The box of every point, of BOX voxels a side, the lattice shifted by `shift` voxels -> (ix, iy, iz) int64."""
    return torch.floor((xyz + shift * VOXEL) / (BOX * VOXEL)).to(torch.int64).clamp_(0, n - 1)


def torch_match(segment, inverse, truth, M, T):
    p = torch.where(inverse >= 0, segment[inverse.clamp(min=0).long()], -1).long()
    t = truth.long()
    ok = (p >= 0) & (t >= 0)
    keys, inter = torch.unique(p[ok] * T + t[ok], return_counts=True)
    pp, tt = keys // T, keys % T
    union = torch.bincount(p[ok], minlength=M)[pp] + torch.bincount(t[t >= 0], minlength=T)[tt] - inter
    iou = inter.double() / union.double()
    best_p = torch.zeros(M, dtype=torch.float64, device=iou.device).scatter_reduce(0, pp, iou, "amax")
    best_t = torch.zeros(T, dtype=torch.float64, device=iou.device).scatter_reduce(0, tt, iou, "amax")
    hit = iou > 0.5
    match = torch.full((M,), -1, dtype=torch.int64, device=iou.device).scatter(0, pp[hit], tt[hit])
    return keys, inter, best_p, best_t, match


def measure(lines, N, dev, calls):
    data, side = make_cloud(N, 4, 6004, dev)
    g0 = grid.grid_subsample(data, None, VOXEL, "mean")
    order = torch.argsort(g0.inverse, stable=True)
    n = int(side / (BOX * VOXEL)) + 2
    for title, rows in (("(a) scan order", data[order].contiguous()), ("(b) shuffled", data)):
        g = grid.grid_subsample(rows, None, VOXEL, "mean")
        V, M = g.num_voxels(), g.data.shape[0]
        b = boxes(rows[:, :3], 0.0, n)
        truth = (b[:, 0] + n * (b[:, 1] + n * b[:, 2])).to(torch.int32).contiguous()
        T = n * n * n
        s = boxes(g.data[:, :3], BOX / 2.0, n + 1)
        labels = ((s[:, 0] + 3 * s[:, 1] + 7 * s[:, 2]) % NCLS).to(torch.int32).contiguous()
        seg = g.segments(labels, NCLS)
        vtruth = torch.full((M,), -1, dtype=torch.int32, device=dev)
        vtruth[g.inverse.long()] = truth                 # any member's instance: a timing input, not a majority
        out = grid.SegmentMatch(M, T, M, 1, dev)
        seg.match(truth, T, out=out)
        st = out.stats.cpu().tolist()
        lines.append("")
        lines.append("%d rows x %d in a cube of %.3f, %s: %d voxels, %d segments, %d instances, %d pairs; %d calls a round"
                     % (N, K, side, title, V, st[2], st[3], st[0], calls))
        varg = torch.arange(M, dtype=torch.int32, device=dev)
        t = alternated((lambda: seg.match(truth, T, out=out),
                        lambda: seg.match(vtruth, T, weight="voxels", out=out),
                        lambda: torch_match(seg.segment, g.inverse, truth, M, T),
                        lambda: torch_match(seg.segment, varg, vtruth, M, T)), calls)
        lines.append(show("match, weight rows", t[0]))
        lines.append(show("match, weight voxels", t[1]))
        lines.append(show("torch composition, rows", t[2], "   %.2fx the call" % (sorted(t[2])[ROUNDS // 2] / sorted(t[0])[ROUNDS // 2])))
        lines.append(show("torch composition, voxels", t[3], "   %.2fx the call" % (sorted(t[3])[ROUNDS // 2] / sorted(t[1])[ROUNDS // 2])))
        del g, seg, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "grid_match_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_match_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["segment matching against the torch composition (unique over pred * T + truth, scatter_reduce), %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; voxel %g, instances of %d^3 voxels, max_pairs = M; "
             "uniform cubes" % (ROUNDS, VOXEL, BOX)]
    if args.note:
        lines.append(args.note)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for N in [int(x) for x in args.rows.split(",") if x]:
        measure(lines, N, dev, 10 if N <= (1 << 20) else 2)
        with open(args.out, "w") as f:                   # after every size: a long run that is cut keeps what it has
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
