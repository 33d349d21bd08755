"""developer: time the on-device agglomeration (grid.SegmentAdjacency.agglomerate: conv3p_grid_agglomerate_segments,
15 + 6 max_rounds + 6 b launches, no host read) against the loop a caller writes today, on the same device, the same
library and GIVEN the same segmentation:

    cur = seg
    while True:
        adj = cur.adjacency(max_edges=cap).trim()                # the walk over all voxels, and a host read (the edges)
        src, dst, E = adj.src.long(), adj.dst.long(), adj.src.numel()
        ok = (cur.size[src] < 8) & (cur.size[dst] >= 8)          # the README's policy: every small patch into the LARGE
        key = torch.where(ok, adj.contacts.long() * E + (E - 1 - torch.arange(E)), -1)      # patch it touches most
        best = torch.full_like(cur.size, -1, dtype=torch.int64).scatter_reduce(0, src, key, "amax")
        select = ok & (key == best[src])
        if not bool(select.any()): break                         # a host read: nothing changes any more
        cur = adj.merge(select)

The loop's policy is the narrower one: it never joins two small patches, so where specks touch each other it stops with
small patches left that agglomerate() folds away (rule H4 ranks a large neighbour first and a small one after it).  Both
group counts are reported.  The call is timed GIVEN the adjacency, which the loop's first round has to make as well; the
adjacency call alone is timed for scale, and `call + adjacency` is the figure to hold against the loop.

Clouds, label fields, rounds and the way a round is timed are tools/grid_segments_time.py's: 65 536, 1 048 576 and 2^24
rows at about 4 rows a voxel (16 911, 257 347 and 4 148 460 voxels); one label, slabs of 16 cells with 5 % redrawn, 13
classes at random; connectivity 26; min_size 8, the default 8 rounds; max_edges = the adjacency's own edges_bound().
Output: profiles/grid_agglomerate_time.txt.

    python tools/grid_agglomerate_time.py [--out profiles/grid_agglomerate_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, build, grid
from tools.grid_segments_time import (CONNECTIVITY, K, NCLS, PER_VOXEL, ROUNDS, ROWS, VOXEL, alternated, label_fields, make_cloud,
                                      show, verdict)

MIN_SIZE = 8
KERNELS = ("agg_",)


def caller_loop(seg, cap):
    """-> (the merged segmentation, rounds that merged something).  Two host reads a round."""
    cur, rounds = seg, 0
    while True:
        adj = cur.adjacency(max_edges=cap).trim()
        src, dst, E = adj.src.long(), adj.dst.long(), adj.src.numel()
        ok = (cur.size[src] < MIN_SIZE) & (cur.size[dst] >= MIN_SIZE)
        key = torch.where(ok, adj.contacts.long() * E + (E - 1 - torch.arange(E, device=src.device)), -1)
        best = torch.full_like(cur.size, -1, dtype=torch.int64).scatter_reduce(0, src, key, "amax")
        select = ok & (key == best[src])
        if not bool(select.any()):
            return cur, rounds
        cur = adj.merge(select)
        rounds += 1


def measure(lines, title, data, calls):
    dev = data.device
    g = grid.grid_subsample(data, None, VOXEL, "mean").trim()
    M = g.voxel_cell.shape[0]
    g.neighbors()
    seg = grid.GridSegments(M, dev)
    lines.append("")
    lines.append("%s: %d voxels; %d calls a round (the caller's loop: 1)" % (title, M, calls))
    mark = len(lines) - 2
    for name, lab in label_fields(g, dev):
        g.segments(lab, NCLS, CONNECTIVITY, out=seg)
        S = seg.num_segments()
        cap = max(seg.adjacency(max_edges=0).edges_bound(), 1)
        adj = seg.adjacency(max_edges=cap)
        E = adj.num_edges()
        res = adj.agglomerate(MIN_SIZE)
        st = res.stats.tolist()
        looped, loop_rounds = caller_loop(seg, cap)
        left = int((looped.size[:looped.num_segments()] < MIN_SIZE).sum())
        ws = _lib.load().conv3p_grid_agglomerate_scratch_bytes(M, cap)
        torch.cuda.synchronize()
        t = alternated((lambda: seg.adjacency(max_edges=cap, out=adj),
                        lambda: adj.agglomerate(MIN_SIZE, out=res),
                        lambda: caller_loop(seg, cap)), calls)
        both = [a + b for a, b in zip(t[0], t[1])]
        lines.append("  -- %s: %d segments, %d edges, max_edges %d; agglomerate: %d groups in %d rounds, %d merges, %d small left "
                     "(%d with a candidate), %d edges left, workspace %.1f MiB; the loop: %d groups in %d merging rounds "
                     "(and one that finds nothing), %d small left"
                     % (name, S, E, cap, st[0], st[2], st[3], st[4], st[5], st[7], ws / 2.0 ** 20, looped.num_segments(),
                        loop_rounds, left))
        lines.append(show("adjacency (for scale)", t[0]))
        lines.append(show("agglomerate, given the adjacency", t[1]))
        lines.append(show("adjacency + agglomerate", both))
        lines.append(show("the caller's loop (adjacency, policy, merge)", t[2]))
        lines.append("  adjacency + agglomerate is %s" % verdict(both, t[2], "the loop"))
        del adj, res, looped
        torch.cuda.empty_cache()
        print("\n".join(lines[mark:]), flush=True)      # as it goes: a long run is seen to move
        mark = len(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_agglomerate_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_agglomerate_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["agglomerate(min_size=%d) against the caller's loop of adjacency / policy / merge, %s" % (MIN_SIZE, torch.cuda.get_device_name(dev)),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes, about %d rows a "
             "voxel; connectivity %d, %d classes" % (ROUNDS, K, VOXEL, PER_VOXEL, CONNECTIVITY, NCLS),
             "the loop is the README's policy (small into LARGE only) iterated with its host reads; agglomerate also joins small with small"]
    if args.note:
        lines.insert(2, args.note)
    for name, v, vs, ss, scr in build.kernel_resources():
        if any(k in name for k in KERNELS):
            lines.append("%s: vgprs %d, vgpr spills %d, sgpr spills %d, private segment %d B" % (name, v, vs, ss, scr))
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 2
        data, side = make_cloud(N, 7104, dev)
        measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), data, calls)
        del data
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:                   # after every shape: a run cut short leaves what it measured
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
