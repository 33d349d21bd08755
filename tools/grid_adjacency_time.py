"""developer: time the segment adjacency (grid.GridSegments.adjacency: conv3p_grid_segment_adjacency, 5 + 6 b launches) and
the merge along every edge (SegmentAdjacency.merge: conv3p_grid_merge_segments, seven launches) against the composition a
caller writes in torch today, on the same device and GIVEN the same neighbour table and segment numbers:

    b = segment[neigh[:, taps]]                                  (M, taps) gathered
    ok = (neigh[:, taps] >= 0) & (b >= 0) & (b != segment[:, None])
    keys = (segment[:, None] * S + b)[ok]                        up to 26 M int64 keys
    edges, contacts = torch.unique(keys, return_counts=True)     a sort of all of them

which yields the edges and their contacts alone: no border voxels, no offsets, no twins, no CSR, no per-segment counts,
and its result's length is a host read.  For scale segments() on the same shape is timed too.

Clouds, label fields, rounds and the way a round is timed are tools/grid_segments_time.py's: 65 536, 1 048 576 and 2^24
rows at about 4 rows a voxel; one label, slabs of 16 cells with 5 % redrawn, 13 classes at random; connectivity 26.  The
adjacency is timed at max_edges = its own edges_bound() (the retry a caller makes; at the default 2 M the two noisy fields
overflow, which is timed as well).  Output: profiles/grid_adjacency_time.txt.

    python tools/grid_adjacency_time.py [--out profiles/grid_adjacency_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, build, grid
from tools.grid_segments_time import (CONNECTIVITY, K, NCLS, PER_VOXEL, ROUNDS, ROWS, VOXEL, alternated, label_fields, make_cloud,
                                      show, tap_columns, verdict)

KERNELS = ("adj_", "conv3p17merge_init", "conv3p18merge_union", "conv3p19merge_number", "conv3p19merge_assign", "conv3p19merge_finish")


def torch_edges(neigh, segment, S, cols):
    """-> (edge keys a * S + b ascending, contacts).  torch.unique reads the number of edges on the host."""
    u = neigh[:, cols].long()
    seg = segment.long()
    b = seg[u.clamp(min=0)]
    ok = (u >= 0) & (b >= 0) & (seg[:, None] >= 0) & (b != seg[:, None])
    keys = (seg[:, None] * S + b)[ok]
    return torch.unique(keys, return_counts=True)


def measure(lines, title, data, calls):
    dev = data.device
    g = grid.grid_subsample(data, None, VOXEL, "mean").trim()
    M = g.voxel_cell.shape[0]
    neigh = g.neighbors()
    cols = torch.tensor(tap_columns(CONNECTIVITY), device=dev)
    seg = grid.GridSegments(M, dev)
    lines.append("")
    lines.append("%s: %d voxels; %d calls a round (the torch composition: 1)" % (title, M, calls))
    mark = len(lines) - 2
    for name, lab in label_fields(g, dev):
        g.segments(lab, NCLS, CONNECTIVITY, out=seg)
        S = seg.num_segments()
        small = seg.adjacency()                          # the default max_edges = 2 M
        bound, over = small.edges_bound(), small.overflowed()
        adj = seg.adjacency(max_edges=max(bound, 1))
        E, st = adj.num_edges(), adj.stats.tolist()
        keys, counts = torch_edges(neigh, seg.segment, S, cols)
        agree = keys.numel() == E and bool(torch.equal(keys, adj.src[:E].long() * S + adj.dst[:E].long())) \
            and bool(torch.equal(counts.to(torch.int32), adj.contacts[:E]))
        merged = adj.merge()
        ms = merged.merge_stats.tolist()
        ws = _lib.load().conv3p_grid_adjacency_scratch_bytes(M, max(bound, 1))
        torch.cuda.synchronize()
        t = alternated((lambda: g.segments(lab, NCLS, CONNECTIVITY, out=seg),
                        lambda: seg.adjacency(out=small),
                        lambda: seg.adjacency(max_edges=max(bound, 1), out=adj),
                        lambda: adj.merge(out=merged),
                        lambda: torch_edges(neigh, seg.segment, S, cols)), calls)
        lines.append("  -- %s: %d segments, %d edges, B %d, %d contacts, largest degree %d, largest contacts %d; workspace %.1f MiB "
                     "at max_edges = B; the default max_edges = %d %s; merged along every edge: %d groups; the torch "
                     "composition: the same edges and contacts: %s"
                     % (name, S, E, bound, st[3], st[4], st[5], ws / 2.0 ** 20, 2 * M, "OVERFLOWS" if over else "fits", ms[0], agree))
        lines.append(show("segments (for scale, 7 launches)", t[0]))
        lines.append(show("adjacency, max_edges = 2 M%s" % (" (overflow)" if over else ""), t[1]))
        lines.append(show("adjacency, max_edges = B", t[2]))
        lines.append(show("merge along every edge (7 launches)", t[3]))
        lines.append(show("torch gather / keys / unique (contacts alone)", t[4]))
        lines.append("  adjacency at max_edges = B is %s; %.2f x segments"
                     % (verdict(t[2], t[4], "the torch composition"), float(np.median(t[2])) / float(np.median(t[0]))))
        del adj, small, merged, keys, counts
        torch.cuda.empty_cache()
        print("\n".join(lines[mark:]), flush=True)      # as it goes: a long run is seen to move
        mark = len(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_adjacency_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_adjacency_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["segment adjacency and merge against a gather / keys / torch.unique composition in torch, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes, about %d rows a "
             "voxel; connectivity %d, %d classes" % (ROUNDS, K, VOXEL, PER_VOXEL, CONNECTIVITY, NCLS),
             "the torch composition is given the call's own neighbour table and segment numbers and yields the edges' contacts alone"]
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
