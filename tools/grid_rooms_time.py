"""developer: time the many-clouds voxel-grid subsampling (grid.grid_subsample_rooms: conv3p_grid_subsample_rooms_f32,
28 launches in the mean mode whatever R) against what a caller had before it: the loop of grid.grid_subsample(...,
out=) calls over the rooms' slices, 24 launches a room, into preallocated per-room outputs.

The loop is timed WITHOUT the per-room num_voxels() reads (a synchronisation each), the concatenation of the per-room
outputs, the shift of every room's inverse and the upload of a room_start for the thinned rows, all of which a real
caller adds before scene_blocks_rooms can run.  That favours the loop.

Shapes (rooms x rows a room): 1 x 65 536, 64 x 65 536, 1024 x 4096, 1 x 4 194 304; every room uniform in a cube of its
own, at its own origin, whose side leaves about 4 rows a voxel; K = 6, voxel 0.05, the mean mode with uint8 labels of 13
classes.  Both sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair
of HIP events around back-to-back calls; every shape is warmed up first.  The spread of the rounds is printed next to
their median.  Output: profiles/grid_rooms_time.txt.

    python tools/grid_rooms_time.py [--out profiles/grid_rooms_time.txt] [--note TEXT] [--shapes 1x65536,64x65536,...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, grid

SHAPES = ((1, 65536), (64, 65536), (1024, 4096), (1, 1 << 22))
PER_VOXEL = 4
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


def verdict(ours, loop):
    """The one call's median below the loop's by more than the larger of the two spreads?"""
    mo, ml = float(np.median(ours)), float(np.median(loop))
    slack = max(spread(ours), spread(loop)) / 100.0
    if mo < ml * (1.0 - slack):
        word = "FASTER than the loop beyond the spread"
    elif mo > ml * (1.0 + slack):
        word = "SLOWER than the loop beyond the spread"
    else:
        word = "within the spread of the loop"
    return "%s (ratio loop / call %.2f)" % (word, ml / mo)


def make_rooms(R, rows, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * (rows / float(PER_VOXEL)) ** (1.0 / 3.0)
    data = torch.rand((R * rows, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    origin = torch.rand((R, 3), generator=g, device=dev, dtype=torch.float32) * 10.0 - 5.0
    data[:, :3] += origin.repeat_interleave(rows, dim=0)
    labels = torch.randint(0, NCLS, (R * rows,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
    start = (torch.arange(R + 1, dtype=torch.int64) * rows).to(torch.int32).to(dev)
    return data.contiguous(), labels, start, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "grid_rooms_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES), help="comma-separated ROOMSxROWS")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_rooms_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["many-clouds voxel-grid subsampling against the loop of single-cloud calls, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g, mean mode, uint8 labels, %d "
             "classes; about %d rows a voxel" % (ROUNDS, K, VOXEL, NCLS, PER_VOXEL),
             "the loop writes into preallocated per-room outputs and is timed without the per-room host reads, the "
             "concatenation, the inverse shift and the room_start upload a caller adds"]
    if args.note:
        lines.insert(2, args.note)
    for R, rows in [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]:
        N = R * rows
        calls = 10 if N <= (1 << 16) else 3
        data, labels, start, side = make_rooms(R, rows, 7000 + R, dev)
        g = grid.grid_subsample_rooms(data, start, labels, VOXEL, "mean", NCLS)
        slices = [(data[r * rows:(r + 1) * rows], labels[r * rows:(r + 1) * rows]) for r in range(R)]
        outs = [grid.grid_subsample(d, l, VOXEL, "mean", NCLS) for d, l in slices]

        def loop():
            for (d, l), o in zip(slices, outs):
                grid.grid_subsample(d, l, VOXEL, "mean", NCLS, out=o)

        V = g.num_voxels()
        per_room = [o.num_voxels() for o in outs]
        first = np.concatenate([[0], np.cumsum(per_room)])
        same = bool(V == first[-1] and g.voxel_start.tolist() == first.tolist()
                    and torch.equal(g.data[:V], torch.cat([o.data[:n] for o, n in zip(outs, per_room)]))
                    and torch.equal(g.labels[:V], torch.cat([o.labels[:n] for o, n in zip(outs, per_room)]))
                    and torch.equal(g.inverse, torch.cat([o.inverse + int(f) for o, f in zip(outs, first[:-1])])))
        st = g.stats.tolist()
        t = alternated((lambda: grid.grid_subsample_rooms(data, start, labels, VOXEL, "mean", NCLS, out=g), loop), calls)
        lines.append("")
        lines.append("%d rooms x %d rows x %d, cubes of %.3f: %d voxels (%.1f rows a voxel, the largest %d), error bits %d; "
                     "data, labels, inverse and voxel_start equal the loop's, stitched: %s"
                     % (R, rows, K, side, V, N / float(max(V, 1)), st[6], st[7], same))
        lines.append("  %d calls a round" % calls)
        lines.append(show("grid_subsample_rooms (28 launches)", t[0]))
        lines.append(show("loop of grid_subsample (%d x 24 launches)" % R, t[1]))
        lines.append("  the one call is %s" % verdict(t[0], t[1]))
        del g, outs, slices, data, labels
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
