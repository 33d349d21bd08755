"""developer: time the connected segments (grid.GridSubsample.segments: conv3p_grid_segments, seven launches) and the
clean-up of small ones (GridSegments.absorb: conv3p_grid_absorb_segments, six launches) against the loop a caller writes
in torch today, on the same device and GIVEN this call's own neighbour table:

    u = neigh[:, taps];  u = where(u >= 0 and lab[u] == lab[:, None], u, own number)          (M, taps), once
    comp = arange(M)
    repeat:  new = minimum(comp, comp[u].amin(1));  new = new[new]  (pointer jumping)
             until (new == comp).all()  -- one host read a pass

which ends with comp[v] = the segment's root; it gives no numbering, sizes or rows, and its pass count grows with the
segments' diameter.  For scale the neighbors() launch and the grid_subsample call on the same shape are timed too.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube whose side leaves about 4 rows a voxel; K = 6, voxel 0.05;
three label fields over the voxels: one label (one segment: the contended size adds), 13 classes in slabs of 16 cells with
5 % of the voxels redrawn, and 13 classes drawn at random.  connectivity 26, min_size 4.  All sides in one process,
alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair of HIP events around back-to-back calls;
every shape is warmed up first.  The spread of the rounds is printed next to their median.  The kernels' registers,
spills and private segments are printed first.  Output: profiles/grid_segments_time.txt.

    python tools/grid_segments_time.py [--out profiles/grid_segments_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, build, grid

ROWS = (65536, 1048576, 1 << 24)
PER_VOXEL = 4
K, VOXEL = 6, 0.05
ROUNDS = 5
NCLS, CONNECTIVITY, MIN_SIZE = 13, 26, 4
KERNELS = ("gseg_", "absorb_")


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def alternated(fns, calls):
    """-> per fn the rounds' us per call; two warm-up calls each first.  The last fn, the torch loop, is called once a
    round (it is orders of magnitude slower)."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(ROUNDS):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, calls if k + 1 < len(fns) else 1))
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / float(np.median(v))


def show(name, v, extra=""):
    return "  %-46s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%%s" % (
        float(np.median(v)), spread(v), extra)


def verdict(ours, other, what):
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    word = "SLOWER than" if mo > mc * (1.0 + slack) else "faster than" if mc > mo * (1.0 + slack) else "within the spread of"
    return "%s %s (ratio %s / call %.2f)" % (word, what, what, mc / mo)


def make_cloud(N, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    side = VOXEL * (N / float(PER_VOXEL)) ** (1.0 / 3.0)
    data = torch.rand((N, K), generator=g, device=dev, dtype=torch.float32)
    data[:, :3] *= side
    return data.contiguous(), side


def label_fields(g, dev):
    """-> [(name, int32 (M) labels)] over the trimmed subsampling's voxels."""
    M = g.voxel_cell.shape[0]
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    cell = g.voxel_cell.long()
    smooth = ((cell[:, 0] // 16) * 5 + (cell[:, 1] // 16) * 3 + cell[:, 2] // 16) % NCLS
    noise = torch.rand(M, generator=gen, device=dev) < 0.05
    drawn = torch.randint(0, NCLS, (M,), generator=gen, device=dev)
    return [("one label", torch.zeros(M, dtype=torch.int32, device=dev)),
            ("slabs of 16 cells, 5 % redrawn", torch.where(noise, drawn, smooth).to(torch.int32).contiguous()),
            ("13 classes at random", drawn.to(torch.int32).contiguous())]


def tap_columns(connectivity):
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [t for t in range(27) if 1 <= abs(t // 9 - 1) + abs(t // 3 % 3 - 1) + abs(t % 3 - 1) <= reach]


def torch_loop(neigh, lab, cols):
    """-> (comp (M) int64, passes).  One .item() a pass."""
    M = neigh.shape[0]
    own = torch.arange(M, device=neigh.device)
    u = neigh[:, cols].long()
    ok = u >= 0
    u = torch.where(ok, u, own[:, None])
    u = torch.where(lab[u] == lab[:, None], u, own[:, None])
    comp, passes = own, 0
    while True:
        new = torch.minimum(comp, comp[u].amin(1))
        new = new[new]
        passes += 1
        if bool((new == comp).all().item()):
            return comp, passes
        comp = new


def measure(lines, title, data, calls):
    dev = data.device
    full = grid.grid_subsample(data, None, VOXEL, "mean")
    g = full.trim()
    M = g.voxel_cell.shape[0]
    neigh = g.neighbors()
    cols = torch.tensor(tap_columns(CONNECTIVITY), device=dev)
    seg = grid.GridSegments(M, dev)
    out = torch.empty(M, dtype=torch.int32, device=dev)

    def table():
        g._neigh = None
        g.neighbors()

    lines.append("")
    lines.append("%s: %d voxels, %.1f of 27 neighbours a voxel; %d calls a round (the torch loop: 1)"
                 % (title, M, float((neigh >= 0).sum()) / max(M, 1), calls))
    first = len(lines)
    scale = alternated((lambda: grid.grid_subsample(data, None, VOXEL, "mean", out=full), table, lambda: None), calls)
    lines.append(show("grid_subsample (for scale)", scale[0]))
    lines.append(show("neighbors (for scale, 1 launch)", scale[1]))
    for name, lab in label_fields(g, dev):
        g.segments(lab, NCLS, CONNECTIVITY, out=seg)
        seg.absorb(MIN_SIZE, out=out)
        comp, passes = torch_loop(neigh, lab, cols)
        torch.cuda.synchronize()
        S, st, ab = seg.num_segments(), seg.stats.tolist(), seg.absorb_stats.tolist()
        roots = int((comp == torch.arange(M, device=dev)).sum())
        agree = bool(torch.equal(seg.root[seg.segment.long()].long(), comp))
        t = alternated((lambda: g.segments(lab, NCLS, CONNECTIVITY, out=seg),
                        lambda: seg.absorb(MIN_SIZE, out=out),
                        lambda: torch_loop(neigh, lab, cols)), calls)
        lines.append("  -- %s: %d segments, largest %d voxels; small %d, absorbed %d, orphans %d, voxels relabelled %d; the torch "
                     "loop: %d passes, %d roots, the same partition: %s" % (name, S, st[4], ab[0], ab[1], ab[2], ab[3], passes,
                                                                           roots, agree))
        lines.append(show("segments (7 launches)", t[0]))
        lines.append(show("absorb (6 launches)", t[1]))
        lines.append(show("torch loop (segments' roots alone)", t[2]))
        lines.append("  segments is %s; %.2f x neighbors, %.2f x grid_subsample"
                     % (verdict(t[0], t[2], "the torch loop"), float(np.median(t[0])) / float(np.median(scale[1])),
                        float(np.median(t[0])) / float(np.median(scale[0]))))
    print("\n".join(lines[first - 2:]), flush=True)      # as it goes: a long run is seen to move


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_segments_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_segments_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["connected segments and the absorb against a gather / amin / pointer-jumping loop in torch, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes, about %d rows a "
             "voxel; connectivity %d, min_size %d, %d classes" % (ROUNDS, K, VOXEL, PER_VOXEL, CONNECTIVITY, MIN_SIZE, NCLS),
             "the torch loop is given the call's own neighbour table and reads one flag on the host a pass"]
    if args.note:
        lines.insert(2, args.note)
    for name, v, vs, ss, scr in build.kernel_resources():
        if any(k in name for k in KERNELS):
            lines.append("%s: vgprs %d, vgpr spills %d, sgpr spills %d, private segment %d B" % (name, v, vs, ss, scr))
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 3
        data, side = make_cloud(N, 7104, dev)
        measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), data, calls)
        del data
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
