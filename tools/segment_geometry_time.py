"""developer: time the per-segment geometry (grid.GridSegments.geometry: conv3p_grid_segment_geometry, six launches, no
workspace) against the composition a caller writes in torch today, on the same device and GIVEN this library's
segmentation:

    lo, hi      = scatter_reduce amin / amax of voxel_cell and of data[:, :3] by segment          (4 scatters)
    moments     = index_add_ of float64 {1, d, d d^T} with d = cell - lo[segment]                 (float atomics)
    centroid, C = moments / W;  eigenvalues, axes = torch.linalg.eigh(C) (batched), flipped to descending, signs by argmax
    extent      = scatter_reduce amin / amax of (cell - centroid[segment]) @ axes[segment]^T     (2 scatters)

Its sums are float64 atomics whose order differs from run to run, where the call's are exact integers.  For scale the
segments() call on the same field is timed too.

Clouds of 65 536, 1 048 576 and 2^24 rows, uniform in a cube whose side leaves about 4 rows a voxel (16 911, 257 347 and
about 4.1 million voxels: the shapes of profiles/grid_segments_time.txt); K = 6, voxel 0.05; the three label fields of
that file: one label, 13 classes in slabs of 16 cells with 5 % of the voxels redrawn, 13 classes drawn at random;
connectivity 26; weight "voxels".  All sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a
round timed with one pair of HIP events around back-to-back calls; every shape is warmed up first.  The spread of the
rounds is printed next to their median, and the largest difference between the call and the composition in the
eigenvalues.  The kernels' registers, spills and private segments are printed first.  Output:
profiles/segment_geometry_time.txt.

    python tools/segment_geometry_time.py [--out profiles/segment_geometry_time.txt] [--note TEXT] [--rows 65536,1048576]
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
NCLS, CONNECTIVITY = 13, 26
KERNELS = ("geom_",)


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
    """-> [(name, int32 (M) labels)] over the trimmed subsampling's voxels: the fields of tools/grid_segments_time.py."""
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


def torch_composition(cell, xyz, segment, S):
    """Every voxel is a member here (all labelled).  -> (lo, hi, box_lo, box_hi, moments, centroid, eigenvalues, axes,
    ext_lo, ext_hi)."""
    dev = cell.device
    idx3 = segment[:, None].expand(-1, 3)
    big = torch.iinfo(torch.int32).max
    lo = torch.full((S, 3), big, dtype=torch.int32, device=dev).scatter_reduce_(0, idx3, cell, "amin")
    hi = torch.full((S, 3), -big, dtype=torch.int32, device=dev).scatter_reduce_(0, idx3, cell, "amax")
    blo = torch.full((S, 3), float("inf"), device=dev).scatter_reduce_(0, idx3, xyz, "amin")
    bhi = torch.full((S, 3), float("-inf"), device=dev).scatter_reduce_(0, idx3, xyz, "amax")
    d = (cell - lo[segment]).double()
    terms = torch.cat([torch.ones_like(d[:, :1]), d, d[:, :, None].mul(d[:, None, :]).reshape(-1, 9)], dim=1)
    mom = torch.zeros((S, 13), dtype=torch.float64, device=dev).index_add_(0, segment, terms)
    W = mom[:, :1]
    e = mom[:, 1:4] / W
    C = mom[:, 4:].reshape(S, 3, 3) / W[:, :, None] - e[:, :, None] * e[:, None, :]
    lam, vec = torch.linalg.eigh(C)
    lam = lam.flip(1).clamp_min(0.0)
    axes = vec.flip(2).transpose(1, 2)
    top = axes.gather(2, axes.abs().argmax(dim=2, keepdim=True))
    axes = axes * torch.where(top < 0, -1.0, 1.0)
    cen = lo.double() + e
    p = torch.einsum("va,vka->vk", cell.double() - cen[segment], axes[segment])
    elo = torch.full((S, 3), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, idx3, p, "amin")
    ehi = torch.full((S, 3), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, idx3, p, "amax")
    return lo, hi, blo, bhi, mom, cen, lam, axes, elo, ehi


def measure(lines, title, data, calls):
    dev = data.device
    g = grid.grid_subsample(data, None, VOXEL, "mean").trim()
    M = g.voxel_cell.shape[0]
    seg = grid.GridSegments(M, dev)
    geo = grid.SegmentGeometry(M, dev)
    xyz = g.data[:, :3].contiguous()
    lines.append("")
    lines.append("%s: %d voxels; %d calls a round" % (title, M, calls))
    first = len(lines)
    for name, lab in label_fields(g, dev):
        g.segments(lab, NCLS, CONNECTIVITY, out=seg)
        seg.geometry(out=geo)
        S = seg.num_segments()
        segment = seg.segment.long()
        ref = torch_composition(g.voxel_cell, xyz, segment, S)
        torch.cuda.synchronize()
        st = geo.stats.tolist()
        agree = bool(torch.equal(geo.cell_box[:S, :3], ref[0]) and torch.equal(geo.cell_box[:S, 3:], ref[1])
                     and torch.equal(geo.box[:S, :3], ref[2]) and torch.equal(geo.box[:S, 3:], ref[3])
                     and torch.equal(geo.moments[:S, 0].double(), ref[4][:, 0]))
        scale = float(ref[6].sum(dim=1).max().clamp_min(1.0))
        dlam = float((geo.eigenvalues[:S] - ref[6]).abs().max()) / scale
        t = alternated((lambda: seg.geometry(out=geo), lambda: torch_composition(g.voxel_cell, xyz, segment, S),
                        lambda: g.segments(lab, NCLS, CONNECTIVITY, out=seg)), calls)
        lines.append("  -- %s: %d segments, %d of one voxel, %d flat; boxes and W equal to the composition's: %s; eigenvalues "
                     "differ by at most %.1e of the largest trace" % (name, S, st[1], st[2], agree, dlam))
        lines.append(show("geometry (6 launches)", t[0]))
        lines.append(show("torch composition", t[1]))
        lines.append(show("segments (7 launches, for scale)", t[2]))
        lines.append("  geometry is %s; %.2f x segments" % (verdict(t[0], t[1], "the composition"),
                                                            float(np.median(t[0])) / float(np.median(t[2]))))
    print("\n".join(lines[first - 2:]), flush=True)      # as it goes: a long run is seen to move


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "segment_geometry_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    ap.add_argument("--calls", type=int, default=0, help="calls a round (0: 10, or 3 past 2^20 rows)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_geometry_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["per-segment geometry against scatter_reduce / index_add_ / batched eigh in torch, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes, about %d rows a "
             "voxel; connectivity %d, %d classes, weight voxels" % (ROUNDS, K, VOXEL, PER_VOXEL, CONNECTIVITY, NCLS),
             "the composition is given the call's own segmentation and number of segments"]
    if args.note:
        lines.insert(2, args.note)
    for name, v, vs, ss, scr in build.kernel_resources():
        if any(k in name for k in KERNELS):
            lines.append("%s: vgprs %d, vgpr spills %d, sgpr spills %d, private segment %d B" % (name, v, vs, ss, scr))
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = args.calls or (10 if N <= (1 << 20) else 3)
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
