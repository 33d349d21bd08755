"""developer: time the smooth segments (grid.GridSubsample.segments(normals=...): conv3p_grid_segments_smooth, seven launches
behind a memset) and the per-segment pool (GridSegments.pool: conv3p_grid_segment_pool_f32, four launches) on the shapes
and label fields of tools/grid_segments_time.py, whose clouds, fields, rounds and spread discipline this tool imports:

    (a) the smooth call, fed the normals of normals(), against the plain segments() on the same field, both through
        Python and this library (the plain call is the parent commit's to within (d));
    (b) the smooth call against the torch loop of tools/grid_segments_time.py with the predicate folded into its `where`;
    (c) pool at C = 13 against torch's index_add_ over seg.segment (float32 atomics: neither exact nor reproducible);
    (d) conv3p_grid_segments of this library against the PARENT commit's library, named by --parent-lib, both called
        through ctypes with the very pointers segments() passes: what sharing the two union-find kernels' bodies with
        the smooth rule cost the plain call.

All sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair of HIP
events around back-to-back calls; every shape is warmed up first.  The normals of a uniform cube are noise, so the
smooth segments are small: the refused pairs dominate, which is the predicate's worst case.  max_angle 30, connectivity
26.  Output: profiles/grid_smooth_time.txt.

    python tools/grid_smooth_time.py [--out profiles/grid_smooth_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
                                     [--parent-lib PATH/libconv3p_hip.so]
"""
import argparse
import ctypes
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from grid_segments_time import (CONNECTIVITY, K, NCLS, PER_VOXEL, ROUNDS, ROWS, VOXEL, alternated, label_fields, make_cloud,
                                show, tap_columns, verdict)
from pointwise_amd import _lib, build, grid

MAX_ANGLE, POOL_C = 30, 13
KERNELS = ("gseg_local", "gseg_link", "smooth_", "pool_")


def torch_loop_smooth(neigh, lab, cols, normals, has, min_cos):
    """tools/grid_segments_time.py's loop with J2 folded into the `where` -> (comp (M) int64, passes)."""
    M = neigh.shape[0]
    own = torch.arange(M, device=neigh.device)
    u = neigh[:, cols].long()
    u = torch.where(u >= 0, u, own[:, None])
    d = (normals[u] * normals[:, None, :]).sum(dim=2).abs()
    join = (lab[u] == lab[:, None]) & has[u] & has[:, None] & (d >= min_cos)
    u = torch.where(join, u, own[:, None])
    comp, passes = own, 0
    while True:
        new = torch.minimum(comp, comp[u].amin(1))
        new = new[new]
        passes += 1
        if bool((new == comp).all().item()):
            return comp, passes
        comp = new


def parent_segments(path):
    """The parent commit's conv3p_grid_segments through ctypes -> a function of (g, lab, seg) that calls it on the tensors
    GridSubsample.segments would pass."""
    lib = ctypes.CDLL(path)
    fn = lib.conv3p_grid_segments
    fn.restype, fn.argtypes = _lib.SYMBOLS["conv3p_grid_segments"]

    def call(g, lab, seg, ws):
        M = g.voxel_count.shape[0]
        rc = fn(g.neighbors().data_ptr(), lab.data_ptr(), lab.numel(), g.voxel_count.data_ptr(), g.stats.data_ptr(), M, NCLS,
                CONNECTIVITY, seg.segment.data_ptr(), seg.root.data_ptr(), seg.size.data_ptr(), seg.rows.data_ptr(),
                seg.label.data_ptr(), seg.stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


def measure(lines, title, data, calls, parent):
    dev = data.device
    g = grid.grid_subsample(data, None, VOXEL, "mean").trim()
    M = g.voxel_cell.shape[0]
    neigh = g.neighbors()
    cols = torch.tensor(tap_columns(CONNECTIVITY), device=dev)
    nrm = g.normals()
    has = nrm.flags == 0
    min_cos = float(np.float32(math.cos(math.radians(MAX_ANGLE))))
    plain, smooth, other = grid.GridSegments(M, dev), grid.GridSegments(M, dev), grid.GridSegments(M, dev)
    values = torch.rand((M, POOL_C), device=dev) * 2 - 1
    acc = torch.zeros((M, POOL_C), device=dev)
    lines.append("")
    lines.append("%s: %d voxels, %d with a normal; %d calls a round (the torch loop: 1)" % (title, M, int(has.sum()), calls))
    first = len(lines)
    for name, lab in label_fields(g, dev):
        g.segments(lab, NCLS, CONNECTIVITY, out=plain)
        g.segments(lab, NCLS, CONNECTIVITY, out=smooth, normals=nrm, max_angle=MAX_ANGLE)
        comp, passes = torch_loop_smooth(neigh, lab, cols, nrm.normals, has, min_cos)
        pool = smooth.pool(values)
        torch.cuda.synchronize()
        agree = bool(torch.equal(smooth.root[smooth.segment.long()].long(), comp))
        st = smooth.smooth_stats.tolist()
        lines.append("  -- %s: plain %d segments, smooth %d (largest %d voxels); pairs %d, joined %d, no normal %d, angle %d; the "
                     "torch loop: %d passes, the same partition: %s" % (name, plain.num_segments(), smooth.num_segments(),
                                                                       smooth.stats.tolist()[4], st[0], st[1], st[2], st[3],
                                                                       passes, agree))
        seg_long = smooth.segment.long()

        def index_add():
            acc.zero_()
            acc.index_add_(0, seg_long, values)

        fns = [lambda: g.segments(lab, NCLS, CONNECTIVITY, out=smooth, normals=nrm, max_angle=MAX_ANGLE),
               lambda: g.segments(lab, NCLS, CONNECTIVITY, out=plain)]
        if parent is not None:
            ws = plain.workspace
            fns += [lambda: parent[0](g, lab, other, ws), lambda: parent[1](g, lab, other, ws)]
        fns += [lambda: smooth.pool(values, out=pool), index_add,
                lambda: torch_loop_smooth(neigh, lab, cols, nrm.normals, has, min_cos)]
        t = alternated(fns, calls)
        ts, tp, tmine, tpar = t[0], t[1], (t[2] if parent is not None else None), (t[3] if parent is not None else None)
        tpool, tadd, tloop = t[-3], t[-2], t[-1]
        if parent is not None:                           # the parent's outputs are the plain call's, word for word
            same = all(torch.equal(getattr(other, k), getattr(plain, k)) for k in ("segment", "root", "size", "rows", "label", "stats"))
            lines.append("  the parent's library gives the plain call's outputs: %s" % same)
        lines.append(show("smooth segments (memset + 7 launches)", ts))
        lines.append(show("plain segments, this library", tp))
        if parent is not None:
            lines.append(show("plain segments, this library (ctypes)", tmine))
            lines.append(show("plain segments, the parent's library (ctypes)", tpar))
        lines.append(show("torch loop with the predicate", tloop))
        lines.append(show("pool, C = 13 (4 launches)", tpool))
        lines.append(show("torch zero_ + index_add_, C = 13 (float)", tadd))
        lines.append("  (a) smooth / plain, both through Python, this library: ratio %.2f"
                     % (float(np.median(ts)) / float(np.median(tp))))
        lines.append("  (b) smooth is %s" % verdict(ts, tloop, "the torch loop"))
        lines.append("  (c) pool is %s" % verdict(tpool, tadd, "index_add_"))
        if parent is not None:
            lines.append("  (d) the default call, both through ctypes, is %s" % verdict(tmine, tpar, "the parent's library"))
    print("\n".join(lines[first - 2:]), flush=True)      # as it goes: a long run is seen to move


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "grid_smooth_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libconv3p_hip.so, for (a) and (d)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_smooth_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    parent = (parent_segments(_lib.LIB_PATH), parent_segments(args.parent_lib)) if args.parent_lib else None   # (this, parent)
    lines = ["smooth segments and the per-segment pool against the plain segments, a torch loop and index_add_, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g; uniform cubes, about %d rows a "
             "voxel; connectivity %d, %d classes, max_angle %d; normals from normals(): noise in a uniform cube"
             % (ROUNDS, K, VOXEL, PER_VOXEL, CONNECTIVITY, NCLS, MAX_ANGLE),
             "the parent commit's library: %s" % ("given" if parent else "not given, (d) is not measured")]
    if args.note:
        lines.insert(2, args.note)
    for name, v, vs, ss, scr in build.kernel_resources():
        if any(k in name for k in KERNELS):
            lines.append("%s: vgprs %d, vgpr spills %d, sgpr spills %d, private segment %d B" % (name, v, vs, ss, scr))
    for N in [int(x) for x in args.rows.split(",") if x]:
        calls = 10 if N <= (1 << 20) else 3
        data, side = make_cloud(N, 7104, dev)
        measure(lines, "%d rows x %d in a cube of %.3f" % (N, K, side), data, calls, parent)
        del data
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
