"""developer: time the k-nearest-voxel search (grid.GridSubsample.knn: conv3p_grid_knn_f32 -- two memsets, the spread and
bound kernels, the near kernel and, with rings > 1, the ring kernel on a fixed grid) and its two consumers, on the same
device and library:

    (a) knn alone, raw rows as the queries, k 3 and 8, rings 1 (the spread, bound and near kernels alone), 2 and 8,
        every voxel voted and 1 % voted; with the mean scanned and the certified share of the live queries;
    (b) knn + GridKnn.interpolate against the plain interpolate(k) and against interpolate(k, rings=R) at the same R;
    (c) the same against what computes the SAME neighbours in torch, over the voted voxels, in chunks of rows of at most
        2^28 distances, timed on the first 65 536 rows at most and scaled to all rows (its chunks are independent):
            d = torch.cdist(p, q_voted);  d2k, j = (d * d).topk(k, largest=False);  u = voted[j]
            w = 1 / d2k.clamp_min(1e-10);  out = (w[..., None] * scores[u]).sum(1) / w.sum(1, keepdim=True)
        (a k-NN over ALL voted voxels: what a certified row's table holds; the search never looks past `rings` cells);
    (d) knn over the voxels (points=None) + GridKnn.normals at k 9 and 16, rings 2, against normals();
    (e) with --parent-tree: the bench headline (bench.py --gpus 1) of this tree and of a checkout of the parent commit
        with its library built (its Python binds its own symbol tables), alternated in fresh child processes of this run.

A k-NN that must scan one ring past the first hit does more work than the ring call, which stops at the first cube that
is not empty, and far more than the plain call's 27 cells: the file says how much.  Clouds of 65 536, 1 048 576 and 2^24
rows, uniform in a cube with about 4 rows a voxel; K = 6, voxel 0.05, C = 13, labels only.  us per call INCLUDING Python,
5 rounds, alternated, a round timed with one pair of HIP events around back-to-back calls, every shape warmed up first;
the spread of the rounds next to their median.  Output: profiles/grid_knn_time.txt.

    python tools/grid_knn_time.py [--out profiles/grid_knn_time.txt] [--note TEXT] [--rows 65536,1048576,16777216]
                                  [--parent-tree PATH] [--bench-steps 20]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import numpy as np
import torch

from grid_interp_rings_time import BASELINE_DISTANCES, BASELINE_ROWS, K, NCLS, ROUNDS, VOXEL, alternated, make_cloud, show
from pointwise_amd import _lib, grid

ROWS = (65536, 1048576, 1 << 24)
KS, RINGS = (3, 8), (2, 8)


def torch_knn(p, q, voted, scores, k):
    """(c) on the rows p (n, 3) against the voted voxels' representatives q (v, 3) -> labels (n) int64."""
    out = []
    k = min(k, q.shape[0])
    chunk = max(1, BASELINE_DISTANCES // max(1, q.shape[0]))
    for a in range(0, p.shape[0], chunk):
        d = torch.cdist(p[a:a + chunk], q)
        d2k, j = (d * d).topk(k, dim=1, largest=False)
        u = voted[j]
        w = 1.0 / d2k.clamp_min(1e-10)
        out.append(((w[:, :, None] * scores[u]).sum(1) / w.sum(1, keepdim=True)).argmax(1))
    return torch.cat(out)


def med(v):
    return float(np.median(v))


def measure(lines, title, data, g, calls):
    dev = data.device
    N = data.shape[0]
    V = g.num_voxels()
    g = g.trim()
    gen = torch.Generator(device=dev)
    gen.manual_seed(78)
    scores = torch.rand((V, NCLS), generator=gen, device=dev, dtype=torch.float32)
    lab = torch.empty((N,), dtype=torch.int32, device=dev)
    g.neighbors()
    lines.append("")
    lines.append("%s: %d voxels (%.1f rows a voxel); %d calls a round" % (title, V, N / float(max(V, 1)), calls))
    for share in (1.0, 0.01):
        valid = None if share == 1.0 else torch.where(torch.rand((V,), generator=gen, device=dev) < share, 1, -1).to(torch.int32)
        voted = torch.arange(V, device=dev) if valid is None else torch.nonzero(valid >= 0)[:, 0]
        lines.append(" %s (%d of %d)" % ("every voxel voted" if valid is None else "1 % of the voxels voted", voted.numel(), V))
        for k in KS:
            tables = {r: grid.GridKnn(N, k, dev) for r in RINGS}

            def search(r):
                return lambda: g.knn(VOXEL, data, k=k, rings=r, valid_labels=valid, out=tables[r])

            def both(r):
                return lambda: g.knn(VOXEL, data, k=k, rings=r, valid_labels=valid, out=tables[r]).interpolate(scores, out=lab)

            def ringed(r):
                return lambda: g.interpolate(data, scores, k=min(k, 8), valid_labels=valid, rings=r, out=lab)

            one = grid.GridKnn(N, k, dev)
            fns = [lambda: g.interpolate(data, scores, k=min(k, 8), valid_labels=valid, out=lab),
                   lambda: g.knn(VOXEL, data, k=k, rings=1, valid_labels=valid, out=one)]
            for r in RINGS:
                fns += [search(r), both(r), ringed(r)]
            t = alternated(fns, calls)
            lines.append(show("k = %d: interpolate, the plain call" % k, t[0]))
            lines.append(show("k = %d, rings = 1: knn alone (no ring kernel)" % k, t[1]))
            for n, r in enumerate(RINGS):
                ts, tb, tr = t[2 + 3 * n:5 + 3 * n]
                search(r)()
                st = tables[r].stats.tolist()
                live = max(sum(st[:3]), 1)
                both(r)()
                labelled = int((lab >= 0).sum())
                lines.append(show("k = %d, rings = %d: knn alone" % (k, r), ts))
                lines.append("      mean scanned %.3f, certified %.4f of the live queries, %d of them with k neighbours; rows labelled %d of %d"
                             % (st[5] / live, st[4] / live, st[0], labelled, N))
                lines.append(show("k = %d, rings = %d: knn + interpolate" % (k, r), tb))
                lines.append(show("k = %d, rings = %d: interpolate(rings=%d)" % (k, r, r), tr))
                lines.append("      knn + interpolate is %.2f x the plain call and %.2f x the ring call at the same rings" % (
                    med(tb) / med(t[0]), med(tb) / med(tr)))
            rows = min(N, BASELINE_ROWS)
            p, q = data[:rows, :3].contiguous(), g.data[voted, :3].contiguous()
            big = q.shape[0] * rows > (1 << 34)
            tt = alternated((lambda: torch_knn(p, q, voted, scores, k),), 1, rounds=2 if big else ROUNDS, warm=1)[0]
            whole = med(tt) * N / rows
            lines.append(show("k = %d: torch cdist + topk + gather-sum, %d rows" % (k, rows), tt))
            lines.append("      scaled to %d rows: %.1f us, %.1f x knn + interpolate at rings = %d (which looks no further than %d cells)"
                         % (N, whole, whole / med(t[3 + 3 * (len(RINGS) - 1)]), RINGS[-1], RINGS[-1]))
            del p, q, tables
    # (d) the normals
    fns = [lambda: g.normals()]
    for k in (9, 16):
        fns.append(lambda k=k: g.knn(VOXEL, k=k, rings=2).normals())
    t = alternated(fns, calls)
    lines.append(" normals")
    lines.append(show("normals(), 27 cells", t[0]))
    for n, k in enumerate((9, 16)):
        nrm = g.knn(VOXEL, k=k, rings=2).normals()
        lines.append(show("knn(k = %d, rings = 2) + normals()" % k, t[1 + n]))
        lines.append("      %.2f x normals(); voxels with a normal %d of %d (normals(): %d)" % (
            med(t[1 + n]) / med(t[0]), int(nrm.stats[0]), V, int(g.normals().stats[0])))


def headline(lines, parent_tree, steps):
    """(e) bench.py's one JSON line, this tree and the parent's, alternated, each run a fresh child process."""
    trees = (("this tree", os.path.join(HERE, "..")), ("the parent's tree", os.path.abspath(parent_tree)))
    got = {name: [] for name, _ in trees}
    env = {k: v for k, v in os.environ.items() if k != "CONV3P_HIP_LIB"}
    for _ in range(2):
        for name, root in trees:
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "5"], env=env,
                                 cwd=root, capture_output=True, text=True, timeout=150)
            if out.returncode != 0:
                lines.append(" bench.py of %s failed: %s" % (name, out.stderr.strip().splitlines()[-1:] or out.returncode))
                return
            got[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    lines.append("")
    lines.append("the bench headline (bench.py --gpus 1 --steps %d --warmup 5), alternated, a fresh process each:" % steps)
    for name, _ in trees:
        lines.append("  %-18s %s" % (name, "   ".join("%s %s" % (r.get("value"), r.get("unit", "")) for r in got[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "grid_knn_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS), help="comma-separated row counts")
    ap.add_argument("--parent-tree", default="", help="a checkout of the parent commit with its library built, for (e)")
    ap.add_argument("--bench-steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_knn_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["k-nearest-voxel search and its consumers against the plain and the ring interpolation, cdist + topk in torch and "
             "normals(), %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, voxel %g, C = %d, labels only; uniform "
             "cubes; raw rows as the queries" % (ROUNDS, K, VOXEL, NCLS),
             "the torch composition is timed on at most %d rows, in chunks of at most 2^28 distances, and scaled" % BASELINE_ROWS]
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
    if args.parent_tree:
        headline(lines, args.parent_tree, args.bench_steps)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    if os.path.exists(args.out + ".part"):
        os.remove(args.out + ".part")


if __name__ == "__main__":
    main()
