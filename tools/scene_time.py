"""developer: time the scene tiling (scene.scene_blocks: conv3p_scene_blocks_f32, seven launches) and the vote
(scene.SceneVotes: conv3p_scene_vote + conv3p_scene_vote_labels) against the torch composition a user would write --
not against the code under test:
    blocks   min / max over the room, then per cell: four comparisons into a boolean mask, nonzero (a host
             synchronisation per cell: the member count decides what happens next), torch.randint draws, gathers,
             the block minimum, the concatenation of the nine channels; torch.stack at the end
    vote     a flat index_put_(accumulate=True) of ones over the valid rows; labels by max / argmax / where
at rooms of 65 536 and 1 048 576 rows, K = 6, P = 4096, block 1, stride 1 and 0.5, min_points 100.  The rooms are
synth.room_like's (floor, ceiling, two walls, clutter) over 6.3 x 4.4 and 24.3 x 20.4 metres; max_blocks is the
number of cells of that extent, as a user who knows the room would pass it.

Both sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair of HIP
events around CALLS back-to-back calls (the composition synchronises inside, per cell; the fused side never does);
every shape is warmed up first.  The spread of the rounds is printed next to their median.  Then the C entry point
alone, 50 back-to-back calls between one event pair, with the bytes it has to move at the least (the room read once,
the blocks written once) per second.
Output: profiles/scene_time.txt (--out).

    python tools/scene_time.py [--out profiles/scene_time.txt] [--note TEXT]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, scene, synth

ROOMS = ((65536, (6.3, 4.4, 3.0)), (1048576, (24.3, 20.4, 3.0)))
STRIDES = (1.0, 0.5)
K, P, BLOCK, MIN_POINTS, NCLS = 6, 4096, 1.0, 100, 13
ROUNDS, BARE = 5, 50


def torch_blocks(data, labels, P, block, stride, min_points):
    """PointNet's room2blocks_plus_normalized as a user would write it with torch on the device."""
    dev = data.device
    xyz = data[:, 0:3]
    s = xyz - xyz.min(dim=0).values
    lim = s.max(dim=0).values
    lx, ly = lim[0:2].tolist()                                   # a synchronisation: the tiling is data-dependent
    nbx = max(1, int(math.ceil((lx - block) / stride)) + 1)
    nby = max(1, int(math.ceil((ly - block) / stride)) + 1)
    sx, sy = s[:, 0], s[:, 1]
    blocks, labs, index = [], [], []
    for i in range(nbx):
        in_x = (sx >= i * stride) & (sx <= i * stride + block)
        for j in range(nby):
            idx = (in_x & (sy >= j * stride) & (sy <= j * stride + block)).nonzero().squeeze(1)   # a synchronisation
            n = idx.numel()
            if n < min_points:
                continue
            if n > P:
                pick = idx[torch.randint(n, (P,), device=dev)]
            else:
                pick = torch.cat([idx, idx[torch.randint(n, (P - n,), device=dev)]])
            rows, sb = data[pick], s[pick]
            centre = sb[:, 0:2].min(dim=0).values + block * 0.5
            blocks.append(torch.cat([sb[:, 0:2] - centre, sb[:, 2:3], rows[:, 3:], sb / lim], dim=1))
            labs.append(labels[pick].to(torch.int32))
            index.append(pick.to(torch.int32))
    return torch.stack(blocks), torch.stack(labs), torch.stack(index)


def torch_vote(votes, pred, index):
    N, C = votes.shape
    pred, index = pred.reshape(-1).long(), index.reshape(-1).long()
    ok = (index >= 0) & (index < N) & (pred >= 0) & (pred < C)
    flat = (index * C + pred)[ok]
    votes.view(-1).index_put_((flat,), torch.ones_like(flat, dtype=votes.dtype), accumulate=True)


def torch_vote_labels(votes):
    most, arg = votes.max(dim=1)
    lab = torch.where(most > 0, arg.to(torch.int32), torch.full_like(arg, -1, dtype=torch.int32))
    voted = (lab >= 0).sum()
    return lab, torch.stack([voted, votes.shape[0] - voted])


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def alternated(pairs):
    """pairs: (fn, calls per round) -> per fn the rounds' us per call; two warm-up calls each first."""
    for _ in range(2):
        for fn, _ in pairs:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in pairs]
    for _ in range(ROUNDS):
        for k, (fn, calls) in enumerate(pairs):
            t[k].append(timed(fn, calls))
    return t


def show(name, v):
    return "  %-34s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%" % (
        float(np.median(v)), 100.0 * (max(v) - min(v)) / float(np.median(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "scene_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_time: needs a HIP device")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["scene tiling and voting against the torch composition a user would write, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds, alternated, HIP events; K = %d, P = %d, block %g, min_points %d"
             % (ROUNDS, K, P, BLOCK, MIN_POINTS)]
    if args.note:
        lines.append(args.note)
    for N, extent in ROOMS:
        xyz = synth.room_like(1, N, 4000 + N % 997, extent)[0]
        rng = np.random.default_rng(N)
        room = torch.from_numpy(np.concatenate([xyz, rng.random((N, K - 3)).astype(np.float32)], axis=1)).to(dev)
        labels = torch.from_numpy(rng.integers(0, NCLS, size=N).astype(np.uint8)).to(dev)
        for stride in STRIDES:
            cells = [max(1, int(math.ceil((e - BLOCK) / stride)) + 1) for e in extent[0:2]]
            max_blocks = cells[0] * cells[1] + cells[0] + cells[1] + 1          # the jittered walls may add a row of cells
            out = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, max_blocks)
            nb = out.num_blocks()
            step = [0]

            def fused():
                step[0] += 1
                return scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, max_blocks, seed=1, step=step[0], out=out)

            def comp():
                return torch_blocks(room, labels, P, BLOCK, stride, MIN_POINTS)
            cb = comp()[0].shape[0]
            slow = 1 if N * nb > 1 << 24 else 3
            t = alternated(((fused, 10), (comp, slow)))
            ws = out.workspace
            a = (room.data_ptr(), labels.data_ptr(), N, K, 1, BLOCK, stride, P, MIN_POINTS, max_blocks, 1, 7, out.data.data_ptr(),
                 out.labels.data_ptr(), out.index.data_ptr(), out.block_cell.data_ptr(), out.block_count.data_ptr(),
                 out.stats.data_ptr(), ws.data_ptr(), ws.numel(), stream)

            def bare():
                if lib.conv3p_scene_blocks_f32(*a) != _lib.OK:
                    raise SystemExit("scene_time: conv3p_scene_blocks_f32 failed")
            bare()
            torch.cuda.synchronize()
            tb = [timed(bare, BARE) for _ in range(3)]
            nbytes = N * (4 * K + 1) + max_blocks * P * (4 * (K + 3) + 8)
            lines.append("")
            lines.append("room %d x %d over %g x %g m, stride %g: %d blocks emitted (composition: %d), max_blocks %d"
                         % (N, K, extent[0], extent[1], stride, nb, cb, max_blocks))
            lines.append(show("scene_blocks (7 launches)", t[0]))
            lines.append(show("torch composition", t[1]))
            lines.append("  %-34s" % "ratio composition / scene_blocks" + "  ".join("%10.2f" % (c / f) for f, c in zip(*t)))
            lines.append("  the C call alone, %d back to back, 3 rounds: " % BARE + "  ".join("%.1f" % v for v in tb) + " us;  room read"
                         " once + blocks written once = %.1f MB: " % (nbytes / 1e6)
                         + "  ".join("%.0f" % (nbytes / (v * 1e-6) / 1e9) for v in tb) + " GB/s")
            # the vote of these blocks: a fixed fake prediction per emitted row
            index = out.index
            pred = torch.from_numpy(rng.integers(0, NCLS, size=tuple(index.shape)).astype(np.int32)).to(dev)
            sv = scene.SceneVotes(N, NCLS, dev)
            tv = torch.zeros((N, NCLS), dtype=torch.int32, device=dev)

            def vote():
                sv.add(pred, index)
                return sv.labels()

            def vote_comp():
                torch_vote(tv, pred, index)
                return torch_vote_labels(tv)
            v = alternated(((vote, 10), (vote_comp, 10)))
            lines.append(show("SceneVotes add + labels (3 launches)", v[0]))
            lines.append(show("torch index_put_ + argmax", v[1]))
            lines.append("  %-34s" % "ratio composition / SceneVotes" + "  ".join("%10.2f" % (c / f) for f, c in zip(*v)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
