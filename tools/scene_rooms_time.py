"""developer: time the many-rooms tiling (scene.scene_blocks_rooms: conv3p_scene_blocks_rooms_f32, 21 launches whatever
the rooms) against the single-room call (scene.scene_blocks: 7 launches plain, 8 covering), which this tree leaves as it
was:
    (a) R = 1: one room of 65 536 and of 1 048 576 rows, stride 1 and 0.5, plain and covering, against scene_blocks on
        the same room with the same max_blocks -- what the radix-sort fill costs or saves against the per-block fill
    (b) 64 rooms of 65 536 rows in one call (+ its one host read, num_blocks(), and trim()) against the loop a caller
        writes today: per room scene_blocks, num_blocks(), trim(), then torch.cat of data and index
K = 6, P = 4096, block 1, min_points 100; the rooms are tools/scene_time.py's.  max_blocks is what the room (or the rooms)
need, read from a first call, on both sides.

Both sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair of HIP
events around 10 back-to-back calls; every shape is warmed up first.  The spread of the rounds is printed next to their
median, and a shape slower than its baseline beyond that spread is called so.  Output: profiles/scene_rooms_time.txt.

    python tools/scene_rooms_time.py [--out profiles/scene_rooms_time.txt] [--note TEXT] [--rooms 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, scene, synth

ROOMS = ((65536, (6.3, 4.4, 3.0)), (1048576, (24.3, 20.4, 3.0)))
STRIDES = (1.0, 0.5)
K, P, BLOCK, MIN_POINTS = 6, 4096, 1.0, 100
ROUNDS, CALLS = 5, 10


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def alternated(fns):
    """-> per fn the rounds' us per call; two warm-up calls each first."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(ROUNDS):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, CALLS))
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / float(np.median(v))


def show(name, v):
    return "  %-44s" % name + "  ".join("%10.1f" % x for x in v) + "   median %10.1f  spread %5.1f %%" % (
        float(np.median(v)), spread(v))


def verdict(ours, other):
    """ours slower than the other side beyond the rounds' spread?"""
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    word = "SLOWER than its baseline beyond the spread" if mo > mc * (1.0 + slack) else "not slower beyond the spread"
    return "%s (ratio baseline / rooms call %.2f)" % (word, mc / mo)


def make_room(N, extent, seed, dev):
    xyz = synth.room_like(1, N, seed, extent)[0]
    rng = np.random.default_rng(seed)
    room = torch.from_numpy(np.concatenate([xyz, rng.random((N, K - 3)).astype(np.float32)], axis=1)).to(dev)
    return room, torch.from_numpy(rng.integers(0, 13, size=N).astype(np.uint8)).to(dev)


def needed(room, labels, stride, cover):
    """The blocks one room needs: kept cells (plain) or parts (covering), from a call with max_blocks = 1."""
    o = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, 1, cover=cover)
    return max(1, o.blocks_needed() if cover else int(o.stats[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "scene_rooms_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    ap.add_argument("--rooms", type=int, default=64, help="rooms of comparison (b)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_rooms_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["many rooms in one call against the single-room call, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds of %d calls, alternated, HIP events; K = %d, P = %d, block %g, min_points %d"
             % (ROUNDS, CALLS, K, P, BLOCK, MIN_POINTS), "(a) R = 1: scene_blocks_rooms against scene_blocks on the same room"]
    if args.note:
        lines.insert(2, args.note)
    for N, extent in ROOMS:
        room, labels = make_room(N, extent, 4000 + N % 997, dev)
        for stride in STRIDES:
            for cover in (False, True):
                mb = needed(room, labels, stride, cover)
                so = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, mb, cover=cover)
                ro = scene.scene_blocks_rooms(room, [0, N], labels, P, BLOCK, stride, MIN_POINTS, mb, cover=cover)
                same = bool(torch.equal(so.index, ro.index) and torch.equal(so.data.view(torch.int32), ro.data.view(torch.int32)))
                step = [0]

                def single():
                    step[0] += 1
                    return scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, mb, seed=1, step=step[0], out=so, cover=cover)

                def rooms():
                    step[0] += 1
                    return scene.scene_blocks_rooms(room, ro.room_start, labels, P, BLOCK, stride, MIN_POINTS, mb, seed=1,
                                                    step=step[0], out=ro, cover=cover)
                t = alternated((rooms, single))
                lines.append("")
                lines.append("room %d x %d over %g x %g m, stride %g, %s: %d blocks; outputs of both calls bitwise equal: %s" % (
                    N, K, extent[0], extent[1], stride, "covering" if cover else "plain", so.num_blocks(), same))
                lines.append(show("scene_blocks_rooms, R = 1 (21 launches)", t[0]))
                lines.append(show("scene_blocks (%d launches)" % (8 if cover else 7), t[1]))
                lines.append("  the rooms call is %s" % verdict(t[0], t[1]))
                del so, ro
        del room, labels
    # (b)
    R, N1, extent = args.rooms, ROOMS[0][0], ROOMS[0][1]
    made = [make_room(N1, extent, 5000 + r, dev) for r in range(R)]
    data = torch.cat([m[0] for m in made]).contiguous()
    labels = torch.cat([m[1] for m in made]).contiguous()
    start = [r * N1 for r in range(R + 1)]
    lines.append("")
    lines.append("(b) %d rooms of %d rows: one scene_blocks_rooms call + num_blocks() + trim() against the loop of %d scene_blocks "
                 "calls, each with num_blocks() and trim(), + torch.cat of data and index" % (R, N1, R))
    for stride, cover in ((1.0, False), (0.5, True)):
        mbs = [needed(made[r][0], made[r][1], stride, cover) for r in range(R)]
        outs = [scene.scene_blocks(made[r][0], made[r][1], P, BLOCK, stride, MIN_POINTS, mbs[r], cover=cover) for r in range(R)]
        ro = scene.scene_blocks_rooms(data, start, labels, P, BLOCK, stride, MIN_POINTS, sum(mbs), cover=cover)
        step = [0]

        def loop():
            step[0] += 1
            parts = []
            for r in range(R):
                parts.append(scene.scene_blocks(made[r][0], made[r][1], P, BLOCK, stride, MIN_POINTS, mbs[r], seed=1 + r,
                                                step=step[0], out=outs[r], cover=cover).trim())
            return torch.cat([p.data for p in parts]), torch.cat([p.index for p in parts])

        def rooms():
            step[0] += 1
            return scene.scene_blocks_rooms(data, ro.room_start, labels, P, BLOCK, stride, MIN_POINTS, sum(mbs), seed=1,
                                            step=step[0], out=ro, cover=cover).trim()
        step[0] = 100
        a = loop()
        step[0] = 100
        b = rooms()
        offs = torch.repeat_interleave(torch.tensor(start[:-1], dtype=torch.int32, device=dev),
                                       torch.tensor([int(o.stats[0]) for o in outs], device=dev))
        same = bool(torch.equal(a[0].view(torch.int32), b.data.view(torch.int32)) and torch.equal(a[1] + offs[:, None], b.index))
        t = alternated((rooms, loop))
        lines.append("")
        lines.append("stride %g, %s: %d blocks in all; data and index (+ room_start) of both sides bitwise equal: %s" % (
            stride, "covering" if cover else "plain", b.data.shape[0], same))
        lines.append(show("scene_blocks_rooms, R = %d (21 launches)" % R, t[0]))
        lines.append(show("loop of %d scene_blocks + cat" % R, t[1]))
        lines.append("  the rooms call is %s" % verdict(t[0], t[1]))
        del outs, ro, a, b
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
