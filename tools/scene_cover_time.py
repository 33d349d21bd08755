"""developer: time the covering mode of the scene tiling (scene.scene_blocks(cover=True): conv3p_scene_blocks_cover_f32,
eight launches) against the plain call of the same room (seven launches), per emitted block, and the votes by summed
probabilities (scene.SceneScores: conv3p_scene_vote_scores_f32, conv3p_scene_score_labels) against the torch
composition a user would write -- not against the code under test:
    add      torch.softmax(logits, -1), then index_add_ into a float32 (N, C) tensor (with the .long() the int32 room
             rows need on the way)
    labels   max / argmax / where over that tensor, and the two counts
at rooms of 65 536 and 1 048 576 rows, K = 6, P = 4096, block 1, stride 1 and 0.5, min_points 100, 13 classes: the rooms
and the plain call's max_blocks are tools/scene_time.py's.  The covering call's max_blocks is the number of blocks the
room needs, read from a first call with max_blocks = 1 (blocks_needed()), as a user who evaluates a room would size it.

Both sides in one process, alternated over 5 rounds, us per call INCLUDING Python, a round timed with one pair of HIP
events around 10 back-to-back calls; every shape is warmed up first.  The spread of the rounds is printed next to their
median.  The expectation to confirm or refute: at no shape slower than the other side beyond the rounds' spread.
Output: profiles/scene_cover_time.txt (--out).

    python tools/scene_cover_time.py [--out profiles/scene_cover_time.txt] [--note TEXT]
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


def show(name, v, per=1.0):
    return "  %-40s" % name + "  ".join("%10.1f" % (x / per) for x in v) + "   median %10.1f  spread %5.1f %%" % (
        float(np.median(v)) / per, spread(v))


def verdict(ours, other):
    """ours slower than the other side beyond the rounds' spread?"""
    mo, mc = float(np.median(ours)), float(np.median(other))
    slack = max(spread(ours), spread(other)) / 100.0
    return "slower beyond the spread" if mo > mc * (1.0 + slack) else "not slower beyond the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "scene_cover_time.txt"))
    ap.add_argument("--note", default="", help="a line for the header")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_cover_time: needs a HIP device")
    _lib.load()
    dev = torch.device("cuda:0")
    lines = ["covering mode against the plain call, SceneScores against softmax + index_add_ / argmax, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds of %d calls, alternated, HIP events; K = %d, P = %d, block %g, min_points %d, "
             "%d classes" % (ROUNDS, CALLS, K, P, BLOCK, MIN_POINTS, NCLS)]
    if args.note:
        lines.append(args.note)
    for N, extent in ROOMS:
        xyz = synth.room_like(1, N, 4000 + N % 997, extent)[0]
        rng = np.random.default_rng(N)
        room = torch.from_numpy(np.concatenate([xyz, rng.random((N, K - 3)).astype(np.float32)], axis=1)).to(dev)
        labels = torch.from_numpy(rng.integers(0, NCLS, size=N).astype(np.uint8)).to(dev)
        for stride in STRIDES:
            cells = [max(1, int(math.ceil((e - BLOCK) / stride)) + 1) for e in extent[0:2]]
            plain_mb = cells[0] * cells[1] + cells[0] + cells[1] + 1          # the jittered walls may add a row of cells
            cover_mb = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, 1, cover=True).blocks_needed()
            po = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, plain_mb)
            co = scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, cover_mb, cover=True)
            pn, cn = po.num_blocks(), co.num_blocks()
            split = int((torch.bincount(co.block_cell[:cn].long()) > 1).sum())
            distinct = [int(torch.unique(o.index[o.index >= 0]).numel()) for o in (po, co)]
            step = [0]

            def plain():
                step[0] += 1
                return scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, plain_mb, seed=1, step=step[0], out=po)

            def cover():
                step[0] += 1
                return scene.scene_blocks(room, labels, P, BLOCK, stride, MIN_POINTS, cover_mb, seed=1, step=step[0], out=co,
                                          cover=True)
            t = alternated((cover, plain))
            lines.append("")
            lines.append("room %d x %d over %g x %g m, stride %g: plain %d blocks (max_blocks %d, %d distinct rows), covering %d blocks "
                         "(%d cells split, %d distinct rows)" % (N, K, extent[0], extent[1], stride, pn, plain_mb, distinct[0], cn,
                                                                  split, distinct[1]))
            lines.append(show("covering (8 launches), per call", t[0]))
            lines.append(show("plain (7 launches), per call", t[1]))
            lines.append(show("covering, per emitted block", t[0], cn))
            lines.append(show("plain, per emitted block", t[1], pn))
            per = ([x / cn for x in t[0]], [x / pn for x in t[1]])
            lines.append("  per emitted block, covering is %s (ratio covering / plain %.2f)" % (
                verdict(*per), float(np.median(per[0])) / float(np.median(per[1]))))
            # the votes of the covering blocks: fixed fake activations per emitted row
            index = co.index[:cn].contiguous()
            logits = torch.from_numpy((rng.standard_normal((cn, P, NCLS)) * 4).astype(np.float32)).to(dev)
            sc = scene.SceneScores(N, NCLS, dev)
            acc = torch.zeros((N, NCLS), dtype=torch.float32, device=dev)

            def add():
                sc.add(logits, index)

            def add_comp():
                acc.index_add_(0, index.reshape(-1).long(), torch.softmax(logits, -1).reshape(-1, NCLS))
            v = alternated((add, add_comp))
            lines.append(show("SceneScores.add (1 launch), %d rows" % (cn * P), v[0]))
            lines.append(show("torch softmax + index_add_", v[1]))
            lines.append("  SceneScores.add is %s (ratio composition / SceneScores %.2f)" % (
                verdict(*v), float(np.median(v[1])) / float(np.median(v[0]))))

            def lab():
                sc._fresh = False
                return sc.labels()

            def lab_comp():
                most, arg = acc.max(dim=1)
                out = torch.where(most > 0, arg.to(torch.int32), torch.full_like(arg, -1, dtype=torch.int32))
                voted = (out >= 0).sum()
                return out, torch.stack([voted, acc.shape[0] - voted])
            w = alternated((lab, lab_comp))
            lines.append(show("SceneScores.labels (2 launches)", w[0]))
            lines.append(show("torch max / where / counts", w[1]))
            lines.append("  SceneScores.labels is %s (ratio composition / SceneScores %.2f)" % (
                verdict(*w), float(np.median(w[1])) / float(np.median(w[0]))))
            del po, co, logits, sc, acc
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
