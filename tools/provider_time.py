"""developer: time the fused batch provider (provider.assemble_batch: conv3p_provider_batch_f32, one launch) against
the composition it replaces -- index the resident set with torch, draw B angles with numpy on the host and upload
cos / sin, draw B x N x 3 float64 normals with torch.randn, prestep.rotate_and_jitter, prestep.sort_order_xyz and the
gathers, the [:, :, 0:3] slice, the label cast -- at
    32 x 2048 x 3    rotate + jitter + sort     (the classification model's batch)
    128 x 4096 x 9   sort only                  (param.json's segmentation batch)
    16 x 8192 x 12   sort only
    32 x 2048 x 3    rotate + jitter, no sort

Both in one process, alternated: 5 rounds x 20 calls each, us per call INCLUDING Python, a round timed with one pair
of HIP events; every size is warmed up first; nothing synchronises inside a round.  Then the C entry point alone,
200 back-to-back calls between one event pair.  For the two large sizes also the achieved bytes per second of
(4 K + 12 + label bytes) * 2 per point (rows, points and labels, read and written), from the C call alone.
Output: profiles/provider_time.txt (--out).

--morton: the three sorted shapes with sort_method="morton" instead.  Per shape and round, alternated: the xyz fused call
(the yardstick: its kernel is the one timed above), the Morton fused call, and the composition with
prestep.sort_order_morton in place of sort_order_xyz; then the C call alone with CONV3P_PROVIDER_MORTON.
Output: profiles/provider_morton_time.txt.

--wide: the wide entry (assemble_batch(wide_sort=True): conv3p_provider_batch_wide_f32, several launches, a cloud spread
over many workgroups).  On the three sorted shapes, per method and round, alternated: the one-launch call (the yardstick),
the wide call and the composition; then both C calls alone.  At 4 x 65536 x 9 and 16 x 20000 x 3, beyond the one-launch
call's limit: the wide call, its C call alone with bytes per second, and -- for orientation only -- what a user would
write in torch: three stable torch.argsort as util.py:66-68, plus the gathers.
--wide-sort: the sort alone, prestep.sort_order (conv3p_sort_order_f32) against prestep.sort_order_xyz / _morton on the
same shapes' clouds, and against the three argsorts on the two large ones.
--note TEXT is written into the header (which build of the library was timed).
Output: profiles/wide_sort_time.txt; --wide-sort appends to it when --wide wrote it first (--append).

    python tools/provider_time.py [--out profiles/provider_time.txt]
    python tools/provider_time.py --morton [--out profiles/provider_morton_time.txt]
    python tools/provider_time.py --wide [--note TEXT] [--out profiles/wide_sort_time.txt]
    python tools/provider_time.py --wide-sort --append [--note TEXT] [--out profiles/wide_sort_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from pointwise_amd import _lib, prestep, provider

# B, N, K, augment, sort, labels per point, samples in the resident set, what
SIZES = ((32, 2048, 3, True, True, False, 256, "rotate + jitter + sort"),
         (128, 4096, 9, False, True, True, 256, "sort only: param.json's segmentation batch"),
         (16, 8192, 12, False, True, True, 64, "sort only"),
         (32, 2048, 3, True, False, False, 256, "rotate + jitter, no sort"))
ROUNDS, CALLS, BARE = 5, 20, 200


def composition(data, labels, perm, start, B, augment, sort, sort_order=prestep.sort_order_xyz):
    """What a user of prestep.py does per batch without the fused call."""
    idx = perm[start:start + B].long()
    rows = data[idx]
    lab = labels[idx]
    xyz = rows if rows.shape[2] == 3 else rows[:, :, 0:3].contiguous()
    if augment:
        xyz = prestep.rotate_and_jitter(xyz)              # numpy angles + upload, torch.randn float64, one launch
        rows = xyz if rows.shape[2] == 3 else torch.cat([xyz, rows[:, :, 3:]], dim=2)
    if sort:
        order = sort_order(rows)
        rows = prestep._gather(rows, order)
        if lab.dim() == 2:
            lab = prestep._gather(lab, order)
    return rows[:, :, 0:3].contiguous(), rows, lab.to(torch.int32)


def timed(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags, o, stream, entry="conv3p_provider_batch_f32"):
    """The C entry point alone: BARE back-to-back calls between one event pair, 3 rounds."""
    fn = getattr(lib, entry)
    ws = o.workspace
    a = (data.data_ptr(), labels.data_ptr(), S, N, K, 1, int(per_point), perm.data_ptr(), S, 0, B, N, flags, 0.01, 0.05,
         1, 7, None, None, o.points.data_ptr(), o.input.data_ptr(), o.labels.data_ptr(), None, None, None,
         o.bad_index.data_ptr(), ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream)

    def bare():
        if fn(*a) != _lib.OK:
            raise SystemExit("provider_time: %s failed" % entry)
    bare()
    torch.cuda.synchronize()
    return [timed(bare, BARE) for _ in range(3)]


def resident_set(B, N, K, per_point, S, dev):
    g = torch.Generator(device="cpu").manual_seed(B + N + K)
    data = torch.rand(S, N, K, generator=g).to(dev)
    labels = torch.randint(0, 13, (S, N) if per_point else (S,), generator=g).to(torch.uint8).to(dev)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(S).astype(np.int32)).to(dev)
    return data, labels, perm


def main_morton(out_path):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["fused batch provider, sort_method=\"morton\" against \"xyz\" (the yardstick) and against the composition, %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds x %d calls, alternated, HIP events" % (ROUNDS, CALLS)]
    for B, N, K, augment, sort, per_point, S, what in SIZES:
        if not sort:
            continue
        data, labels, perm = resident_set(B, N, K, per_point, S, dev)
        bufs = {m: [provider.BatchBuffers(B, N, K, per_point, dev, True, sort_method=m) for _ in range(2)]
                for m in provider.SORT_METHODS}
        step = [0]

        def fused(method):
            step[0] += 1
            return provider.assemble_batch(data, labels, B, perm=perm, start=(step[0] * B) % (S - B + 1), rotate=augment,
                                           jitter=augment, sort_cloud=True, seed=1, step=step[0],
                                           out=bufs[method][step[0] & 1], sort_method=method)

        def comp():
            step[0] += 1
            return composition(data, labels, perm, (step[0] * B) % (S - B + 1), B, augment, True, prestep.sort_order_morton)
        calls = (lambda: fused("xyz"), lambda: fused("morton"), comp)
        for _ in range(5):
            for fn in calls:
                fn()
        torch.cuda.synchronize()
        t = [[], [], []]
        for _ in range(ROUNDS):
            for k, fn in enumerate(calls):
                t[k].append(timed(fn))
        flags = (3 if augment else 0) | _lib.PROVIDER_SORT
        tx = bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags, bufs["xyz"][0], stream)
        tm = bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags | _lib.PROVIDER_MORTON, bufs["morton"][0], stream)
        row = lambda v, f="%8.1f": "  ".join(f % x for x in v)
        lines.append("")
        lines.append("B x N x K = %d x %d x %d  (%s)" % (B, N, K, what.replace("sort", "sort (morton)")))
        lines.append("  fused xyz     (1 launch)        " + row(t[0]))
        lines.append("  fused morton  (1 launch)        " + row(t[1]))
        lines.append("  composition   (morton)          " + row(t[2]))
        lines.append("  ratio xyz / morton              " + row([x / m for x, m in zip(t[0], t[1])], "%8.2f"))
        lines.append("  ratio composition / morton      " + row([c / m for c, m in zip(t[2], t[1])], "%8.2f"))
        lines.append("  the C call alone, %d back to back, 3 rounds: xyz " % BARE + "  ".join("%.1f" % v for v in tx)
                     + " us;  morton " + "  ".join("%.1f" % v for v in tm) + " us")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


# beyond the one-launch call's limit: B, N, K, labels per point, samples in the resident set
LARGE = ((4, 65536, 9, True, 8), (16, 20000, 3, False, 32))
ROW = lambda v, f="%8.1f": "  ".join(f % x for x in v)


def torch_order_xyz(rows):
    """util.py:66-68 as a user would write it in torch: argsort by z, then stable by y, then stable by x."""
    B = rows.shape[0]
    ar = torch.arange(B, device=rows.device)[:, None]
    order = torch.argsort(rows[:, :, 2], dim=1, stable=True)
    order = order[ar, torch.argsort(rows[:, :, 1][ar, order], dim=1, stable=True)]
    return order[ar, torch.argsort(rows[:, :, 0][ar, order], dim=1, stable=True)]


def torch_composition(data, labels, perm, start, B):
    idx = perm[start:start + B].long()
    rows, lab = data[idx], labels[idx]
    order = torch_order_xyz(rows)
    rows = torch.gather(rows, 1, order[:, :, None].expand(-1, -1, rows.shape[2]))
    if lab.dim() == 2:
        lab = torch.gather(lab, 1, order)
    return rows[:, :, 0:3].contiguous(), rows, lab.to(torch.int32)


def alternated(calls):
    for _ in range(5):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in calls]
    for _ in range(ROUNDS):
        for k, fn in enumerate(calls):
            t[k].append(timed(fn))
    return t


def finish(lines, out_path, append):
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write(("\n" if append else "") + text)


def main_wide(out_path, note, append):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["wide batch provider (wide_sort=True, several launches) against the one-launch call (the yardstick) and the "
             "composition, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds x %d calls, alternated, HIP events" % (ROUNDS, CALLS)]
    if note:
        lines.append(note)
    for B, N, K, augment, sort, per_point, S, what in SIZES:
        if not sort:
            continue
        data, labels, perm = resident_set(B, N, K, per_point, S, dev)
        for method in provider.SORT_METHODS:
            bufs = {w: [provider.BatchBuffers(B, N, K, per_point, dev, True, sort_method=method, wide_sort=w)
                        for _ in range(2)] for w in (False, True)}
            step = [0]

            def fused(wide):
                step[0] += 1
                return provider.assemble_batch(data, labels, B, perm=perm, start=(step[0] * B) % (S - B + 1), rotate=augment,
                                               jitter=augment, sort_cloud=True, seed=1, step=step[0],
                                               out=bufs[wide][step[0] & 1], sort_method=method, wide_sort=wide)

            def comp():
                step[0] += 1
                return composition(data, labels, perm, (step[0] * B) % (S - B + 1), B, augment, True,
                                   prestep.sort_order_morton if method == "morton" else prestep.sort_order_xyz)
            t = alternated((lambda: fused(False), lambda: fused(True), comp))
            flags = (3 if augment else 0) | _lib.PROVIDER_SORT | (_lib.PROVIDER_MORTON if method == "morton" else 0)
            t1 = bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags, bufs[False][0], stream)
            tw = bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags, bufs[True][0], stream,
                           "conv3p_provider_batch_wide_f32")
            lines.append("")
            lines.append("B x N x K = %d x %d x %d  (%s), sort_method=%s" % (B, N, K, what, method))
            lines.append("  one launch                      " + ROW(t[0]))
            lines.append("  wide                            " + ROW(t[1]))
            lines.append("  composition                     " + ROW(t[2]))
            lines.append("  ratio one launch / wide         " + ROW([x / m for x, m in zip(t[0], t[1])], "%8.2f"))
            lines.append("  ratio composition / wide        " + ROW([c / m for c, m in zip(t[2], t[1])], "%8.2f"))
            lines.append("  the C call alone, %d back to back, 3 rounds: one launch " % BARE + "  ".join("%.1f" % v for v in t1)
                         + " us;  wide " + "  ".join("%.1f" % v for v in tw) + " us")
    for B, N, K, per_point, S in LARGE:
        data, labels, perm = resident_set(B, N, K, per_point, S, dev)
        nbytes = (4 * K + 12 + (1 if per_point else 0)) * 2 * B * N
        step = [0]

        def torch_comp():
            step[0] += 1
            return torch_composition(data, labels, perm, (step[0] * B) % (S - B + 1), B)
        for method in provider.SORT_METHODS:
            bufs = [provider.BatchBuffers(B, N, K, per_point, dev, True, sort_method=method, wide_sort=True) for _ in range(2)]

            def wide():
                step[0] += 1
                return provider.assemble_batch(data, labels, B, perm=perm, start=(step[0] * B) % (S - B + 1), sort_cloud=True,
                                               seed=1, step=step[0], out=bufs[step[0] & 1], sort_method=method, wide_sort=True)
            t = alternated((wide, torch_comp) if method == "xyz" else (wide,))
            flags = _lib.PROVIDER_SORT | (_lib.PROVIDER_MORTON if method == "morton" else 0)
            tw = bare_call(lib, data, labels, perm, S, N, K, B, per_point, flags, bufs[0], stream,
                           "conv3p_provider_batch_wide_f32")
            lines.append("")
            lines.append("B x N x K = %d x %d x %d  (sort only; no one-launch call at this N), sort_method=%s" % (B, N, K, method))
            lines.append("  wide                            " + ROW(t[0]))
            if method == "xyz":
                lines.append("  torch: 3 stable argsorts + gathers (orientation)  " + ROW(t[1]))
            lines.append("  the C call alone, %d back to back, 3 rounds: " % BARE + "  ".join("%.1f" % v for v in tw) + " us")
            lines.append("  (4 K + 12 + label bytes) * 2 per point = %.2f MB: " % (nbytes / 1e6)
                         + "  ".join("%.0f" % (nbytes / (v * 1e-6) / 1e9) for v in tw) + " GB/s")
    finish(lines, out_path, append)


def main_wide_sort(out_path, note, append):
    dev = torch.device("cuda:0")
    lines = ["the sort alone: prestep.sort_order (several launches) against prestep.sort_order_xyz / _morton (one launch), %s"
             % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds x %d calls, alternated, HIP events" % (ROUNDS, CALLS)]
    if note:
        lines.append(note)
    shapes = [(B, N, K) for B, N, K, _, sort, _, _, _ in SIZES if sort] + [(B, N, K) for B, N, K, _, _ in LARGE]
    for B, N, K in shapes:
        x = torch.rand(B, N, K, generator=torch.Generator(device="cpu").manual_seed(B + N + K)).to(dev)
        ws = {m: torch.empty(_lib.load().conv3p_sort_order_workspace_bytes(B, N, prestep.SORT_METHODS[m]), dtype=torch.uint8,
                             device=dev) for m in provider.SORT_METHODS}
        old = {"xyz": prestep.sort_order_xyz, "morton": prestep.sort_order_morton}
        for method in provider.SORT_METHODS:
            wide = lambda: prestep.sort_order(x, method, workspace=ws[method])
            if N <= 8192:
                t = alternated((lambda: old[method](x), wide))
                names = ("one launch", "wide")
            elif method == "xyz":
                t = alternated((lambda: torch_order_xyz(x), wide))
                names = ("torch: 3 stable argsorts (orientation)", "wide")
            else:
                t = alternated((wide,))
                names = ("wide",)
            lines.append("")
            lines.append("B x N x K = %d x %d x %d, sort_method=%s" % (B, N, K, method))
            for n, v in zip(names, t):
                lines.append("  %-40s" % n + ROW(v))
            if len(t) == 2:
                lines.append("  %-40s" % ("ratio " + names[0].split(":")[0] + " / wide") + ROW([a / b for a, b in zip(*t)], "%8.2f"))
    finish(lines, out_path, append)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--morton", action="store_true", help="time sort_method=\"morton\" on the sorted shapes")
    ap.add_argument("--wide", action="store_true", help="time wide_sort=True against the one-launch call")
    ap.add_argument("--wide-sort", action="store_true", help="time prestep.sort_order against the one-launch sorts")
    ap.add_argument("--note", default="", help="a line for the header of the --wide / --wide-sort output")
    ap.add_argument("--append", action="store_true", help="--wide / --wide-sort: append to the output file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "wide_sort_time.txt" if args.wide or args.wide_sort else \
            "provider_morton_time.txt" if args.morton else "provider_time.txt"
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", name)
    if not torch.cuda.is_available():
        raise SystemExit("provider_time: needs a HIP device")
    if args.wide:
        return main_wide(args.out, args.note, args.append)
    if args.wide_sort:
        return main_wide_sort(args.out, args.note, args.append)
    if args.morton:
        return main_morton(args.out)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = ["fused batch provider (one launch) vs the composition it replaces, %s" % torch.cuda.get_device_name(dev),
             "us per call including Python; %d rounds x %d calls, alternated, HIP events; ratio = composition / fused per round"
             % (ROUNDS, CALLS)]
    for B, N, K, augment, sort, per_point, S, what in SIZES:
        data, labels, perm = resident_set(B, N, K, per_point, S, dev)
        bufs = [provider.BatchBuffers(B, N, K, per_point, dev, sort) for _ in range(2)]
        step = [0]

        def fused():
            step[0] += 1
            return provider.assemble_batch(data, labels, B, perm=perm, start=(step[0] * B) % (S - B + 1), rotate=augment,
                                           jitter=augment, sort_cloud=sort, seed=1, step=step[0], out=bufs[step[0] & 1])

        def comp():
            step[0] += 1
            return composition(data, labels, perm, (step[0] * B) % (S - B + 1), B, augment, sort)
        for _ in range(5):
            fused(), comp()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(fused))
            tc.append(timed(comp))
        tb = bare_call(lib, data, labels, perm, S, N, K, B, per_point, (3 if augment else 0) | (4 if sort else 0), bufs[0],
                       torch.cuda.current_stream(dev).cuda_stream)
        lines.append("")
        lines.append("B x N x K = %d x %d x %d  (%s)" % (B, N, K, what))
        lines.append("  fused  (1 launch)          " + "  ".join("%8.1f" % v for v in tf))
        lines.append("  composition                " + "  ".join("%8.1f" % v for v in tc))
        lines.append("  ratio composition / fused  " + "  ".join("%8.2f" % (c / f) for f, c in zip(tf, tc)))
        lines.append("  the C call alone, %d back to back, 3 rounds: " % BARE + "  ".join("%.1f" % v for v in tb) + " us")
        if B * N >= 16 * 8192:
            nbytes = (4 * K + 12 + (1 if per_point else 0)) * 2 * B * N
            lines.append("  (4 K + 12 + label bytes) * 2 per point = %.2f MB: " % (nbytes / 1e6)
                         + "  ".join("%.0f" % (nbytes / (v * 1e-6) / 1e9) for v in tb) + " GB/s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
