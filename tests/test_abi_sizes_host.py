"""CPU test (not gpu) of every size the C ABI reports: each `*_workspace_bytes` export, conv3p_cache_bytes and
conv3p_stack_scratch_bytes over the fixed table of arguments below -- the refusals (0), the smallest accepted arguments,
both sides of every branch of the layouts, and a value near each documented limit -- against tests/golden/abi_sizes.json.

The golden values were written by evaluate() on the library of the commit BEFORE the layouts were rewritten as single
walks (one function per workspace serving as both its size and its pointers), so the test pins that the rewrite, and
any later change to a layout function, leaves every size a caller allocates by unchanged.  A deliberate change of a
layout regenerates the file with write_golden() and says so."""
import ctypes
import itertools
import json
import math
import os

import pytest

from pointwise_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_sizes.json")
NAN = float("nan")
I31 = 2 ** 31 - 1


def _conv3p_workspace():
    rows = [(3, 4, 2, 1024, 3, 9, 3, 3, 3), (0, 2, 2, 1024, 3, 9, 3, 3, 3), (0, 4, -1, 1024, 3, 9, 3, 3, 3),
            (0, 4, 2, -1, 3, 9, 3, 3, 3), (0, 4, 2, 1024, 3, 9, 0, 3, 3), (0, 4, 2, 1024, -1, 9, 3, 3, 3),
            (1, 8, 2, 1024, 3, -1, 3, 3, 3), (0, 4, 2, 1024, 3, 9, 16, 16, 16), (0, 4, 2, 1024, 3, 9, 1, 1, 4097),
            (0, 4, 0, 0, 0, 0, 1, 1, 1), (1, 8, 0, 0, 0, 0, 1, 1, 1), (2, 4, 0, 0, 0, 0, 1, 1, 1),
            (2, 4, 1, 1, -1, -1, 1, 1, 1), (2, 8, 4, 1000, 0, 0, 3, 3, 3), (2, 4, 2, 16385, 0, 0, 5, 5, 5)]
    # register path (3 -> 9, 9 -> 9, 36 -> 13: fp32 transform + gather, fp64 three column passes), matrix core (padded
    # classes, 128 -> 256), more than 256 channels on either side and on both, fp64 blocks, the generic kernels
    shapes = [(3, 9), (9, 9), (36, 13), (5, 7), (20, 20), (64, 64), (100, 33), (128, 256), (300, 64), (64, 300),
              (512, 512), (0, 9), (9, 0)]
    for (cin, cout), pas, elem in itertools.product(shapes, (0, 1), (4, 8)):
        rows.append((pas, elem, 2, 1024, cin, cout, 3, 3, 3))
    for pas, elem in itertools.product((0, 1), (4, 8)):
        rows += [(pas, elem, 1, 1, 3, 9, 1, 1, 1),              # one point, one tap
                 (pas, elem, 9, 64, 9, 9, 3, 3, 3),             # one tile a cloud, two rounds of clouds
                 (pas, elem, 3, 16384, 9, 9, 3, 3, 3),          # with the fused search's tables ...
                 (pas, elem, 3, 16385, 9, 9, 3, 3, 3),          # ... and without
                 (pas, elem, 2, 1000, 9, 9, 5, 5, 5),           # 125 taps: past the 64-bit tap sets
                 (pas, elem, 2, 1000, 64, 64, 5, 5, 5),
                 (pas, elem, 2, 1000, 36, 13, 3, 3, 4),         # 36 taps
                 (pas, elem, 2, 1000, 16, 8, 1, 7, 9),
                 (pas, elem, 16, 65536, 256, 256, 3, 3, 3),     # large
                 (pas, elem, 4, 8192, 1024, 300, 3, 3, 3)]
    return rows


def _cache():
    ok = (1, 27, 0, 9, 9, 0)
    rows = [(2, 2, 1024, ok), (4, -1, 1024, ok), (4, 2, -1, ok), (4, 2, 1024, None), (4, 2, 1024, (0, 27, 0, 9, 9, 0)),
            (4, 2, 1024, (65, 27, 0, 9, 9, 0)), (4, 2, 1024, (1, 0, 0, 9, 9, 0)), (4, 2, 1024, (1, 4095, 0, 9, 9, 0)),
            (4, 2, 1024, (1, 27, 0, -1, 9, 0)), (4, 2, 1024, (1, 27, 0, 9, -1, 0)),
            (4, 0, 0, (1, 1, 0, 0, 0, 0)), (8, 0, 0, (1, 1, 0, 0, 0, 0)), (4, 1, 1, (1, 1, 0, 0, 0, 0))]
    chans = [(0, 0), (9, 9), (36, 13), (64, 64), (128, 256), (300, 64), (512, 512)]
    for (ci, co), elem in itertools.product(chans, (4, 8)):
        rows.append((elem, 2, 1024, (4, 27, 0, ci, co, 0)))
    for elem in (4, 8):
        rows += [(elem, 2, 1024, (64, 27, 0, 9, 9, 0)), (elem, 2, 1024, (4, 125, 0, 36, 13, 0)),
                 (elem, 2, 1024, (4, 27, 64, 64, 64, 0)), (elem, 2, 1024, (4, 27, 1, 64, 64, 64)),
                 (elem, 3, 16384, (4, 27, 0, 36, 13, 7)), (elem, 3, 16385, (4, 27, 0, 36, 13, 0)),
                 (elem, 9, 64, (2, 33, 300, 13, 36, 0)), (elem, 16, 65536, (8, 64, 256, 256, 256, 0)),
                 (elem, 1, 100000, (1, 4094, 0, 3, 9, 0))]
    return rows


def _stack():
    s1, s4 = [(1, 1, 1)], [(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4), (1, 1, 1)]
    s9 = [(1, 1, 1)] * 9
    ok = (4, 3, 9, 13, 3, 3, 3, s4)
    rows = [(None, 4, 2, 1024), (ok, 2, 2, 1024), (ok, 4, -1, 1024), (ok, 4, 2, -1),
            ((0, 3, 9, 13, 3, 3, 3, s4), 4, 2, 1024), ((9, 3, 9, 13, 3, 3, 3, s9), 4, 2, 1024),
            ((4, 0, 9, 13, 3, 3, 3, s4), 4, 2, 1024), ((4, 3, 0, 13, 3, 3, 3, s4), 4, 2, 1024),
            ((4, 3, 9, -1, 3, 3, 3, s4), 4, 2, 1024), ((4, 3, 9, 13, 0, 3, 3, s4), 4, 2, 1024),
            ((4, 3, 9, 13, 3, 3, 3, s4[:4] + [(1, 0, 1)]), 4, 2, 1024),
            ((4, 3, 9, 0, 3, 3, 3, s4[:4] + [(1, 0, 1)]), 4, 2, 1024),        # no head: its strides are not read
            (ok, 4, 0, 0), (ok, 8, 0, 1024), ((1, 1, 1, 0, 1, 1, 1, s1), 4, 1, 1), ((1, 1, 1, 0, 1, 1, 1, s1), 8, 1, 1)]
    for elem in (4, 8):
        rows += [(ok, elem, 2, 1024), (ok, elem, 9, 64), (ok, elem, 3, 1000), ((4, 9, 9, 0, 3, 3, 3, s4), elem, 2, 1024),
                 ((2, 3, 9, 40, 3, 3, 3, s4), elem, 2, 1024),                 # the head wider than the hidden layers
                 ((4, 6, 12, 13, 5, 5, 5, s4), elem, 2, 1024), ((8, 3, 64, 40, 3, 3, 3, s9), elem, 16, 8192),
                 ((8, 9, 9, 13, 1, 7, 9, s9), elem, 7, 16385)]
    return rows


def _scene():
    ratios = [(1.0, 1.0), (1.5, 1.0), (2.0, 1.0), (0.75, 0.5)]
    rows = [(0, 4096, 100, 1.0, 1.0), (-1, 4096, 100, 1.0, 1.0), (2 ** 24 + 1, 4096, 100, 1.0, 1.0),
            (1000, 0, 100, 1.0, 1.0), (1000, 65537, 100, 1.0, 1.0), (1000, 4096, 0, 1.0, 1.0), (1000, 4096, -1, 1.0, 1.0),
            (1000, 4096, 100, 0.5, 1.0), (1000, 4096, 100, 2.5, 1.0), (1000, 4096, 100, NAN, 1.0),
            (1000, 4096, 100, 1.0, NAN), (1000, 4096, 100, 1.0, 0.0), (1000, 4096, 100, 0.0, 0.0),
            (1000, 4096, 100, -1.0, -1.0), (1, 1, 1, 1.0, 1.0)]
    for (block, stride), mb in itertools.product(ratios, (100, 65535, 65536, 65537, 1000000)):
        rows.append((100000, 4096, mb, block, stride))
    for n in (1, 255, 256, 257, 65536, 65537, 1 << 20, (1 << 20) + 1, 3000000):
        rows.append((n, 4096, 1000, 1.5, 1.0))
    rows += [(2 ** 24, 65536, I31, 2.0, 1.0), (2 ** 24, 1, 1, 1.0, 1.0)]
    return rows


def _rooms():
    rows = [(1000, 3, 4096, 100, 1.0, 1.0, 2), (1000, 3, 4096, 100, 1.0, 1.0, -1), (1000, 0, 4096, 100, 1.0, 1.0, 0),
            (1000, 65537, 4096, 100, 1.0, 1.0, 0), (0, 3, 4096, 100, 1.0, 1.0, 0), (2 ** 26 + 1, 3, 4096, 100, 1.0, 1.0, 0),
            (1000, 3, 0, 100, 1.0, 1.0, 0), (1000, 3, 65537, 100, 1.0, 1.0, 0), (1000, 3, 4096, 0, 1.0, 1.0, 0),
            (1000, 3, 4096, 100, 0.5, 1.0, 0), (1000, 3, 4096, 100, 2.5, 1.0, 0), (1000, 3, 4096, 100, NAN, 1.0, 0),
            (1000, 3, 4096, 100, 1.0, 0.0, 1), (1, 1, 1, 1, 1.0, 1.0, 0), (1, 1, 1, 1, 1.0, 1.0, 1)]
    for (block, stride), mb, cover in itertools.product([(1.0, 1.0), (1.5, 1.0), (2.0, 1.0)],
                                                        (100, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 5000000), (0, 1)):
        rows.append((100000, 7, 4096, mb, block, stride, cover))
    for n, r in [(1, 1), (255, 2), (256, 2), (257, 300), (2047, 1), (2048, 1), (2049, 1), (500000, 65536)]:
        rows.append((n, r, 4096, 1000, 1.5, 1.0, 0))
    rows += [(2 ** 26, 65536, 65536, I31, 2.0, 1.0, 1), (2 ** 26, 1, 1, 1, 1.0, 1.0, 0)]
    return rows


def _labels(max_class):
    return [(0, 13), (-1, 13), (2 ** 31, 13), (1000, 0), (1000, -1), (1000, max_class + 1), (1, 1), (1000, 13),
            (65536, 2), (I31, max_class)]


def _grid():
    rows = [(0, 100), (-1, 100), (2 ** 24 + 1, 100), (1000, 0), (1000, -1), (1, 1)]
    for n in (1, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 100000, 2 ** 24):
        rows += [(n, 1), (n, max(1, n // 3)), (n, n), (n, n + 1), (n, 4 * n)]      # N above, at and below max_voxels
    rows += [(1000, I31), (2 ** 24, I31)]
    return list(dict.fromkeys(rows))


def _grid_rooms():
    rows = [(1000, 0, 100), (1000, -1, 100), (1000, 65537, 100), (0, 3, 100), (2 ** 24 + 1, 3, 100), (1000, 3, 0), (1, 1, 1)]
    for n, r in itertools.product((1, 256, 257, 1000, 4097, 100000, 2 ** 24), (1, 5, 65536)):
        rows += [(n, r, max(1, n // 3)), (n, r, n + 1)]
    rows.append((2 ** 24, 65536, I31))
    return list(dict.fromkeys(rows))


def _rows_only():
    return [(-1,), (0,), (2 ** 31,), (2 ** 40,), (1,), (2,), (1023,), (1024,), (1025,), (4096,), (4097,), (1000000,), (I31,)]


def _wide(flag_sets):
    rows = [(0, 1000, flag_sets[0]), (-1, 1000, flag_sets[0]), (3, 0, flag_sets[0]), (3, 65537, flag_sets[0])]
    for n, b, f in itertools.product((1, 64, 65, 1000, 8192, 8193, 65535, 65536), (1, 3), flag_sets):
        rows.append((b, n, f))
    rows.append((32767, 65536, flag_sets[-1]))
    return rows


def _seg():
    return [(0, 13), (1000, 1), (1000, 0), (1000, 129), (1, 2), (64, 2), (65, 13), (1000, 13), (65536, 13), (65537, 13),
            (64 * 1024, 41), (64 * 1024 + 1, 41), (1 << 20, 128), (1 << 40, 128), (1 << 62, 2)]


TABLE = {
    "conv3p_workspace_bytes": _conv3p_workspace(),
    "conv3p_cache_bytes": _cache(),
    "conv3p_stack_scratch_bytes": _stack(),
    "conv3p_provider_workspace_bytes": [(0, 1000, 4), (-1, 1000, 4), (3, 0, 4), (3, 1000, 0), (3, 1000, 3), (3, 1000, 8),
                                        (3, 8193, 4), (1, 1, 4), (3, 1000, 4), (3, 1000, 12), (3, 1000, 15), (16, 8192, 4),
                                        (100000, 8192, 12)],
    "conv3p_sort_order_workspace_bytes": _wide([0, 1]) + [(3, 1000, 2), (3, 1000, -1)],
    "conv3p_provider_wide_workspace_bytes": _wide([4, 12]) + [(3, 1000, 0), (3, 1000, 8), (3, 1000, 3), (3, 1000, 15)],
    "conv3p_scene_blocks_workspace_bytes": _scene(),
    "conv3p_scene_blocks_cover_workspace_bytes": _scene(),
    "conv3p_scene_blocks_rooms_workspace_bytes": _rooms(),
    "conv3p_scene_vote_labels_workspace_bytes": _labels(128),
    "conv3p_scene_score_labels_workspace_bytes": _labels(128),
    "conv3p_grid_subsample_workspace_bytes": _grid(),
    "conv3p_grid_subsample_rooms_workspace_bytes": _grid_rooms(),
    "conv3p_grid_interpolate_rings_workspace_bytes": _rows_only(),
    "conv3p_grid_segments_workspace_bytes": _rows_only(),
    "conv3p_grid_absorb_workspace_bytes": _rows_only(),
    "conv3p_fc_workspace_bytes": [(0, 100, 8), (129, 100, 8), (4, 0, 8), (4, 100, 0), (4, 100, 12), (4, 100, 1032),
                                  (-1, 100, 8), (1, 1, 8), (4, 10, 8), (32, 8192, 64), (33, 8193, 64), (64, 16384, 256),
                                  (128, 73728, 256), (1, 73728, 1024), (128, 122880, 1024), (128, 122881, 8),
                                  (128, 10000000, 1024)],
    "conv3p_seg_head_workspace_bytes": _seg(),
    "conv3p_seg_head_weighted_workspace_bytes": _seg(),
    "conv3p_seg_confusion_workspace_bytes": _seg(),
    "conv3p_grad_norm_workspace_bytes": [()],
    "conv3p_cls_tail_workspace_bytes": [(0, 256, 40), (129, 256, 40), (32, 4, 40), (32, 12, 40), (32, 0, 40), (32, 1032, 40),
                                        (32, 256, 1), (32, 256, 129), (-1, 256, 40), (1, 8, 2), (32, 256, 40), (33, 264, 41),
                                        (128, 1024, 128), (64, 8, 128), (7, 1024, 2)],
}


def _call(lib, name, args):
    if name == "conv3p_cache_bytes":
        cfg = None if args[3] is None else ctypes.byref(_lib.CacheConfig(*args[3]))
        return lib.conv3p_cache_bytes(args[0], args[1], args[2], cfg)
    if name == "conv3p_stack_scratch_bytes":
        desc = None
        if args[0] is not None:
            sd = _lib.StackDesc(*args[0][:7])
            for l, st in enumerate(args[0][7]):
                for a in range(3):
                    sd.strides[l][a] = st[a]
            desc = ctypes.byref(sd)
        return lib.conv3p_stack_scratch_bytes(desc, *args[1:])
    return getattr(lib, name)(*args)


def _plain(x):
    """Arguments as JSON holds them: tuples as lists, NaN by name."""
    if isinstance(x, (tuple, list)):
        return [_plain(v) for v in x]
    return "nan" if isinstance(x, float) and math.isnan(x) else x


def evaluate(lib):
    return {name: [{"args": _plain(args), "bytes": int(_call(lib, name, args))} for args in rows]
            for name, rows in TABLE.items()}


def write_golden(lib, path=GOLDEN):
    got = evaluate(lib)
    with open(path, "w") as fh:   # a row a line
        fh.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(r, sort_keys=True) for r in got[name]))
                                    for name in sorted(got)) + "\n}\n")


def test_the_table_covers_every_size_export():
    sizes = {n for n in _lib.SYMBOLS if n.endswith("_workspace_bytes")} | {"conv3p_cache_bytes", "conv3p_stack_scratch_bytes"}
    assert sizes == set(TABLE)
    for name, rows in TABLE.items():
        assert len(rows) == len({json.dumps(_plain(r)) for r in rows}), name      # no row twice


@pytest.mark.parametrize("name", sorted(TABLE))
def test_sizes_are_those_recorded(name):
    with open(GOLDEN) as fh:
        golden = json.load(fh)[name]
    got = evaluate_one(name)
    assert [g["args"] for g in golden] == [g["args"] for g in got]               # the file is this table's
    wrong = [(g["args"], g["bytes"], w["bytes"]) for g, w in zip(golden, got) if g["bytes"] != w["bytes"]]
    assert not wrong, "%s: (args, recorded, now) %r" % (name, wrong[:8])
    # the rows do what they are there for: some refuse, some accept, and every accepted size keeps the alignment
    assert all(w["bytes"] % 256 == 0 for w in got)
    if name != "conv3p_grad_norm_workspace_bytes":
        assert any(w["bytes"] == 0 for w in got) and any(w["bytes"] > 0 for w in got)


def evaluate_one(name):
    lib = _lib.load()
    return [{"args": _plain(args), "bytes": int(_call(lib, name, args))} for args in TABLE[name]]
