"""The stream-contract cases of include/conv3p_match.h: the table of tests/stream_contract_cases.py continued for the header
of the segment matching, with the same Entry and the same builders, as tests/stream_contract_knn_cases.py continues it for
conv3p_knn.h.  It keeps a list of its own -- the main table, and the CPU test that pins it to conv3p.h and to
pointwise_amd.__all__, stay as they are.  The header's functions carry the prefix c3p_, so the scan of its declarations
has its own regular expression.  Importing this module does not touch the device."""
import os
import re

import torch

from tests import stream_contract_cases as main
from tests.stream_rig import Case

ENTRIES = []
HEADER = os.path.join(os.path.dirname(main.HEADER), "conv3p_match.h")
MATCH_OUT = ("pred_size", "pred_void", "truth_size", "truth_missed", "pair_pred", "pair_truth", "pair_inter", "start", "t_start",
             "t_pair", "best_truth", "best_truth_inter", "best_truth_union", "best_pred", "best_pred_inter", "best_pred_union",
             "pred_match", "truth_match", "pred_iou_q30", "class_stats", "stats")


def streamed_functions():
    """Every function include/conv3p_match.h declares with a `void *stream` parameter."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {name for name, params in re.findall(r"\b(c3p_\w+)\s*\(([^;{}()]*)\)\s*;", text)
            if re.search(r"void\s*\*\s*stream\b", params)}


def _add(name, make_run, rooms=False, seed=9300):
    """main._add_grid for this table: make_run(dev, a, b) -> (run, further (input, poison) pairs), a and b the (raw data, raw
    labels, g) of the two halves; the poison is another seed's room of the same shapes."""
    def build(dev, real, poison):
        a, b = main._grid_pair(dev, real, poison, rooms)
        run, more = make_run(dev, a, b)
        inputs = [a[0]] + main._grid_state(a[2]) + [x for x, _ in more]
        bad = [b[0]] + main._grid_state(b[2]) + [p for _, p in more]
        return Case(inputs, bad, run, lambda: None)
    ENTRIES.append(main.Entry(name, main.two(main._room_arrays, seed), build, frozenset(["c3p_grid_match_segments"])))


def _run_match(weight, classes):
    def make(dev, a, b):
        sa, sb, more = main._segmentations(a, b)
        # the instance of a row is its raw label, of a voxel its slab: ids in [0, NCLS), a truth as good as any
        ta, tb = (a[1], b[1]) if weight == "rows" else (more[0][0], more[0][1])
        more = more + ([(a[1], b[1])] if weight == "rows" else [])
        kw = {}
        if classes:
            tc = torch.arange(main.NCLS, dtype=torch.int32).to(dev)
            kw = dict(pred_class=sa.label, truth_class=tc, num_class=main.NCLS)
            more = more + [(tc, ((tc + 1) % main.NCLS).contiguous())]

        def run():
            return main.tensors(sa.match(ta, main.NCLS, weight=weight, max_pairs=4 * sa.shape[0], **kw), MATCH_OUT)
        return run, more
    return make


_add("GridSegments.match/rows, classes", _run_match("rows", True))
_add("GridSegments.match/voxels", _run_match("voxels", False))
_add("GridSegments.match/rows, many clouds", _run_match("rows", False), rooms=True)
NAMES = [e.name for e in ENTRIES]
