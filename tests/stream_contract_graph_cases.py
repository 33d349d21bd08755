"""The stream-contract cases of include/conv3p_graph.h: the table of tests/stream_contract_cases.py continued for the header
that stands beside conv3p.h, with the same Entry and the same builders.  It keeps a list of its own -- the main table, and
the CPU test that pins it to conv3p.h and to pointwise_amd.__all__, stay as they are.  Importing this module does not touch
the device."""
import os

from tests import stream_contract_cases as main
from tests.stream_rig import Case

ENTRIES = []
HEADER = os.path.join(os.path.dirname(main.HEADER), "conv3p_graph.h")
AGG_IN = ("start", "src", "dst", "contacts", "offset", "stats")
AGG_OUT = ("voxel_label", "log_a", "log_b", "log_round", "log_contacts", "start", "src", "dst", "contacts", "offset", "twin", "stats")


def streamed_functions():
    """Every function include/conv3p_graph.h declares with a `void *stream` parameter."""
    return main.streamed_functions(HEADER)


def _agglomerate(dev, real, poison):
    """SegmentAdjacency.agglomerate on a segmentation and its adjacency made in build(); the poison is those of another
    seed's room and labels: another segmentation and another graph of the same M and max_edges, every number in range."""
    a, b = main._grid_pair(dev, real, poison)
    sa, sb, more = main._segmentations(a, b)
    adj = [s.adjacency(max_edges=8 * s.shape[0]) for s in (sa, sb)]
    assert not adj[0].overflowed() and not adj[1].overflowed() and adj[0].shape == adj[1].shape
    more = more + list(zip(main.tensors(adj[0], AGG_IN), main.tensors(adj[1], AGG_IN)))

    def run():
        res = adj[0].agglomerate(8)
        return main.tensors(res.segments, main.SEG_STATE + ("seg_map", "merge_stats")) + main.tensors(res, AGG_OUT)
    inputs = [a[0]] + main._grid_state(a[2]) + [x for x, _ in more]
    bad = [b[0]] + main._grid_state(b[2]) + [p for _, p in more]
    return Case(inputs, bad, run, lambda: None)


ENTRIES.append(main.Entry("SegmentAdjacency.agglomerate", main.two(main._room_arrays, 8900), _agglomerate,
                          frozenset(["conv3p_grid_agglomerate_segments"])))
NAMES = [e.name for e in ENTRIES]
