"""GPU tests (-m gpu) of the segment matching, GridSegments.match on c3p_grid_match_segments: every output bit for bit
(np.array_equal, no tolerance) against tests/grid_match_ref.py, for both weights, into outputs prefilled with garbage --
unit counts around a wave and a workgroup, one hot pair, every unit its own pair at P == max_pairs and one past it (M5,
then the retry), the edge inputs, rows of the table the whole wave walks, ties, three thresholds, classes given and
omitted, out= reuse, segmentations the pipeline made (plain, merged, agglomerated, two rooms), reproducibility."""
import functools

import numpy as np
import pytest

from tests import grid_match_cases as mc
from tests import grid_match_ref as mr

pytestmark = pytest.mark.gpu
WEIGHTS = ("rows", "voxels")
IOUS = ((1, 2), (3, 4), (9, 10))


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def on_device(c):
    """A case as the objects match() reads: a GridSubsample and a GridSegments with the case's arrays in them."""
    import torch
    from pointwise_amd import grid
    dev = _dev()
    M, N = c["segment"].shape[0], c["inverse"].shape[0]
    g = grid.GridSubsample(N, M, 3, False, dev)
    g.inverse.copy_(torch.from_numpy(c["inverse"]))
    g.stats.copy_(torch.tensor([c["emitted"], c["emitted"], 0, 0, 0, 0, 0, 0], dtype=torch.int32))
    seg = grid.GridSegments(M, dev)
    seg.segment.copy_(torch.from_numpy(c["segment"]))
    seg.stats.copy_(torch.tensor([c["S"], 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32))
    seg._source = (g, None, 0, None, 26)
    return g, seg


def garbage(M, T, max_pairs, num_class):
    """A SegmentMatch whose every word is set to something the call never leaves there."""
    from pointwise_amd import grid
    out = grid.SegmentMatch(M, T, max_pairs, num_class, _dev())
    for name in mr.OUTPUTS:
        getattr(out, name).fill_(-(1 << 40) if name in ("class_stats", "stats") else 0x5a5a5a5a)
    return out


def same(got, ref, what):
    for name in mr.OUTPUTS:
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == ref[name].dtype and a.shape == ref[name].shape, "%s: %s" % (what, name)
        assert np.array_equal(a, ref[name]), "%s: %s\n%s\n%s" % (what, name, a, ref[name])


def run(c, weight, iou=(1, 2), max_pairs=None, objects=None, out=None, classes=True):
    """match() on the case and the reference on the same arrays -> (the result, the reference)."""
    import torch
    dev = _dev()
    g, seg = objects or on_device(c)
    M, T = c["segment"].shape[0], c["T"]
    use = classes and c["pred_class"] is not None
    kw = {}
    if use:
        kw = dict(pred_class=torch.from_numpy(c["pred_class"]).to(dev), truth_class=torch.from_numpy(c["truth_class"]).to(dev),
                  num_class=c["num_class"])
    truth = mc.truth_of(c, weight)
    mp = M if max_pairs is None else max_pairs
    if out is None:
        out = garbage(M, T, mp, c["num_class"] if use else 1)
    got = seg.match(torch.from_numpy(truth).to(dev), T, weight=weight, iou=iou, max_pairs=max_pairs, out=out, **kw)
    assert got is out
    ref = mr.match_ref(c["segment"], c["S"], c["inverse"], c["emitted"], truth, T, weight, c["pred_class"] if use else None,
                       c["truth_class"] if use else None, c["num_class"] if use else 1, iou, mp)
    return got, ref


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("scatter", [False, True])
@pytest.mark.parametrize("n", mc.UNIT_COUNTS)
def test_unit_counts_around_a_wave_and_a_workgroup_at_three_thresholds(n, scatter, weight):
    c = mc.planted(n, seed=n, classes=n != 64, scatter=scatter)
    objects = on_device(c)
    for iou in IOUS:
        got, ref = run(c, weight, iou, objects=objects)
        same(got, ref, "n = %d, %s, iou %s" % (n, weight, iou))
        mr.check_theorem(ref)
    got, ref = run(c, weight, objects=objects, classes=False)                  # the classes omitted
    same(got, ref, "n = %d, %s, no classes" % (n, weight))
    assert got.num_pairs() == ref["stats"][0] >= 0 and not got.overflowed()


@pytest.mark.parametrize("weight", WEIGHTS)
def test_all_units_in_one_pair(weight):
    c = mc.one_pair(20000)
    got, ref = run(c, weight, max_pairs=1)
    same(got, ref, "one pair, " + weight)
    assert ref["stats"][0] == 1 and ref["pair_inter"][0] == 20000 and ref["pred_iou_q30"][0] == 1 << 30


@pytest.mark.parametrize("weight", WEIGHTS)
def test_every_unit_its_own_pair_fits_exactly_and_overflows_one_short(weight):
    n = 1025
    c = mc.all_pairs(n)
    objects = on_device(c)
    got, ref = run(c, weight, max_pairs=n, objects=objects)
    same(got, ref, "P == max_pairs, " + weight)
    assert got.num_pairs() == n and not got.overflowed() and got.trim().pair_pred.shape[0] == n
    got, ref = run(c, weight, max_pairs=n - 1, objects=objects)
    same(got, ref, "P == max_pairs + 1, " + weight)
    assert got.num_pairs() == -1 and got.overflowed() and got.trim().pair_pred.shape[0] == 0
    assert (ref["pair_pred"] == -1).all() and (ref["start"] == 0).all() and (ref["class_stats"] == 0).all()
    assert ref["pred_size"].sum() == n                                          # the sizes stay exact (M5)
    bound = got.pairs_bound()
    assert bound == n
    got, ref = run(c, weight, max_pairs=bound, objects=objects)
    same(got, ref, "the retry, " + weight)
    assert got.num_pairs() == n


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("name", mc.EDGES)
def test_edge_inputs(name, weight):
    c = mc.edge(name)
    got, ref = run(c, weight)
    same(got, ref, "%s, %s" % (name, weight))
    if name == "top_ids":
        assert ref["stats"][5] > 0 and ref["truth_size"][c["T"] - 1] > 0 and ref["pred_size"][c["S"] - 1] > 0
    if name == "no_inverse" and weight == "rows":
        assert ref["stats"][1] == 0 and ref["stats"][6] > 0


@pytest.mark.parametrize("weight", WEIGHTS)
def test_rows_of_the_table_longer_than_a_thread_walks(weight):
    c = mc.long_rows(300)
    got, ref = run(c, weight)
    same(got, ref, "long rows, " + weight)
    assert ref["start"][1] - ref["start"][0] == 300 and ref["t_start"][1] - ref["t_start"][0] == 300


@pytest.mark.parametrize("weight", WEIGHTS)
def test_equal_best_ious_go_to_the_lowest_number(weight):
    c = mc.ties()
    got, ref = run(c, weight)
    same(got, ref, "ties, " + weight)
    assert ref["best_pred"][0] == 0 and ref["best_truth"][2] == 1               # of segments 0 / 1 and of instances 1 / 2


def test_out_reuse_after_a_larger_call_and_two_runs_are_bitwise_equal():
    big, small = mc.all_pairs(500), mc.planted(500, 3, S=500, T=500)
    assert big["T"] == small["T"] == 500
    for weight in WEIGHTS:
        out = garbage(500, 500, 500, 1)
        got, ref = run(big, weight, out=out)
        same(got, ref, "the larger call")
        got, ref = run(small, weight, out=out)                                  # fewer pairs: the rows past P are filler again
        same(got, ref, "out= reuse, " + weight)
        assert 0 <= ref["stats"][0] < 500
        again, _ = run(small, weight)
        for name in mr.OUTPUTS:
            assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(again, name).cpu().numpy()), name


@functools.lru_cache(maxsize=None)
def scene(rooms):
    import torch
    from pointwise_amd import grid
    data, inst, lab, start = mc.boxes_scene(boxes=4, rooms=rooms)
    dev = _dev()
    d, l = torch.from_numpy(data).to(dev), torch.from_numpy(lab).to(dev)
    if rooms == 1:
        g = grid.grid_subsample(d, l, voxel=0.1, num_class=3)
    else:
        g = grid.grid_subsample_rooms(d, torch.from_numpy(start).to(dev), l, voxel=0.1, num_class=3)
    return g, inst, 4 * rooms


def against_ref(g, seg, inst, T, what):
    """match() on a segmentation the pipeline made, against the reference on its arrays read back."""
    import torch
    dev = _dev()
    inverse, segment = g.inverse.cpu().numpy(), seg.segment.cpu().numpy()
    M = segment.shape[0]
    voxel_truth = np.full(M, -1, np.int32)
    voxel_truth[inverse[inverse >= 0]] = inst[inverse >= 0]                    # every voxel lies in one box
    pc = seg.label
    tcls = (np.arange(T) % 4 % 3).astype(np.int32)                              # boxes_scene's labels
    for weight, truth in (("rows", inst), ("voxels", voxel_truth)):
        got = seg.match(torch.from_numpy(truth).to(dev), T, weight=weight, pred_class=pc, truth_class=torch.from_numpy(tcls).to(dev),
                        num_class=3, out=garbage(M, T, M, 3))
        ref = mr.match_ref(segment, int(seg.stats[0]), inverse, int(g.stats[0]), truth, T, weight, pc.cpu().numpy(), tcls, 3, (1, 2), M)
        same(got, ref, "%s, %s" % (what, weight))
    return got, ref


def test_a_plain_a_merged_and_an_agglomerated_segmentation():
    g, inst, T = scene(1)
    seg = g.segments(g.labels, 3)
    got, ref = against_ref(g, seg, inst, T, "plain")
    assert ref["stats"][0] == 4 and ref["class_stats"][:, 0].sum() == 4 and got.summary()["mean_pq"] == 1.0
    import torch
    pair = torch.tensor([0, 2], dtype=torch.int32, device=_dev())
    merged = seg.merge(pair[:1], pair[1:])                                      # boxes 0 and 2 as one segment: no match for either
    got, ref = against_ref(g, merged, inst, T, "merged")
    assert ref["class_stats"][:, 0].sum() == 2 and ref["class_stats"][:, 2].sum() == 2
    agg = seg.adjacency().agglomerate(min_size=8).segments                      # nothing is small: the identity
    got, ref = against_ref(g, agg, inst, T, "agglomerated")
    assert ref["class_stats"][:, 0].sum() == 4


def test_two_rooms_in_one_call():
    g, inst, T = scene(2)
    seg = g.segments(g.labels, 3)
    got, ref = against_ref(g, seg, inst, T, "two rooms")
    assert ref["stats"][0] == 8 and ref["stats"][8] == 8 << 30 and (ref["truth_match"] >= 0).all()
