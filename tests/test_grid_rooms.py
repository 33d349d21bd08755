"""GPU tests (-m gpu) of the many-clouds voxel-grid subsampling, grid.grid_subsample_rooms on
conv3p_grid_subsample_rooms_f32: every output bit for bit against tests/grid_rooms_ref.py, in both modes -- one room against
the single call, room boundaries inside and on the edges of a row tile, thousands of tiny rooms, a room twice, a signed-zero
minimum in one room, non-finite rows, the cut of max_voxels at, inside and before rooms, a list that spans sort tiles
behind another room, cell_base past every digit of the sort, the limit of the cells' sum, a room past its own limit, a
malformed room_start, label types and channel counts, reproducibility, and the loop of single calls on the device."""
import numpy as np
import pytest

from tests import grid_ref as gr
from tests import grid_rooms_ref as grr
from tests.test_grid import _dev, _two_clusters
from tests.test_grid import as_np as single_np

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("mean", "center")


def as_np(g):
    r = single_np(g)
    r.update({k: getattr(g, k).cpu().numpy() for k in ("voxel_room", "voxel_start", "room_stats")})
    return r


def run(data, room_start, labels=None, **kw):
    import torch
    from pointwise_amd import grid
    dev = _dev()
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    return grid.grid_subsample_rooms(d, torch.from_numpy(np.asarray(room_start, np.int32)).to(dev), lab, **kw)


def check(data, room_start, labels, voxel, what, num_class=13, max_voxels=None, modes=MODES):
    """Both modes against the reference; -> the reference results."""
    out = []
    for mode in modes:
        want = grr.grid_subsample_rooms_ref(data, room_start, labels, voxel=voxel, mode=mode, num_class=num_class,
                                            max_voxels=max_voxels)
        got = as_np(run(data, room_start, labels, voxel=voxel, mode=mode, num_class=num_class if labels is not None else None,
                        max_voxels=max_voxels))
        grr.assert_equal(got, want, "%s, %s" % (what, mode))
        out.append(want)
    return out


@pytest.mark.parametrize("N", [1, 1025, 4097])
def test_one_room_equals_the_single_call(N):
    import torch
    from pointwise_amd import grid
    data, labels = gr.cloud(N, 6, 100 + N, extent=(1.0, 0.8, 0.5), origin=(-2.0, 3.0, 0.1))
    want = check(data, [0, N], labels, 0.11, "R = 1, N = %d" % N)
    assert want[0]["stats"][7] == 0 and want[0]["stats"][[2, 3]].tolist() == [1, 1]
    dev = _dev()
    for mode in MODES:
        nc = 13 if mode == "mean" else None
        one = single_np(grid.grid_subsample(torch.from_numpy(data).to(dev), torch.from_numpy(labels).to(dev), voxel=0.11,
                                            mode=mode, num_class=nc))
        got = as_np(run(data, [0, N], labels, voxel=0.11, mode=mode, num_class=nc))
        gr.assert_equal(got, dict(one, stats=got["stats"]), "the single call on the device, " + mode)
        assert np.array_equal(got["room_stats"][0], one["stats"]) and got["voxel_start"].tolist() == [0, int(one["stats"][0])]


def test_room_boundaries_inside_and_on_the_edges_of_a_row_tile():
    data, labels = gr.cloud(5100, 5, 31, extent=(1.0, 0.9, 0.7), origin=(-0.3, 0.2, 0.0))
    start = [3, 4, 1023, 1024, 1024, 1025, 2048, 4097, 5000]
    for want in check(data, start, labels, 0.1, "boundaries"):
        assert (want["inverse"][:3] == -1).all() and (want["inverse"][5000:] == -1).all() and (want["inverse"][3:5000] >= 0).all()
        assert want["room_stats"][3].tolist() == [0] * 8 and want["stats"][[2, 3, 4, 5, 7]].tolist() == [8, 7, 0, 0, 0]
        assert int(want["voxel_count"].sum()) == 4997 and int(want["room_stats"][:, 1].sum()) == want["stats"][1]


def test_three_thousand_rooms_of_one_to_three_rows():
    sizes = np.random.default_rng(32).integers(1, 4, size=3000)
    data, labels, start = grr.rooms_cloud(sizes, 4, 33)
    for want in check(data, start, labels, 0.3, "3000 rooms"):
        assert want["stats"][[2, 3, 7]].tolist() == [3000, 3000, 0] and want["stats"][1] > 3000


def test_a_room_concatenated_with_itself_keeps_its_voxels_apart():
    d, l = gr.cloud(2500, 5, 34)
    want = check(np.concatenate([d, d]), [0, 2500, 5000], np.concatenate([l, l]), 0.1, "a room twice")[0]
    V = int(want["room_stats"][0, 1])
    assert want["stats"][1] == 2 * V and np.array_equal(want["inverse"][2500:], want["inverse"][:2500] + V)
    assert np.array_equal(want["data"][:V].view(np.uint32), want["data"][V:2 * V].view(np.uint32))


def test_a_minimum_that_is_minus_zero_in_one_room_only():
    d, l = gr.cloud(1500, 4, 16, extent=(1.0, 1.0, 1.0))
    z = d.copy()
    z[7, 0], z[900, 0], z[20, 1], z[21, 1], z[1400, 2] = 0.0, -0.0, -0.0, 0.0, -0.0
    z[8, :3] = -0.0
    p = d.copy()
    p[7, 0], p[20, 1], p[1400, 2] = 0.0, 0.0, 0.0
    check(np.concatenate([p, z, p]), [0, 1500, 3000, 4500], np.concatenate([l, l, l]), 0.07, "signed zeros in room 1")


def test_non_finite_rows_and_a_room_without_a_finite_row():
    data, labels, start = grr.rooms_cloud([1200, 300, 1500, 2], 5, 35)
    bad = np.random.default_rng(36).permutation(1200)[:30]
    data[bad[:10], 0], data[bad[10:20], 1], data[bad[20:], 2] = np.nan, np.inf, -np.inf
    data[1200:1500, :3] = np.nan
    data[2000, 1] = np.inf
    for want in check(data, start, labels, 0.09, "non-finite rows"):
        assert want["stats"][5] == 331 and want["room_stats"][1].tolist() == [0, 0, 0, 0, 0, 300, 0, 0]
        assert want["stats"][3] == 3 and (want["inverse"][1200:1500] == -1).all() and (want["inverse"][bad] == -1).all()


def test_the_cut_at_a_boundary_inside_a_room_and_before_the_last_rooms():
    data, labels, start = grr.rooms_cloud([900, 1100, 700, 800], 5, 37)
    full = grr.grid_subsample_rooms_ref(data, start, labels, voxel=0.1, mode="mean", num_class=13)
    first = np.concatenate([[0], np.cumsum(full["room_stats"][:, 1])])
    for mv, what in ((int(first[2]), "at a boundary"), (int(first[2]) + 5, "inside a room"), (int(first[2]) - 3, "before the last two"),
                     (1, "one voxel"), (int(first[4]) + 9, "never")):
        for want in check(data, start, labels, 0.1, "max_voxels %d, %s" % (mv, what), max_voxels=mv):
            assert want["stats"][0] == min(mv, first[4]) and want["stats"][1] == first[4]
            assert np.array_equal(want["room_stats"][:, 1:], full["room_stats"][:, 1:])          # words 1-7 whatever the cut
            assert want["room_stats"][:, 0].tolist() == np.diff(np.minimum(first, mv)).tolist()
    assert full["room_stats"][:, 1].min() > 8


def test_a_list_that_spans_sort_tiles_in_the_second_room():
    small, ls = gr.cloud(700, 4, 38, extent=(0.5, 0.5, 0.5), origin=(3.0, 3.0, 3.0))
    crowd, lc = gr.cloud(9000, 4, 8, extent=(0.09, 0.09, 0.09), origin=(0.505, 0.505, 0.505))
    rest, lr = gr.cloud(3000, 4, 9, extent=(1.0, 1.0, 1.0))
    rest[0, :3] = 0.0                                    # lo = 0: the crowd is all of cell (5, 5, 5)
    perm = np.random.default_rng(10).permutation(12000)
    data = np.concatenate([small, np.concatenate([crowd, rest])[perm]])
    labels = np.concatenate([ls, np.concatenate([lc, lr])[perm]])
    want = check(data, [0, 700, 12700], labels, 0.1, "a voxel of 9000 rows in room 1")[0]
    assert want["room_stats"][1, 6] >= 9000 and want["stats"][6] == want["room_stats"][1, 6] > want["room_stats"][0, 6]


def test_cell_base_crossing_every_digit_of_the_sort():
    big, lb = gr.cloud(3000, 5, 13, extent=(70000.0, 5000.0, 3000.0))        # 1.05e12 cells: cell_base[1] > 2^32
    parts, labs, sizes = [big], [lb], [3000]
    for k in range(5):
        d, l = gr.cloud(400 + 37 * k, 5, 40 + k, extent=(9.0 + k, 7.0, 5.0), origin=(100.0 * k, -3.0, 2.0))
        parts.append(d)
        labs.append(l)
        sizes.append(d.shape[0])
    start = np.concatenate([[0], np.cumsum(sizes)])
    want = check(np.concatenate(parts), start, np.concatenate(labs), 1.0, "cell_base > 2^32")[0]
    n = want["room_stats"][0, 2:5].astype(np.int64)
    assert n.prod() > 1 << 32 and want["stats"][7] == 0 and want["stats"][3] == 6 and want["room_stats"][1:, 1].min() > 100


def test_the_limit_of_the_cells_summed_over_the_rooms():
    a, la = _two_clusters((1048575.5, 1023.5, 1022.5))                        # 2^20 x 1024 x 1023 cells
    b, lb = _two_clusters((1023.5, 1023.5, 1023.5))                           # 2^30 cells: exactly 2^40 in all
    data, labels = np.concatenate([a, b]), np.concatenate([la, lb])
    start = [0, a.shape[0], a.shape[0] + b.shape[0]]
    for want in check(data, start, labels, 1.0, "2^40 cells in all"):
        assert want["stats"][7] == 0 and want["room_stats"][:, 2:5].tolist() == [[1 << 20, 1024, 1023], [1024, 1024, 1024]]
        assert want["stats"][1] > 100 and want["room_stats"][:, 1].min() > 50
    one = np.array([[4.0, 4.0, 4.0, 0.5], [np.nan, 4.0, 4.0, 0.5]], F)       # one cell more
    data, labels = np.concatenate([data, one]), np.concatenate([labels, np.array([1, 2], np.int32)])
    for want in check(data, start + [start[2] + 2], labels, 1.0, "one cell past 2^40", max_voxels=60):
        assert want["stats"].tolist() == [0, 0, 3, 0, 0, 1, 0, 4] and (want["inverse"] == -1).all() and not want["voxel_start"].any()
        assert want["room_stats"].tolist() == [[0, 0, 1 << 20, 1024, 1023, 0, 0, 0], [0, 0, 1024, 1024, 1024, 0, 0, 0],
                                               [0, 0, 1, 1, 1, 1, 0, 0]]
        assert (want["voxel_row"] == -1).all() and not want["data"].any()


def test_a_room_past_its_own_limit_between_two_good_rooms():
    a, la = gr.cloud(1300, 4, 41, extent=(2.0, 1.0, 1.0))
    c, lc = gr.cloud(1100, 4, 42, extent=(1.0, 2.0, 1.0), origin=(5.0, 5.0, 5.0))
    bad, lbad = _two_clusters((1048576.5, 1.5, 1.5))
    la, lc = la.astype(np.int32), lc.astype(np.int32)
    with_bad = check(np.concatenate([a, bad, c]), [0, 1300, 1300 + bad.shape[0], 2400 + bad.shape[0]],
                     np.concatenate([la, lbad, lc]), 0.2, "a bad room in the middle")
    without = check(np.concatenate([a, c]), [0, 1300, 2400], np.concatenate([la, lc]), 0.2, "the good rooms alone")
    for w, o in zip(with_bad, without):
        assert w["stats"][[4, 7]].tolist() == [1, 1] and w["room_stats"][1][[0, 1, 5, 6, 7]].tolist() == [0, 0, 0, 0, 1] and w["room_stats"][1, 2] > 1 << 20
        nv = int(o["stats"][0])
        assert w["stats"][0] == nv and (w["inverse"][1300:1300 + bad.shape[0]] == -1).all()
        for k in ("data", "labels", "voxel_count", "voxel_cell"):            # the numbering shifted by nothing
            assert np.array_equal(w[k][:nv], o[k][:nv]), k
        assert np.array_equal(np.delete(w["inverse"], np.arange(1300, 1300 + bad.shape[0])), o["inverse"])
        assert np.array_equal(w["room_stats"][[0, 2]], o["room_stats"]) and w["voxel_room"][:nv].max() == 2


@pytest.mark.parametrize("start", [[0, 2000, 1500, 3000], [-1, 1500, 3000], [0, 1500, 3001]])
def test_a_malformed_room_start_sets_bit_1(start):
    data, labels = gr.cloud(3000, 4, 43)
    for want in check(data, start, labels, 0.1, "room_start %r" % (start,), max_voxels=500):
        assert want["stats"].tolist() == [0, 0, len(start) - 1, 0, 0, 0, 0, 2] and (want["inverse"] == -1).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64])
def test_label_dtypes(dtype):
    data, labels, start = grr.rooms_cloud([800, 1, 1200], 4, 44)
    labels = labels.astype(dtype)
    if dtype != np.uint8:
        labels[::7] = -1
        labels[3::11] = 13
    if dtype == np.int64:
        labels[5::13] = (1 << 32) + 2                    # not class 2: compared in 64 bits; the centre mode casts it
    check(data, start, labels, 0.12, "labels %s" % np.dtype(dtype).name)
    check(data, start, labels, 0.12, "labels %s, 128 classes" % np.dtype(dtype).name, num_class=128, modes=("mean",))


@pytest.mark.parametrize("K", [3, 12])
def test_no_features_many_features_and_no_labels(K):
    data, labels, start = grr.rooms_cloud([1000, 1500], K, 45 + K)
    check(data, start, labels, 0.07, "K = %d" % K)
    check(data, start, None, 0.2, "K = %d, no labels" % K)


def test_two_calls_are_bitwise_equal_and_out_leaves_no_stale_word():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    data, labels, start = grr.rooms_cloud([1500, 900, 1600], 6, 47)
    other, lo, so = grr.rooms_cloud([100, 2400, 1500], 6, 48, spread=3.0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for mode in MODES:
        nc = 13 if mode == "mean" else None
        a = run(data, start, labels, voxel=0.08, mode=mode, num_class=nc, max_voxels=3000)
        first = {k: (None if v is None else v.copy()) for k, v in as_np(a).items()}
        grr.assert_equal(as_np(run(data, start, labels, voxel=0.08, mode=mode, num_class=nc, max_voxels=3000)), first,
                         "a second call, " + mode)
        b = run(other, so, lo, voxel=0.3, mode=mode, num_class=nc, max_voxels=3000)       # other content, fewer voxels
        again = grid.grid_subsample_rooms(t(data), t(start), t(labels), voxel=0.08, mode=mode, num_class=nc, max_voxels=3000, out=b)
        assert again is b
        grr.assert_equal(as_np(b), first, "written into the out of another call, " + mode)
        want = grr.grid_subsample_rooms_ref(data, start, labels, voxel=0.08, mode=mode, num_class=13, max_voxels=3000)
        grr.assert_equal(first, want, "the reference, " + mode)
        tr = a.trim()
        nv = a.num_voxels()
        assert tr.data.shape == (nv, 6) and tr.voxel_room.shape == (nv,) and tr.voxel_start is a.voxel_start
        r1 = a.room(1)
        v0, v1 = want["voxel_start"][1:3]
        assert r1.data.data_ptr() == a.data[v0:].data_ptr() and r1.data.shape == (v1 - v0, 6)
        assert r1.stats.cpu().numpy().tolist() == want["room_stats"][1].tolist()


def test_the_rooms_call_equals_the_loop_of_single_calls_on_the_device():
    import torch
    from pointwise_amd import grid
    dev = _dev()
    data, labels, start = grr.rooms_cloud([1300, 0, 40, 2100, 1], 5, 49)
    for mode in MODES:
        nc = 13 if mode == "mean" else None

        def single(rows, lab, mv):
            return single_np(grid.grid_subsample(torch.from_numpy(np.ascontiguousarray(rows)).to(dev),
                                                 torch.from_numpy(np.ascontiguousarray(lab)).to(dev), voxel=0.1, mode=mode,
                                                 num_class=nc, max_voxels=mv))
        for mv in (None, 700):
            loop = grr.loop_ref(single, data, start, labels, mv, 5)
            got = as_np(run(data, start, labels, voxel=0.1, mode=mode, num_class=nc, max_voxels=mv))
            grr.assert_equal(got, loop, "the loop, %s, max_voxels %r" % (mode, mv),
                             keys=("inverse", "voxel_count", "voxel_cell", "voxel_row", "labels", "data", "voxel_start"))
