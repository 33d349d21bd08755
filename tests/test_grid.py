"""GPU tests (-m gpu) of the voxel-grid subsampling, grid.grid_subsample on conv3p_grid_subsample_f32 and
GridSubsample.project on conv3p_grid_project_labels: every output bit for bit against tests/grid_ref.py, in both modes --
the edges of the row and sort tiles, lists that span sort tiles, every row its own voxel, lattices that need every sort
pass, the lattice limit and the error behind it, rows on lattice planes, a signed-zero minimum, non-finite rows, channel
counts, label types, the majority rule, the cut of max_voxels, reproducibility and the projection."""
import numpy as np
import pytest

from tests import grid_ref as gr

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("mean", "center")


def _dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def as_np(g):
    t = lambda x: None if x is None else x.cpu().numpy()
    return {"data": t(g.data), "labels": t(g.labels), "inverse": t(g.inverse), "voxel_row": t(g.voxel_row),
            "voxel_count": t(g.voxel_count), "voxel_cell": t(g.voxel_cell), "stats": t(g.stats)}


def run(data, labels=None, **kw):
    import torch
    from pointwise_amd import grid
    dev = _dev()
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    return grid.grid_subsample(d, lab, **kw)


def check(data, labels, voxel, what, num_class=13, max_voxels=None, modes=MODES):
    """Both modes against the reference; -> the reference results."""
    out = []
    for mode in modes:
        want = gr.grid_subsample_ref(data, labels, voxel=voxel, mode=mode, num_class=num_class, max_voxels=max_voxels)
        got = as_np(run(data, labels, voxel=voxel, mode=mode, num_class=num_class if labels is not None else None,
                        max_voxels=max_voxels))
        gr.assert_equal(got, want, "%s, %s" % (what, mode))
        out.append(want)
    return out


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 4095, 4096, 4097])
def test_the_smallest_cloud_and_the_edges_of_the_row_and_sort_tiles(N):
    data, labels = gr.cloud(N, 6, 100 + N, extent=(1.0, 0.8, 0.5), origin=(-2.0, 3.0, 0.1))
    want = check(data, labels, 0.11, "N = %d" % N)[0]
    assert want["stats"][7] == 0 and want["stats"][0] == want["stats"][1] >= 1 and (want["inverse"] >= 0).all()
    if N > 1:
        assert 1 < want["stats"][6] and want["stats"][0] < N                # voxels of several rows


def test_lists_that_span_sort_tiles():
    # all rows in one voxel: one list of 5000 rows, no sort pass runs (cells - 1 has no bit)
    data, labels = gr.cloud(5000, 4, 7, extent=(0.09, 0.09, 0.09), origin=(1.0, 1.0, 1.0))
    want = check(data, labels, 0.1, "one voxel")[0]
    assert want["stats"].tolist() == [1, 1, 1, 1, 1, 0, 5000, 0]
    # one voxel of 9000 rows among 3000 others, its rows scattered through the cloud
    crowd, lc = gr.cloud(9000, 4, 8, extent=(0.09, 0.09, 0.09), origin=(0.505, 0.505, 0.505))
    rest, lr = gr.cloud(3000, 4, 9, extent=(1.0, 1.0, 1.0))
    rest[0, :3] = 0.0                                    # lo = 0: the crowd is all of cell (5, 5, 5)
    perm = np.random.default_rng(10).permutation(12000)
    data, labels = np.concatenate([crowd, rest])[perm], np.concatenate([lc, lr])[perm]
    want = check(data, labels, 0.1, "a voxel of 9000 rows")[0]
    assert want["stats"][6] >= 9000 and want["stats"][1] > 500


def test_every_row_its_own_voxel():
    rng = np.random.default_rng(11)
    N = 4500
    cells = np.concatenate([[0], 1 + rng.permutation(20 * 20 * 20 - 1)[:N - 1]])
    ijk = np.stack([cells // 400, (cells // 20) % 20, cells % 20], axis=1)
    xyz = (ijk + 0.25 + 0.5 * rng.random((N, 3))) * 0.1
    xyz[0] = 0.0                                         # lo = 0, so a row's cell is the one it was drawn in
    data = np.concatenate([xyz, rng.random((N, 2))], axis=1).astype(F)
    labels = rng.integers(0, 13, size=N).astype(np.uint8)
    for want in check(data, labels, 0.1, "M = N"):
        assert want["stats"][0] == want["stats"][1] == N and want["stats"][6] == 1
        assert np.array_equal(np.sort(want["inverse"]), np.arange(N))
        assert np.array_equal(want["data"].view(np.uint32), data[want["voxel_row"]].view(np.uint32))   # x / 1.0f is x


def test_a_sparse_lattice_where_every_sort_pass_moves_data():
    data, labels = gr.cloud(3000, 5, 12, extent=(300.0, 310.0, 290.0), origin=(-150.0, 0.0, 7.0))
    want = check(data, labels, 1.0, "2.7e7 cells")[0]
    n = want["stats"][2:5].astype(np.int64)
    assert n.prod() > 1 << 24 and want["stats"][7] == 0
    # wider still: cells - 1 has a bit in each of the five digits
    data, labels = gr.cloud(3000, 5, 13, extent=(70000.0, 5000.0, 3000.0))
    want = check(data, labels, 1.0, "1.05e12 cells")[0]
    n = want["stats"][2:5].astype(np.int64)
    assert n.prod() > 1 << 32 and want["stats"][7] == 0 and want["stats"][1] > 2900


def _two_clusters(far):
    """200 rows in the cells next to the origin and 200 in the cells just inside `far`, voxel 1."""
    rng = np.random.default_rng(14)
    a = rng.random((200, 3)) * 3.0
    b = np.asarray(far)[None, :] - rng.random((200, 3)) * 3.0
    xyz = np.concatenate([a, b, [[0.0, 0.0, 0.0]], [far]])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    data = np.concatenate([xyz, rng.random((xyz.shape[0], 1))], axis=1).astype(F)
    return data, rng.integers(0, 13, size=data.shape[0]).astype(np.int32)


def test_the_lattice_limit_and_one_step_past_it():
    data, labels = _two_clusters((1048575.5, 1023.5, 1023.5))
    want = check(data, labels, 1.0, "2^40 cells")[0]
    assert want["stats"][2:5].tolist() == [1 << 20, 1024, 1024] and want["stats"][7] == 0 and want["stats"][1] > 50
    data, labels = _two_clusters((1048575.5, 1023.5, 1022.5))
    want = check(data, labels, 1.0, "just under 2^40 cells")[0]
    assert want["stats"][2:5].tolist() == [1 << 20, 1024, 1023] and want["stats"][7] == 0
    for far in ((1048575.5, 1023.5, 1024.5), (1048576.5, 1.5, 1.5), (3.0e38, 1.5, 1.5)):
        data, labels = _two_clusters(far)
        for want in check(data, labels, 1.0, "past the limit %r" % (far,), max_voxels=50):
            assert want["stats"][[0, 1, 6, 7]].tolist() == [0, 0, 0, 1] and (want["inverse"] == -1).all()
            assert (want["voxel_row"] == -1).all() and not want["data"].any()


def test_rows_on_exact_lattice_planes():
    rng = np.random.default_rng(15)
    for voxel, quantum in ((0.25, 0.25), (0.1, 0.1), (0.3, 0.1)):
        q = rng.integers(0, 12, size=(2000, 3))
        xyz = (q.astype(F) * F(quantum)).astype(F)                            # float32 products: s / voxel is, or just misses, an integer
        data = np.concatenate([xyz, rng.random((2000, 1)).astype(F)], axis=1)
        check(data, rng.integers(0, 5, size=2000).astype(np.uint8), voxel, "planes of %g at voxel %g" % (quantum, voxel), num_class=5)


def test_a_minimum_that_is_minus_zero_next_to_plus_zero():
    data, labels = gr.cloud(1500, 4, 16, extent=(1.0, 1.0, 1.0))
    data[7, 0], data[900, 0], data[20, 1], data[21, 1], data[1400, 2] = 0.0, -0.0, -0.0, 0.0, -0.0
    data[8, 0], data[8, 1], data[8, 2] = -0.0, -0.0, -0.0                     # a voxel whose mean keeps the sign of its zeros
    fin, lo, s, i, n = gr.cells_of(data, 0.07)
    assert np.signbit(lo).all() and (lo == 0).all()
    check(data, labels, 0.07, "signed zeros")
    check(data[[8, 900, 1400]], labels[[8, 900, 1400]], 0.07, "only zeros")


def test_non_finite_rows_are_counted_and_get_no_voxel():
    data, labels = gr.cloud(3000, 5, 17)
    bad = np.random.default_rng(18).permutation(3000)[:40]
    data[bad[:15], 0], data[bad[15:30], 1], data[bad[30:], 2] = np.nan, np.inf, -np.inf
    data[bad[0], 1] = np.inf
    for want in check(data, labels, 0.09, "non-finite rows"):
        assert want["stats"][5] == 40 and (want["inverse"][bad] == -1).all() and (np.delete(want["inverse"], bad) >= 0).all()
    none = np.full((300, 3), np.nan, F)
    for want in check(none, None, 0.09, "no finite row"):
        assert want["stats"].tolist() == [0, 0, 0, 0, 0, 300, 0, 0] and (want["inverse"] == -1).all()


@pytest.mark.parametrize("K", [3, 12])
def test_no_features_and_many_features(K):
    data, labels = gr.cloud(2500, K, 19 + K, extent=(0.6, 0.7, 0.8))
    check(data, labels, 0.05, "K = %d" % K)
    check(data, None, 0.2, "K = %d, no labels" % K)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64])
def test_label_dtypes(dtype):
    data, labels = gr.cloud(2000, 4, 22, extent=(0.5, 0.5, 0.5))
    labels = labels.astype(dtype)
    if dtype != np.uint8:
        labels[::7] = -1
        labels[3::11] = 13
    if dtype == np.int64:
        labels[5::13] = (1 << 32) + 2                    # not class 2: compared in 64 bits; the centre mode casts it
        labels[6::17] = -(1 << 40)
    check(data, labels, 0.06, "labels %s" % np.dtype(dtype).name)
    check(data, labels, 0.06, "labels %s, 128 classes" % np.dtype(dtype).name, num_class=128, modes=("mean",))
    check(data, (labels.astype(np.int64) * 9 % 128).astype(dtype), 0.06, "classes up to 127", num_class=128, modes=("mean",))


def test_the_majority_rule_on_the_cloud_written_out_by_hand():
    data, labels = gr.hand_cloud()
    mean, center = check(data, labels, 0.5, "by hand", num_class=4, max_voxels=7)
    got = as_np(run(data, labels, voxel=0.5, mode="mean", num_class=4, max_voxels=7))
    assert got["labels"].tolist() == [1, 0, 0, -1, 3, -1, -1] and got["stats"].tolist() == [5, 5, 3, 2, 3, 2, 4, 0]
    assert got["inverse"].tolist() == [0, 0, 3, -1, 0, 1, 3, 0, 2, -1, 1, 4] and got["data"][:5, 3].tolist() == [3.5, 8.0, 8.0, 4.5, 12.0]
    got = as_np(run(data, labels, voxel=0.5, mode="center", max_voxels=7))
    assert got["voxel_row"].tolist() == [1, 10, 8, 6, 11, -1, -1] and got["labels"].tolist() == [1, 0, 0, -1, 3, -1, -1]
    # a long list (the LDS histogram over many steps of its lanes) with a tie and with no valid label
    crowd, _ = gr.cloud(696, 3, 23, extent=(0.09, 0.09, 0.09))
    crowd[0] = 0.0                                       # lo = 0: the other rows are all of cell (5, 0, 0)
    other, _ = gr.cloud(300, 3, 24, extent=(0.05, 0.09, 0.09), origin=(0.52, 0.0, 0.0))
    lab = np.concatenate([np.tile(np.array([9, 4, 200, 4, 9, -3], np.int32), 116), np.full(300, 77, np.int32)])   # 232 : 232
    want = check(np.concatenate([crowd, other]), lab, 0.1, "a long tie", num_class=13)[0]
    assert want["stats"][0] == 2 and want["labels"][:2].tolist() == [4, -1]


def test_max_voxels_cuts_the_cloud():
    data, labels = gr.cloud(3000, 5, 25)
    full = gr.grid_subsample_ref(data, labels, voxel=0.1, mode="mean", num_class=13)
    V = int(full["stats"][1])
    for mv in (1, V // 2, V - 1, V, V + 5):
        for want in check(data, labels, 0.1, "max_voxels %d of %d" % (mv, V), max_voxels=mv):
            assert want["stats"][0] == min(mv, V) and want["stats"][1] == V and want["data"].shape[0] == mv
            assert (want["stats"][0] < want["stats"][1]) == (mv < V)
            assert (want["inverse"] >= min(mv, V)).sum() == 0 and ((want["inverse"] == -1).sum() > 0) == (mv < V)


def test_two_calls_are_bitwise_equal_and_trim_is_a_view():
    import torch
    data, labels = gr.cloud(4000, 6, 26)
    for mode in MODES:
        a = run(data, labels, voxel=0.08, mode=mode, num_class=13)
        first = {k: (None if v is None else v.copy()) for k, v in as_np(a).items()}
        b = run(data, labels, voxel=0.08, mode=mode, num_class=13)
        gr.assert_equal(as_np(b), first, "a second call, " + mode)
        dev = a.data.device
        again = __import__("pointwise_amd.grid", fromlist=["x"]).grid_subsample(
            torch.from_numpy(data).to(dev), torch.from_numpy(labels).to(dev), voxel=0.08, mode=mode, num_class=13, out=a)
        assert again is a
        gr.assert_equal(as_np(a), first, "written into out, " + mode)
        t = a.trim()
        nv = a.num_voxels()
        assert t.data.shape == (nv, 6) and t.labels.shape == (nv,) and t.voxel_cell.shape == (nv, 3) and t.num_voxels() == nv
        assert t.data.data_ptr() == a.data.data_ptr() and t.inverse is a.inverse and int(t.voxel_count.sum()) == 4000


def test_project_on_voxels_that_include_minus_one():
    import torch
    data, labels = gr.cloud(3000, 4, 27)
    data[11, 0] = np.nan
    labels = labels.astype(np.int32)
    labels[::3] = -1                                     # voxels without a valid label get -1
    g = run(data, labels, voxel=0.1, mode="mean", num_class=13, max_voxels=400)       # and max_voxels cuts: inverse has -1
    want = gr.grid_subsample_ref(data, labels, voxel=0.1, mode="mean", num_class=13, max_voxels=400)
    gr.assert_equal(as_np(g), want, "cut")
    assert (want["labels"][:400] == -1).any() and (want["inverse"] == -1).sum() > 1
    got = g.project(g.labels)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), gr.project_ref(want["labels"], want["inverse"]))
    t = g.trim()
    short = t.labels[:250].contiguous()                  # fewer labels than voxels: the rows of the others get -1
    assert np.array_equal(t.project(short).cpu().numpy(), gr.project_ref(want["labels"][:250], want["inverse"]))
    out = torch.empty(3000, dtype=torch.int32, device=got.device)
    assert t.project(t.labels, out=out) is out and np.array_equal(out.cpu().numpy(), got.cpu().numpy())
    assert (t.project(torch.empty(0, dtype=torch.int32, device=got.device)) == -1).all()
