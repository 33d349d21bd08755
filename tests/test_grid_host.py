"""CPU tests (not gpu) of the voxel-grid subsampling (include/conv3p.h: conv3p_grid_subsample_f32,
conv3p_grid_project_labels): the symbols and their argument types, the workspace bound and every status through the
library (none of them launches), the argument checks of grid.grid_subsample (all before device work), and the numpy
reference against a cloud written out by hand and against np.unique."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, grid
from pointwise_amd.conv3p_op import Conv3pInvalidArgument
from tests import grid_ref as gr

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
PTR = ctypes.c_void_p(4096)
F = np.float32


def test_symbols_are_declared_with_argtypes():
    lib = _lib.load()
    for name, nargs in (("conv3p_grid_subsample_workspace_bytes", 2), ("conv3p_grid_subsample_f32", 19),
                        ("conv3p_grid_project_labels", 6)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert lib.conv3p_abi_version() == _lib.ABI_VERSION == 5                 # additions do not move it
    assert (_lib.GRID_MEAN, _lib.GRID_CENTER) == (0, 1) and _lib.GRID_MAX_ROWS == 1 << 24


def test_workspace_bytes_through_the_library():
    f = _lib.load().conv3p_grid_subsample_workspace_bytes
    rows = (1, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 70000, 1 << 20, 1 << 24)
    for mv in (1, 1000, 1 << 24, 2 ** 31 - 1):
        sizes = [f(N, mv) for N in rows]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
        assert sizes[-1] >= (1 << 24) * 20                                   # two pair buffers and the list starts
    assert f(1000, 1) <= f(1000, 1 << 30)
    # refused, or nothing to do
    assert f(0, 10) == 0 and f(-1, 10) == 0 and f((1 << 24) + 1, 10) == 0
    assert f(1000, 0) == 0 and f(1000, -1) == 0


def test_status_codes_and_their_order():
    lib = _lib.load()
    f, nbytes = lib.conv3p_grid_subsample_f32, lib.conv3p_grid_subsample_workspace_bytes
    big = 1 << 40

    def call(N=100, K=6, lb=1, voxel=0.1, mode=0, ncls=13, mv=10, data=PTR, labels=PTR, lab_out=PTR, out=PTR, row=PTR,
             cnt=PTR, cell=PTR, inverse=PTR, stats=PTR, ws=PTR, ws_bytes=big):
        return f(data, labels, N, K, lb, voxel, mode, ncls, mv, out, lab_out, row, cnt, cell, inverse, stats, ws, ws_bytes, None)
    assert call(N=-1) == INV and call(K=2) == INV and call(mv=-1) == INV and call(mode=2) == INV and call(mode=-1) == INV
    assert call(voxel=float("inf")) == INV and call(voxel=float("nan")) == INV and call(voxel=0.0) == INV and call(voxel=-1.0) == INV
    assert call(labels=None) == INV and call(lab_out=None) == INV and call(lb=2) == INV and call(lb=0) == INV
    assert call(ncls=0) == INV and call(ncls=-5) == INV
    assert call(ncls=0, mode=1, ws=None) == WS and call(ncls=0, labels=None, lab_out=None, ws=None) == WS   # not read there
    nothing = dict(data=None, out=None, row=None, cnt=None, cell=None, inverse=None, stats=None, labels=None, lab_out=None,
                   ws=None, ws_bytes=0)
    assert call(N=-1, mv=0) == INV and call(K=2, N=0) == INV                 # invalid arguments before "nothing to do"
    assert call(N=0, **nothing) == OK and call(mv=0, **nothing) == OK
    assert call(N=0, K=70000, ncls=500, **nothing) == OK                     # ... which comes before the limits
    for name in ("data", "out", "row", "cnt", "cell", "inverse", "stats"):
        assert call(**{name: None}) == INV, name
    assert call(data=None, N=(1 << 24) + 1) == INV                           # a NULL pointer before the limits
    assert call(N=(1 << 24) + 1) == UNS and call(K=65537) == UNS and call(ncls=129) == UNS
    assert call(ncls=129, mode=1, ws=None) == WS and call(ncls=128, ws=None) == WS
    assert call(N=(1 << 24) + 1, ws=None) == UNS                             # the limits before the workspace
    need = nbytes(100, 10)
    assert need > 0 and call(ws=None) == WS and call(ws_bytes=need - 1) == WS and call(ws=ctypes.c_void_p(4097)) == WS
    assert call(mode=1, ws_bytes=need - 1) == WS and call(labels=None, lab_out=None, ws=None) == WS


def test_project_status_codes():
    f = _lib.load().conv3p_grid_project_labels
    assert f(PTR, PTR, -1, 5, PTR, None) == INV and f(PTR, PTR, 5, -1, PTR, None) == INV
    assert f(None, None, 0, 5, None, None) == OK
    assert f(PTR, None, 5, 5, PTR, None) == INV and f(PTR, PTR, 5, 5, None, None) == INV and f(None, PTR, 5, 5, PTR, None) == INV
    assert f(PTR, PTR, 1 << 31, 5, PTR, None) == UNS and f(PTR, PTR, 5, 1 << 31, PTR, None) == UNS


@pytest.mark.parametrize("kw,msg", [
    (dict(data=torch.zeros((10, 6), dtype=torch.float64)), "float32"),
    (dict(data=torch.zeros((10, 2), dtype=torch.float32)), "float32"),
    (dict(data=torch.zeros((6, 10), dtype=torch.float32).t()), "contiguous"),
    (dict(labels=torch.zeros(10, dtype=torch.int16), num_class=4), "labels"),
    (dict(labels=torch.zeros(9, dtype=torch.int32), num_class=4), "labels"),
    (dict(voxel=0.0), "voxel"),
    (dict(voxel=float("nan")), "voxel"),
    (dict(voxel=1e-60), "voxel"),
    (dict(voxel="0.1"), "voxel"),
    (dict(mode="median"), "mode"),
    (dict(mode=0), "mode"),
    (dict(labels=torch.zeros(10, dtype=torch.uint8)), "num_class"),
    (dict(labels=torch.zeros(10, dtype=torch.uint8), num_class=0), "num_class"),
    (dict(labels=torch.zeros(10, dtype=torch.uint8), num_class=129), "num_class"),
    (dict(num_class=2.5), "num_class"),
    (dict(max_voxels=-1), "max_voxels"),
    (dict(max_voxels=2 ** 31), "max_voxels"),
    (dict(out=object()), "another shape"),
])
def test_argument_checks_raise_before_device_work(kw, msg):
    a = dict(data=torch.zeros((10, 6), dtype=torch.float32))
    a.update(kw)
    with pytest.raises(Conv3pInvalidArgument, match=msg):
        grid.grid_subsample(**a)


def test_out_of_another_shape_and_the_no_cpu_path_check_come_last():
    data = torch.zeros((10, 6), dtype=torch.float32)
    out = grid.GridSubsample(10, 8, 6, False, torch.device("cpu"))
    for kw in (dict(max_voxels=9), dict(max_voxels=8, data=torch.zeros((11, 6))), dict(max_voxels=8, data=torch.zeros((10, 7))),
               dict(max_voxels=8, labels=torch.zeros(10, dtype=torch.uint8), num_class=3)):
        a = dict(data=data, out=out)
        a.update(kw)
        with pytest.raises(Conv3pInvalidArgument, match="another shape"):
            grid.grid_subsample(**a)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):          # every check passed: only the device is wrong
        grid.grid_subsample(data, max_voxels=8, out=out)
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):
        grid.grid_subsample(data, torch.zeros(10, dtype=torch.int64), mode="center")
    with pytest.raises(Conv3pInvalidArgument, match="voxel_labels"):
        out.project(torch.zeros(8, dtype=torch.int64))
    with pytest.raises(Conv3pInvalidArgument, match="no CPU path"):
        out.project(torch.zeros(8, dtype=torch.int32))


def chain(*v):
    """(((v0 + v1) + v2) + ...) / float32(n), every step one float32 operation."""
    acc = F(v[0])
    for x in v[1:]:
        acc = F(acc + F(x))
    return F(acc / F(len(v)))


def test_reference_on_the_cloud_written_out_by_hand():
    data, labels = gr.hand_cloud()
    r = gr.grid_subsample_ref(data, labels, voxel=0.5, mode="mean", num_class=4, max_voxels=7)
    assert r["stats"].tolist() == [5, 5, 3, 2, 3, 2, 4, 0]
    assert r["inverse"].tolist() == [0, 0, 3, -1, 0, 1, 3, 0, 2, -1, 1, 4]
    assert r["voxel_cell"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 2], [2, 0, 0], [2, 0, 2], [-1, -1, -1], [-1, -1, -1]]
    assert r["voxel_count"].tolist() == [4, 2, 1, 2, 1, 0, 0]
    assert r["voxel_row"].tolist() == [0, 5, 8, 2, 11, -1, -1]
    # voxel 0: classes 2, 1, 1, 2 tie -> the lower; voxel 1: 3 and 0 tie -> 0; voxel 3: labels 5 and -1, none valid
    assert r["labels"].tolist() == [1, 0, 0, -1, 3, -1, -1]
    members = [[0, 1, 4, 7], [5, 10], [8], [2, 6], [11]]
    want = np.zeros((7, 4), F)
    for v, m in enumerate(members):
        for k in range(4):
            want[v, k] = chain(*[data[i, k] for i in m])
    assert np.array_equal(r["data"].view(np.uint32), want.view(np.uint32))
    assert r["data"][:5, 3].tolist() == [3.5, 8.0, 8.0, 4.5, 12.0]
    # the centre mode: row 1 sits on its voxel's centre, rows 10 and 6 are the nearer of two
    c = gr.grid_subsample_ref(data, labels, voxel=0.5, mode="center", max_voxels=7)
    assert c["voxel_row"].tolist() == [1, 10, 8, 6, 11, -1, -1]
    assert c["labels"].tolist() == [1, 0, 0, -1, 3, -1, -1]
    assert np.array_equal(c["data"][:5].view(np.uint32), data[[1, 10, 8, 6, 11]].view(np.uint32)) and not c["data"][5:].any()
    for k in ("stats", "inverse", "voxel_cell", "voxel_count"):
        assert np.array_equal(c[k], r[k]), k
    # max_voxels cuts: the rows of voxels 3 and 4 lose their voxel
    cut = gr.grid_subsample_ref(data, labels, voxel=0.5, mode="mean", num_class=4, max_voxels=3)
    assert cut["stats"].tolist() == [3, 5, 3, 2, 3, 2, 4, 0]
    assert cut["inverse"].tolist() == [0, 0, -1, -1, 0, 1, -1, 0, 2, -1, 1, -1]
    assert np.array_equal(cut["data"].view(np.uint32), want[:3].view(np.uint32)) and cut["labels"].tolist() == [1, 0, 0]
    # the projection
    assert gr.project_ref([7, 8, 9], cut["inverse"]).tolist() == [7, 7, -1, -1, 7, 8, -1, 7, 9, -1, 8, -1]
    assert gr.project_ref([7, 8], cut["inverse"]).tolist() == [7, 7, -1, -1, 7, 8, -1, 7, -1, -1, 8, -1]


def test_a_tie_of_the_centre_mode_goes_to_the_lowest_row():
    data = np.array([[0.0, 0.0, 0.0], [0.75, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.25, 0.5]], F)   # rows 1-3 at 0.25 of (0.5, 0.5, 0.5)
    c = gr.grid_subsample_ref(data, None, voxel=1.0, mode="center")
    assert c["stats"].tolist() == [1, 1, 1, 1, 1, 0, 4, 0] and c["voxel_row"].tolist() == [1, -1, -1, -1] and c["labels"] is None


@pytest.mark.parametrize("seed,N,voxel", [(1, 1, 0.1), (2, 777, 0.1), (3, 3000, 0.031), (4, 2000, 0.5)])
def test_reference_voxels_and_inverse_equal_np_unique(seed, N, voxel):
    data, labels = gr.cloud(N, 5, seed, extent=(1.0, 2.0, 0.7), origin=(-3.0, 5.0, 0.25))
    if N > 10:
        data[5, 0], data[N - 1, 2] = np.nan, np.inf
    r = gr.grid_subsample_ref(data, labels, voxel=voxel, mode="mean", num_class=13)
    fin, lo, s, i, n = gr.cells_of(data, voxel)
    cells, inverse, counts = np.unique(i, axis=0, return_inverse=True, return_counts=True)
    V = cells.shape[0]
    assert r["stats"].tolist() == [V, V, n[0], n[1], n[2], int((~fin).sum()), int(counts.max()), 0]
    assert np.array_equal(r["voxel_cell"][:V], cells.astype(np.int32)) and (r["voxel_cell"][V:] == -1).all()
    assert np.array_equal(r["inverse"][fin], inverse.reshape(-1).astype(np.int32)) and (r["inverse"][~fin] == -1).all()
    assert np.array_equal(r["voxel_count"][:V], counts.astype(np.int32)) and not r["voxel_count"][V:].any()
    # the mean is within rounding of numpy's own, and exact where a voxel has one member
    rows = np.nonzero(fin)[0]
    for v in range(0, V, max(1, V // 50)):
        m = rows[inverse.reshape(-1) == v]
        assert r["voxel_row"][v] == m[0]
        assert np.allclose(r["data"][v], data[m].astype(np.float64).mean(axis=0), rtol=1e-5, atol=1e-5)
        if m.size == 1:
            assert np.array_equal(r["data"][v].view(np.uint32), data[m[0]].view(np.uint32))


def test_reference_reports_the_lattice_limit():
    a = np.array([[0.5, 0.5, 0.5], [1048575.5, 1023.5, 1023.5]], F)
    ok = gr.grid_subsample_ref(a, None, voxel=1.0)
    assert ok["stats"].tolist() == [2, 2, 1 << 20, 1024, 1024, 0, 1, 0] and ok["inverse"].tolist() == [0, 1]
    for far in ([1048575.5, 1023.5, 1024.5], [1048576.5, 0.5, 0.5], [3e38, 0.5, 0.5]):
        a[1] = far
        bad = gr.grid_subsample_ref(a, None, voxel=1.0)
        assert bad["stats"][0] == 0 and bad["stats"][1] == 0 and bad["stats"][7] == 1 and bad["inverse"].tolist() == [-1, -1]
    a[0, 0], a[1] = -3e38, [3e38, 0.5, 0.5]                                  # s overflows: the quotient is held at 2^30
    assert gr.grid_subsample_ref(a, None, voxel=1.0)["stats"].tolist() == [0, 0, (1 << 30) + 1, 1, 1, 0, 0, 1]
