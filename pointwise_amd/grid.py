"""Voxel-grid subsampling of a cloud, and voxel predictions carried back to every raw row (include/conv3p.h:
conv3p_grid_subsample_f32, conv3p_grid_project_labels, conv3p_grid_neighbors, conv3p_grid_interpolate_f32 / _i64,
conv3p_grid_interpolate_rings_f32 / _i64, conv3p_grid_normals_f32, conv3p_grid_segments, conv3p_grid_absorb_segments,
conv3p_grid_segments_smooth, conv3p_grid_segment_pool_f32 / _i64 (kernels in csrc/conv3p_grid_smooth.hpp),
conv3p_grid_segment_geometry, conv3p_grid_segment_adjacency, conv3p_grid_merge_segments; kernels in csrc/conv3p_grid.hpp,
csrc/conv3p_grid_interp.hpp, csrc/conv3p_grid_interp_rings.hpp, csrc/conv3p_grid_normals.hpp,
csrc/conv3p_grid_segments.hpp, csrc/conv3p_grid_geometry.hpp and csrc/conv3p_grid_adjacency.hpp).

A raw room or scan has hundreds of thousands to millions of rows at a density that varies by an order of magnitude.  The
first step of a scene pipeline thins it to one row per occupied voxel of a lattice; the model runs on those rows, and
every raw row takes the prediction of its voxel.  include/conv3p.h defines the result bit for bit -- the voxels in
ascending (i_x, i_y, i_z), a voxel's members in ascending row, the mean a chain of float32 additions in that order -- and
tests/grid_ref.py restates it in numpy.

    grid_subsample   one cloud (N, K) -> GridSubsample: data (max_voxels, K), labels, inverse (the voxel of every raw
                     row), voxel_row, voxel_count, voxel_cell, stats
    GridSubsample.project   voxel labels (num_voxels) -> a label per raw row (N) int32, -1 for a row without a voxel
    GridSubsample.neighbors     -> int32 (max_voxels, 27), the voxels of the 3 x 3 x 3 cells around every voxel
    GridSubsample.interpolate   voxel scores (num_voxels, C) -> a label (and a score row) per raw row, blended from the
                     k nearest voxels around the row with inverse-distance weights (tests/grid_interp_ref.py); rings > 1:
                     a row with no voted voxel in its 27 cells searches ring after ring (tests/grid_interp_rings_ref.py)
    GridSubsample.normals       -> GridNormals: a unit normal, a curvature, the sample count and a flag per voxel, from the
                     representatives of the 3 x 3 x 3 cells around it (tests/grid_normals_ref.py)
    GridSubsample.knn           -> GridKnn: the k nearest voxels of every voxel or raw row, an exact k-NN within `rings` cells
                     with a per-query proof that nothing nearer lies further out (include/conv3p_knn.h, kernels in
                     csrc/conv3p_grid_knn.hpp; tests/grid_knn_ref.py); GridKnn.interpolate and GridKnn.normals are
                     interpolate and normals on those neighbours: rows next to a hole, thin and sparse surfaces
    GridSubsample.with_normals  data and those normals side by side, (M, K + 3): what scene_blocks takes in place of data
    GridSubsample.segments      voxel labels -> GridSegments: the connected pieces of one class over the 27-cell table (a
                     lock-free union-find), their root, size, rows and label (tests/grid_segments_ref.py);
                     GridSegments.absorb / GridSubsample.clean_labels: pieces below a size take the label around them;
                     with normals= / features=: smooth segments, joined only where the normals, the curvature and the
                     features agree across the contact -- planes and patches (tests/grid_smooth_ref.py)
    GridSegments.pool           a row of values per voxel -> SegmentPool: exact int64 fixed-point sums per segment, their
                     mean, the class they vote for and that class per voxel (tests/grid_smooth_ref.py)
    GridSegments.geometry       -> SegmentGeometry: per segment the box of its cells and of its representatives, the exact
                     integer moments of its cells, the centroid, the principal axes and the oriented extents
                     (tests/grid_geometry_ref.py): a list of objects from a labelled scan
    GridSegments.adjacency      -> SegmentAdjacency: which segments touch, in CSR form, with the contacts, border voxels
                     and summed direction of every edge and the border counts of every segment
                     (tests/grid_adjacency_ref.py); GridSegments.merge / SegmentAdjacency.merge: segments joined along
                     any selection of pairs -> a GridSegments again
    SegmentAdjacency.agglomerate   -> SegmentAgglomeration: small groups of segments folded into the neighbour they touch
                     most, round after round on the device, with the merged segments, their label per voxel, the log of
                     the merges and the contracted graph (include/conv3p_graph.h, kernels in
                     csrc/conv3p_grid_agglomerate.hpp; tests/grid_agglomerate_ref.py)
    grid_subsample_rooms    many clouds (N, K) with room_start (R + 1) on the device -> GridRoomSubsample: the same, the
                     voxels numbered room after room, plus voxel_room, voxel_start, room_stats

mode="mean" averages every channel over a voxel's members and takes their majority label; mode="center" keeps the member
nearest the voxel's centre as it is.

From a raw room to the model and back:

    g = grid_subsample(room, room_labels, voxel=0.04, num_class=13).trim()
    sb = scene_blocks(g.data, g.labels, num_point=4096, stride=0.5, cover=True, min_points=1).trim()
    pv = BatchProvider(sb.data, sb.index, batch_size, training=False, sort_cloud=True)   # index: the voxel of every row
    scores = SceneScores(g.num_voxels(), num_class, room.device)
    per batch:  points, inp, idx = pv.get_batch_point_cloud();  scores.add(model(points, inp), idx)
    labels = g.project(scores.labels())                              # (N) int32 over the raw rows: its voxel's label
  or
    labels = g.project(g.clean_labels(scores.labels(), num_class, min_size=4))   # speckles of < 4 voxels absorbed first
  or
    labels = g.interpolate(room, scores, k=3, rings=4)               # the 3 nearest voted voxels' scores, blended: rows
                                                                     # of an unvoted voxel are labelled from its neighbours,
                                                                     # up to 4 cells away where the 27 cells around hold none

A model trained on files with normals, fed from a raw scan that has none (xyz + rgb in, blocks of 12 channels out:
xyz, rgb, normal, room-normalised xyz):

    g = grid_subsample(room, room_labels, voxel=0.04, num_class=13).trim()
    nrm = g.normals(viewpoint=(x, y, z))                             # the scanner's position; None: largest component positive
    sb = scene_blocks(g.with_normals(nrm), g.labels, num_point=4096, stride=0.5, cover=True, min_points=1).trim()
    ... as above; the many-clouds result takes a (R, 3) tensor of viewpoints, one per room

A whole area or split, room_start its R + 1 row boundaries on the device: one call, and voxel_start is, as it stands, the
room_start of the tiling (see grid_subsample_rooms).
"""
import math

import numpy as np
import torch

from . import _lib
from ._host import (_LABEL_DTYPES, _call, _fill_empty, _grow, _is_int, _is_tensor, _ptr, _require, _require_int,
                    _require_tensor, _stream, _upload, _view)

_VIEWPOINT = "viewpoint must be None, three finite numbers, or a float32 (1, 3) or (R, 3) tensor on the cloud's device"
_MODES = {"mean": _lib.GRID_MEAN, "center": _lib.GRID_CENTER}
_NO_CPU = "the cloud must live on a HIP device (there is no CPU path)"
_TABLE_MESSAGE = "%s must be a contiguous int32 tensor of the subsampling's shape on its device"


def _require_table(dev, entries, vector=True):
    """The int32 tensors a call reads beside its arguments, (name, tensor, shape) each, are contiguous, on `dev` and of
    that shape; shape None: a vector of at least one entry, or with vector=False of any shape."""
    for name, t, shape in entries:
        _require(_is_tensor(t, torch.int32, shape, dev) and (shape is not None or not vector or (t.dim() == 1 and t.numel() >= 1)),
                 _TABLE_MESSAGE % name)


def _check_viewpoint(grid, viewpoint, dev, rooms):
    """The viewpoint argument of the normals calls checked -> the three numbers to upload, None for a tensor or no
    viewpoint."""
    upload = None
    if viewpoint is not None and not isinstance(viewpoint, torch.Tensor):
        try:
            upload = [float(x) for x in viewpoint]
        except (TypeError, ValueError):
            upload = None
        _require(upload is not None and len(upload) == 3 and all(math.isfinite(x) for x in upload)
                 and all(abs(x) <= float(np.finfo(np.float32).max) for x in upload), _VIEWPOINT)
    elif viewpoint is not None:
        _require(_is_tensor(viewpoint, torch.float32, dev=dev, ndim=2) and viewpoint.shape[1] == 3 and viewpoint.shape[0] >= 1,
                 _VIEWPOINT)
        if viewpoint.shape[0] != 1:
            _require(rooms is not None, "a viewpoint per room needs a GridRoomSubsample")
            _require(viewpoint.shape[0] == grid.voxel_start.numel() - 1,
                     "viewpoint must have one row, or one per room (%d)" % (grid.voxel_start.numel() - 1))
    return upload


class GridSubsample:
    """The outputs of grid_subsample: data float32 (max_voxels, K), labels int32 (max_voxels) or None, inverse int32
    (N) (the voxel number of every raw row; -1 for a non-finite row and for a row of a voxel that max_voxels cut),
    voxel_row (mean: the lowest member row; center: the representative), voxel_count, voxel_cell (max_voxels, 3), stats
    int32 (8) = {emitted voxels, occupied voxels, n_x, n_y, n_z, non-finite rows, largest member count, error}.  Voxels
    past the emitted ones hold data 0, labels -1, voxel_row -1, voxel_count 0, voxel_cell -1."""

    _ROWS = ("data", "labels", "voxel_row", "voxel_count", "voxel_cell")         # per voxel: what a view cuts; it shares the rest
    _SLICED, _SHARED = _ROWS + ("_neigh",), ("inverse", "stats")
    _FILL = (("data", 0), ("labels", -1), ("inverse", -1), ("voxel_row", -1), ("voxel_count", 0), ("voxel_cell", -1), ("stats", 0))

    def __init__(self, num_rows, max_voxels, K, with_labels, device, workspace_bytes=0):
        N, M = int(num_rows), int(max_voxels)
        self.shape = (N, M, int(K), bool(with_labels))
        self.data = torch.empty((M, K), dtype=torch.float32, device=device)
        self.labels = torch.empty((M,), dtype=torch.int32, device=device) if with_labels else None
        self.inverse = torch.empty((N,), dtype=torch.int32, device=device)
        self.voxel_row = torch.empty((M,), dtype=torch.int32, device=device)
        self.voxel_count = torch.empty((M,), dtype=torch.int32, device=device)
        self.voxel_cell = torch.empty((M, 3), dtype=torch.int32, device=device)
        self.stats = torch.zeros((8,), dtype=torch.int32, device=device)
        self.workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device) if workspace_bytes else None

    def num_voxels(self):
        """The number of emitted voxels: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def trim(self):
        """Views of the first num_voxels() voxels, as a GridSubsample (inverse and stats shared)."""
        nv = self.num_voxels()
        return _view(self, GridSubsample, slice(nv), self._SLICED, self._SHARED, shape=(self.shape[0], nv) + self.shape[2:],
                     workspace=None)

    def project(self, voxel_labels, out=None):
        """voxel_labels int32 (M), a label per voxel (the model's, SceneVotes.labels(), ...) -> (N) int32, the label of
        every raw row's voxel; -1 for a row whose inverse is -1 or not below M.  One launch, nothing synchronised on."""
        dev = self.inverse.device
        _require_tensor(voxel_labels, "voxel_labels must be a contiguous int32 (M,) tensor on the cloud's device", torch.int32,
                        dev=dev, ndim=1)
        N, M = self.inverse.numel(), voxel_labels.numel()
        if out is None:
            out = torch.empty((N,), dtype=torch.int32, device=dev)
        _require_tensor(out, "out must be a contiguous int32 (N,) tensor on the cloud's device", torch.int32, (N,), dev)
        _require(dev.type == "cuda", _NO_CPU)
        if N == 0:
            return out
        with torch.cuda.device(dev):
            _call(_lib.load().conv3p_grid_project_labels, _ptr(voxel_labels), self.inverse.data_ptr(), N, M, out.data_ptr(),
                  _stream(dev))
        return out

    def _table(self, dev, M, vector):
        """The check of the tensors the neighbour table is built from and the ring search reads (_require_table) -> the
        many-clouds result's (voxel_room, voxel_start), (None, None) from one cloud."""
        room, start = getattr(self, "voxel_room", None), getattr(self, "voxel_start", None)
        _require_table(dev, (("voxel_cell", self.voxel_cell, (M, 3)), ("stats", self.stats, (8,))) + (
            (("voxel_room", room, (M,)), ("voxel_start", start, None)) if room is not None else ()), vector)
        return room, start

    def neighbors(self):
        """int32 (max_voxels, 27): neigh[v][(dx+1)*9 + (dy+1)*3 + (dz+1)] is the emitted voxel of the cell (i+dx, j+dy,
        l+dz) of voxel v's cell (i, j, l), -1 if there is none; rows past the emitted voxels are -1.  Built on first use
        (one launch, nothing synchronised on: the number of voxels is read on the device) and kept on the object."""
        neigh = getattr(self, "_neigh", None)
        if neigh is not None:
            return neigh
        dev = self.voxel_cell.device
        M = self.voxel_cell.shape[0]
        room, start = self._table(dev, M, vector=False)
        _require(dev.type == "cuda", _NO_CPU)
        neigh = torch.empty((M, 27), dtype=torch.int32, device=dev)
        if M:
            with torch.cuda.device(dev):
                _call(_lib.load().conv3p_grid_neighbors, self.voxel_cell.data_ptr(), _ptr(room), _ptr(start, room is not None),
                      self.stats.data_ptr(), M, start.numel() - 1 if room is not None else 0, neigh.data_ptr(), _stream(dev))
        self._neigh = neigh
        return neigh

    def interpolate(self, data, voxel_scores, k=3, valid_labels=None, return_scores=False, out=None, rings=1,
                    return_ring=False):
        """Scores per voxel -> a label per raw row (N) int32, or (labels, scores float32 (N, C)) with return_scores: the
        scores of the k nearest voxels among the 3 x 3 x 3 cells around the row's own, blended with weights 1 / max(d^2,
        1e-10), d from the raw row to the voxel's representative (include/conv3p.h: conv3p_grid_interpolate_f32, rules 1-5).

        rings in [1, 8]: a row whose 27 cells hold no candidate searches the cells at Chebyshev distance 2, 3, ..., rings
        of its own and is interpolated from the first ring that has one (conv3p_grid_interpolate_rings_f32, rules 6-9: not
        a k-NN, the search stops at the first cube that is not empty; rows labelled at rings=1 keep their bits).
        return_ring: also ring int32 (N), the ring a row was interpolated at, 0 for a row left at -1; the return value is
        labels, (labels, scores), (labels, ring) or (labels, scores, ring), and out= has the same shape.  With rings > 1 or
        return_ring the call goes through the ring entry: ring_stats int64 (9) on the device = {rows that entered the
        fallback, rows interpolated at ring 1, ..., at ring 8}, interp_stats[0] counts the rows interpolated at any ring,
        and the launches are the plain call's, a list kernel and, with rings > 1, the ring kernel (the workspace, an int32
        per row, is kept on the object).

        data is the raw (N, K) tensor the subsampling was given.  voxel_scores: a contiguous float32 (M, C) tensor, C <=
        128 (valid_labels=None: every voxel is a candidate), or a SceneScores, whose exact int64 sums are read as they
        are and whose labels() are the default valid_labels, so a voxel nobody voted for is no candidate.  valid_labels
        int32 (M): voxels with a negative entry are no candidates.  -1 and a zero score row for a row without a voxel or
        without a candidate; interp_stats int64 (3) on the device = {rows interpolated, without a voxel, without a
        candidate}.  out: the labels tensor, or (labels, scores) with return_scores.  The default call is one kernel launch
        behind a 24-byte memset of interp_stats (and the neighbour table's launch on first use); nothing is synchronised on
        in either form."""
        from .scene import SceneScores
        dev = self.inverse.device
        N = self.inverse.numel()
        _require(_is_tensor(data, torch.float32, ndim=2, contiguous=False) and data.shape[1] >= 3,
                 "data must be a float32 (N, K >= 3) tensor, xyz first")
        _require(data.is_contiguous() and data.device == dev, "data must be contiguous and on the cloud's device")
        _require(data.shape[0] == N, "data must have the rows the subsampling was given (inverse has %d)" % N)
        _require_int(k, "k must be an integer in [1, 8]", 1, 8)
        if isinstance(voxel_scores, SceneScores):
            _require(voxel_scores.device == dev, "voxel_scores must live on the cloud's device")
            scores, entry = voxel_scores.scores, "conv3p_grid_interpolate%s_i64"
        else:
            _require_tensor(voxel_scores, "voxel_scores must be a contiguous float32 (M, C) tensor on the cloud's device, or a "
                            "SceneScores", torch.float32, dev=dev, ndim=2)
            scores, entry = voxel_scores, "conv3p_grid_interpolate%s_f32"
        M, C = scores.shape
        _require(1 <= C <= 128, "at most 128 classes (and at least one)")
        _require(M <= self.data.shape[0], "voxel_scores has more rows than the subsampling has voxels")
        if valid_labels is not None:
            _require_tensor(valid_labels, "valid_labels must be a contiguous int32 (M,) tensor on the cloud's device",
                            torch.int32, (M,), dev)
        _require_int(rings, "rings must be an integer in [1, 8]", 1, 8)
        _require(isinstance(return_ring, bool), "return_ring must be a bool")
        parts = 1 + bool(return_scores) + return_ring
        _require(out is None or parts == 1 or (isinstance(out, (tuple, list)) and len(out) == parts),
                 "out must be (labels, scores) with return_scores" if not return_ring else
                 "out must be (labels, ring) with return_ring, (labels, scores, ring) with return_scores too")
        lab = sc = rg = None
        if out is not None:
            lab = out if parts == 1 else out[0]
            sc = out[1] if return_scores else None
            rg = out[parts - 1] if return_ring else None
            _require_tensor(lab, "out labels must be a contiguous int32 (N,) tensor on the cloud's device", torch.int32, (N,), dev)
            _require(not return_scores or _is_tensor(sc, torch.float32, (N, C), dev),
                     "out scores must be a contiguous float32 (N, C) tensor on the cloud's device")
            _require(not return_ring or _is_tensor(rg, torch.int32, (N,), dev),
                     "out ring must be a contiguous int32 (N,) tensor on the cloud's device")
        ringed = rings > 1 or return_ring
        if ringed:
            room, start = self._table(dev, self.data.shape[0], vector=True)
        _require(dev.type == "cuda", _NO_CPU)
        if valid_labels is None and isinstance(voxel_scores, SceneScores):
            valid_labels = voxel_scores.labels()
        if lab is None:
            lab = torch.empty((N,), dtype=torch.int32, device=dev)
        if return_scores and sc is None:
            sc = torch.empty((N, C), dtype=torch.float32, device=dev)
        if getattr(self, "interp_stats", None) is None:
            self.interp_stats = torch.zeros((3,), dtype=torch.int64, device=dev)
        neigh = self.neighbors()
        lib = _lib.load()
        cloud = (_ptr(data), N, data.shape[1], _ptr(self.inverse), _ptr(self.data, M), self.data.shape[1], _ptr(neigh, M))
        votes = (_ptr(scores), M, C, _ptr(valid_labels, M), k)
        if not ringed:
            with torch.cuda.device(dev):
                _call(getattr(lib, entry % ""), *cloud, *votes, _ptr(lab), _ptr(sc), self.interp_stats.data_ptr(), _stream(dev))
            return (lab, sc) if return_scores else lab
        rooms = room is not None and M > 0               # without voxels no row has one: the rooms are not read
        if return_ring and rg is None:
            rg = torch.empty((N,), dtype=torch.int32, device=dev)
        if getattr(self, "ring_stats", None) is None:
            self.ring_stats = torch.zeros((9,), dtype=torch.int64, device=dev)
        ws = _grow(self, "_ring_workspace", int(lib.conv3p_grid_interpolate_rings_workspace_bytes(N)), dev)
        with torch.cuda.device(dev):
            _call(getattr(lib, entry % "_rings"), *cloud, _ptr(self.voxel_cell, M), _ptr(room, rooms), _ptr(start, rooms),
                  start.numel() - 1 if rooms else 0, self.stats.data_ptr(), *votes, rings, _ptr(lab), _ptr(sc), _ptr(rg),
                  self.interp_stats.data_ptr(), self.ring_stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        return tuple(t for t in (lab, sc, rg) if t is not None) if parts > 1 else lab

    def normals(self, viewpoint=None, min_neighbors=6, return_moments=False, out=None):
        """A surface normal and a curvature per voxel -> GridNormals, from the representatives (data[:, :3]) of the 3 x 3
        x 3 cells around every voxel: the moments of the neighbours about the voxel's own representative, the eigenvector
        of the covariance's smallest eigenvalue, curvature = l0 / (l0 + l1 + l2) (include/conv3p.h:
        conv3p_grid_normals_f32, rules R1-R6; tests/grid_normals_ref.py).

        viewpoint: None -- the normal's component of largest magnitude is made positive; a sequence of three finite
        numbers (uploaded as a (1, 3) tensor through pinned memory, on the current stream) or a contiguous float32 (1, 3) tensor on the device -- every normal turned
        towards that point; on a GridRoomSubsample also a contiguous float32 (R, 3) tensor on the device, a point per
        room.  A voxel with fewer than min_neighbors (3 .. 27) occupied cells around it, itself included, gets flags 1 and
        a zero normal; flags 2 marks degenerate moments, -1 the filler rows past the emitted voxels.  return_moments: also
        the float32 (M, 9) moments {m, C_xx, C_xy, C_xz, C_yy, C_yz, C_zz}.  out: a GridNormals of an earlier call with
        the same shapes.  Works on a trimmed object and on many clouds as they stand (the table is per room).  One kernel
        launch behind a 16-byte memset (and the neighbour table's launch on first use), nothing synchronised on."""
        dev = self.data.device
        M, K = self.data.shape
        rooms = getattr(self, "voxel_room", None)
        _require_int(min_neighbors, "min_neighbors must be an integer in [3, 27]", 3, 27)
        _require(isinstance(return_moments, bool), "return_moments must be a bool")
        upload = _check_viewpoint(self, viewpoint, dev, rooms)
        _require(_is_tensor(self.data, torch.float32) and K >= 3, "data must be a contiguous float32 (M, K >= 3) tensor")
        if rooms is not None:
            _require_tensor(rooms, "voxel_room must be a contiguous int32 (M,) tensor on the cloud's device", torch.int32, (M,), dev)
        if out is not None:
            _require(isinstance(out, GridNormals) and out.shape == (M, return_moments) and out.normals.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = GridNormals(M, return_moments, dev)
        if M == 0:
            out.stats.zero_()
            return out
        if upload is not None:
            viewpoint = _upload(torch.tensor([upload], dtype=torch.float32), dev)
        neigh = self.neighbors()
        with torch.cuda.device(dev):
            _call(_lib.load().conv3p_grid_normals_f32, self.data.data_ptr(), K, neigh.data_ptr(), self.stats.data_ptr(),
                  _ptr(rooms), _ptr(viewpoint), viewpoint.shape[0] if viewpoint is not None else 0, M, min_neighbors,
                  out.normals.data_ptr(), out.curvature.data_ptr(), out.samples.data_ptr(), out.flags.data_ptr(),
                  _ptr(out.moments), out.stats.data_ptr(), _stream(dev))
        return out

    def with_normals(self, nrm, curvature=False):
        """data and the normals of normals() side by side -> a contiguous float32 (M, K + 3) tensor, or (M, K + 4) with
        curvature: the K channels of data, then the normal, then the curvature.  This is what scene_blocks /
        scene_blocks_rooms take in place of data: with xyz + rgb in, the blocks come out as xyz, rgb, normal,
        room-normalised xyz -- 12 channels.  The layout is this project's own: the channel order of SceneNN's files is
        not in the reference tree.  Voxels without a normal (flags != 0) carry zeros.  A torch concatenation."""
        M = self.data.shape[0]
        _require(isinstance(nrm, GridNormals), "nrm must be the GridNormals of normals()")
        _require(tuple(nrm.normals.shape) == (M, 3) and nrm.normals.device == self.data.device,
                 "nrm was made for another subsampling (%d voxels here)" % M)
        _require(isinstance(curvature, bool), "curvature must be a bool")
        parts = [self.data, nrm.normals] + ([nrm.curvature[:, None]] if curvature else [])
        return torch.cat(parts, dim=1).contiguous()

    def knn(self, voxel, points=None, query_voxel=None, k=8, rings=2, valid_labels=None, exclude_self=False, out=None):
        """The k nearest voxels of every query -> GridKnn: an exact k-NN among the cells within Chebyshev distance `rings`
        of the query's own cell, in ascending (d2, voxel), with the proof per query of whether those are the k nearest of
        the whole room (include/conv3p_knn.h: conv3p_grid_knn_f32, rules K1-K8; tests/grid_knn_ref.py).

        voxel is the lattice step the subsampling was given (the object does not keep it); it only decides how early a
        query may stop, never which neighbours it gets.  points=None: the voxels query themselves (Q = max_voxels; the
        table GridKnn.normals takes).  points: the raw (N, K) tensor the subsampling was given, query_voxel defaulting to
        inverse; or any float32 (Q, K >= 3) rows with query_voxel int32 (Q), the voxel whose cell each row lies in (a
        negative entry: no neighbours).  k in [1, 16], rings in [1, 8].  valid_labels int32 (M): voxels with a negative
        entry are no neighbours; a SceneScores: its labels().  exclude_self: a query's own voxel is no neighbour.  out: a
        GridKnn of an earlier call with the same shapes.  Works on a trimmed object and on many clouds as they stand
        (rooms share nothing).  Nothing is synchronised on; the launches depend on nothing but rings > 1 (plus the
        neighbour table's launch on first use); the scratch is kept on the object."""
        from .scene import SceneScores
        dev = self.data.device
        M, K = self.data.shape
        _require(isinstance(voxel, (int, float, np.integer, np.floating)) and not isinstance(voxel, bool) and math.isfinite(voxel)
                 and math.isfinite(float(np.float32(voxel))) and float(np.float32(voxel)) > 0, "voxel must be finite and positive")
        voxel = float(np.float32(voxel))
        if points is None:
            _require(query_voxel is None, "query_voxel needs points")
            _require(_is_tensor(self.data, torch.float32) and K >= 3, "data must be a contiguous float32 (M, K >= 3) tensor")
            query, Q = self.data, M
        else:
            _require(_is_tensor(points, torch.float32, ndim=2, contiguous=False) and points.shape[1] >= 3,
                     "points must be a float32 (Q, K >= 3) tensor, xyz first")
            _require(points.is_contiguous() and points.device == dev, "points must be contiguous and on the cloud's device")
            query, Q = points, points.shape[0]
            if query_voxel is None:
                query_voxel = self.inverse
            _require_tensor(query_voxel, "query_voxel must be a contiguous int32 (Q,) tensor on the cloud's device (the default, "
                            "inverse, has %d rows)" % self.inverse.numel(), torch.int32, (Q,), dev)
        _require_int(k, "k must be an integer in [1, 16]", 1, 16)
        _require_int(rings, "rings must be an integer in [1, 8]", 1, 8)
        _require(isinstance(exclude_self, bool), "exclude_self must be a bool")
        if isinstance(valid_labels, SceneScores):
            _require(valid_labels.device == dev, "valid_labels must live on the cloud's device")
        elif valid_labels is not None:
            _require_tensor(valid_labels, "valid_labels must be a contiguous int32 (M,) tensor on the cloud's device, or a "
                            "SceneScores", torch.int32, (M,), dev)
        if out is not None:
            _require(isinstance(out, GridKnn) and out.shape == (Q, k) and out.index.device == dev, "out was made for another shape")
        room, start = self._table(dev, M, vector=True)
        _require(dev.type == "cuda", _NO_CPU)
        if isinstance(valid_labels, SceneScores):
            valid_labels = valid_labels.labels()
            _require(valid_labels.numel() == M, "valid_labels has %d rows, the subsampling %d voxels" % (valid_labels.numel(), M))
        if out is None:
            out = GridKnn(Q, k, dev)
        out.grid, out.voxel_queries = self, points is None
        rooms = room is not None and M > 0
        num_rooms = start.numel() - 1 if rooms else 0
        neigh = self.neighbors()
        lib = _lib.load()
        ws = _grow(self, "_knn_scratch", int(lib.conv3p_grid_knn_scratch_bytes(Q, num_rooms)), dev)
        with torch.cuda.device(dev):
            _call(lib.conv3p_grid_knn_f32, _ptr(query), Q, query.shape[1], _ptr(query_voxel), _ptr(self.data), K, _ptr(neigh),
                  _ptr(self.voxel_cell), _ptr(room, rooms), _ptr(start, rooms), num_rooms, self.stats.data_ptr(), M,
                  _ptr(valid_labels), voxel, k, rings, int(exclude_self), _ptr(out.index), _ptr(out.d2), _ptr(out.count),
                  _ptr(out.ring), _ptr(out.scanned), _ptr(out.certified), out.stats.data_ptr(), ws.data_ptr(), ws.numel(),
                  _stream(dev))
        return out

    def segments(self, voxel_labels=None, num_class=None, connectivity=26, out=None, *, normals=None, max_angle=None,
                 signed=False, max_curvature=None, features=None, max_difference=None):
        """The connected segments of a label per voxel -> GridSegments: voxels are joined when they are neighbours under
        the connectivity (6: faces, 18: and edges, 26: and corners of the 27 cells of neighbors()) and carry the same
        label; a segment's number is its rank by lowest voxel, so for one class it is scipy.ndimage.label's numbering
        minus 1 (include/conv3p.h: conv3p_grid_segments, rules S1-S4; tests/grid_segments_ref.py).

        voxel_labels: a contiguous int32 (L <= rows) tensor on the device, for example scores.labels(); voxels past L,
        negative labels and labels >= num_class are in no segment (-1).  None: every emitted voxel is labelled 0 -- the
        geometric components of the occupied cells.  num_class in [1, 128] is required with labels.  out: a GridSegments
        of an earlier call with the same number of rows.  Works on a trimmed object and on the many-clouds result as they
        stand: the table is per room, so no segment crosses a room, the numbers run room after room and a segment's room
        is voxel_room[root].  g.project(seg.segment) gives the segment number of every raw row.  Seven launches whatever
        the data (and the neighbour table's on first use), nothing synchronised on.

        Smooth segments (include/conv3p.h: conv3p_grid_segments_smooth, rules J1-J5; tests/grid_smooth_ref.py): with
        normals= or features= two neighbours of one label are joined only when the surface is smooth across the contact,
        so a floor and its walls, or two tables that touch, come apart.  normals: the GridNormals of normals() -- its
        normals, flags and curvature are read -- or a contiguous float32 (M, 3) tensor on the device (no flags, and
        max_curvature is then refused); max_angle, in degrees in [0, 180], is required with it, and the pair passes when
        the dot product d of the two normals (|d| unless signed=True) satisfies d >= min_cos with

            min_cos = np.float32(math.cos(math.radians(max_angle)))

        computed on the host; that line is part of the definition.  A voxel without a normal (flags != 0, or a non-finite
        component) joins nobody and is a segment of its own.  max_curvature: both voxels' curvature must be at most it.
        features: a float32 (M, F <= 16) tensor on the device whose rows may be strided (a column slice such as
        g.data[:, 3:6]: its row stride is passed); it requires max_difference >= 0, and every channel of the pair must
        differ by at most that.  The result carries smooth_stats int64 (8) on the device = {candidate pairs, joined,
        refused for a missing normal, by angle, by curvature, by features, labelled voxels without a normal, 0}.  The same
        seven launches behind a 64-byte memset.  geometry(), adjacency(), merge(), pool() and g.project(seg.segment) work
        on it as on any other; absorb() and clean_labels() do not: rule A2 assumes that neighbours of one class share a
        segment.  Small patches are folded in with adjacency().agglomerate() (README: smooth segments).  With all six
        keywords at their defaults the call is the plain one, argument for argument."""
        dev = self.voxel_count.device
        M = self.voxel_count.shape[0]
        L = _check_segment_arguments(voxel_labels, num_class, connectivity, M, dev)
        smooth = _check_smooth_arguments(normals, max_angle, signed, max_curvature, features, max_difference, M, dev)
        _require(_is_tensor(self.voxel_count, torch.int32) and tuple(self.voxel_cell.shape) == (M, 3),
                 "voxel_count must be a contiguous int32 (M,) tensor beside voxel_cell (M, 3)")
        if out is not None:
            _require(isinstance(out, GridSegments) and out.shape == (M,) and out.segment.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = GridSegments(M, dev)
        out._source = (self, voxel_labels, L, 1 if voxel_labels is None else num_class, connectivity)
        if out._merged:                                  # an object merge() wrote into earlier: a plain segmentation again
            del out._merged, out.seg_map, out.merge_stats
        out._smooth = smooth is not None                 # absorb() asks
        if smooth is None:
            out.smooth_stats = None
        elif out.smooth_stats is None:
            out.smooth_stats = torch.zeros((8,), dtype=torch.int64, device=dev)
        if M == 0:
            out.stats.zero_()
            if smooth is not None:
                out.smooth_stats.zero_()
            return out
        lib = _lib.load()
        ws = _grow(out, "workspace", int(lib.conv3p_grid_segments_workspace_bytes(M)), dev)
        neigh = self.neighbors()
        plain = (neigh.data_ptr(), _labels_pointer(voxel_labels, L, out.segment), L, self.voxel_count.data_ptr(),
                 self.stats.data_ptr(), M, out._source[3], connectivity, out.segment.data_ptr(), out.root.data_ptr(),
                 out.size.data_ptr(), out.rows.data_ptr(), out.label.data_ptr(), out.stats.data_ptr())
        with torch.cuda.device(dev):
            if smooth is None:
                _call(lib.conv3p_grid_segments, *plain, ws.data_ptr(), ws.numel(), _stream(dev))
            else:
                _call(lib.conv3p_grid_segments_smooth, *plain, *smooth, out.smooth_stats.data_ptr(), ws.data_ptr(), ws.numel(),
                      _stream(dev))
        return out

    def clean_labels(self, voxel_labels, num_class, min_size, connectivity=26, drop_orphans=False):
        """voxel_labels with every segment of fewer than min_size voxels given the label that surrounds it -> int32 (M):
        segments(voxel_labels, num_class, connectivity).absorb(min_size, drop_orphans).  One pass; run it again on the
        result to absorb what the first pass left (GridSegments.absorb)."""
        _require_int(min_size, "min_size must be a positive integer", 1, 2 ** 31 - 1)
        _require(isinstance(drop_orphans, bool), "drop_orphans must be a bool")
        return self.segments(voxel_labels, num_class, connectivity).absorb(min_size, drop_orphans)


def _check_segment_arguments(voxel_labels, num_class, connectivity, M, dev):
    """The argument checks of GridSubsample.segments -> L, the number of label words (0 without labels)."""
    L = 0
    if voxel_labels is not None:
        _require_tensor(voxel_labels, "voxel_labels must be a contiguous int32 (L,) tensor on the cloud's device, or None",
                        torch.int32, dev=dev, ndim=1)
        L = voxel_labels.numel()
        _require(L <= M, "voxel_labels has more rows than the subsampling has voxels (%d)" % M)
        _require_int(num_class, "num_class must be an integer in [1, %d] with voxel_labels" % _lib.GRID_MAX_CLASS, 1,
                     _lib.GRID_MAX_CLASS)
    else:
        _require(num_class is None or _is_int(num_class, 1, _lib.GRID_MAX_CLASS),
                 "num_class must be None or an integer in [1, %d]" % _lib.GRID_MAX_CLASS)
    _require(_is_int(connectivity, 6, 26) and connectivity in (6, 18, 26), "connectivity must be 6, 18 or 26")
    return L


def _is_real(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and not math.isnan(v)


def _check_smooth_arguments(normals, max_angle, signed, max_curvature, features, max_difference, M, dev):
    """The checks of the six smooth keywords of GridSubsample.segments -> None with all of them at their defaults (the
    plain call), else conv3p_grid_segments_smooth's arguments from normals to max_difference.  The tuple holds addresses
    of the arguments' own tensors: nothing is copied."""
    _require(isinstance(signed, bool), "signed must be a bool")
    if normals is None:
        _require(max_angle is None, "max_angle needs normals=")
        _require(max_curvature is None, "max_curvature needs normals= (a GridNormals)")
        _require(not signed, "signed needs normals=")
    if features is None:
        _require(max_difference is None, "max_difference needs features=")
    if normals is None and features is None:
        return None
    nrm = flags = curv = None
    min_cos = 0.0
    if normals is not None:
        if isinstance(normals, GridNormals):
            nrm, flags, curv = normals.normals, normals.flags, normals.curvature
            _require(_is_tensor(nrm, torch.float32, (M, 3), dev) and _is_tensor(flags, torch.int32, (M,), dev)
                     and _is_tensor(curv, torch.float32, (M,), dev),
                     "normals was made for another subsampling (%d voxels here)" % M)
        else:
            _require_tensor(normals, "normals must be the GridNormals of normals() or a contiguous float32 (M, 3) tensor on "
                            "the cloud's device (%d voxels here)" % M, torch.float32, (M, 3), dev)
            _require(max_curvature is None, "max_curvature needs the curvature of a GridNormals: normals= is a bare tensor")
            nrm = normals
        _require(_is_real(max_angle) and 0 <= max_angle <= 180, "max_angle, in degrees in [0, 180], is required with normals=")
        min_cos = float(np.float32(math.cos(math.radians(max_angle))))
        if max_curvature is None:
            curv = None
        else:
            _require(_is_real(max_curvature) and not math.isnan(float(np.float32(max_curvature))),
                     "max_curvature must be None or a number")
    F = stride = 0
    if features is not None:
        _require(_is_tensor(features, torch.float32, dev=dev, ndim=2, contiguous=False) and features.shape[0] == M
                 and 1 <= features.shape[1] <= 16,
                 "features must be a float32 (M, 1 <= F <= 16) tensor on the cloud's device (%d voxels here)" % M)
        F = features.shape[1]
        stride = features.stride(0) if M > 1 else F      # a single row has no stride to speak of
        _require((F == 1 or features.stride(1) == 1) and stride >= F,
                 "features must have contiguous rows (a column slice of a contiguous tensor is fine)")
        _require(_is_real(max_difference) and max_difference >= 0 and not math.isnan(float(np.float32(max_difference))),
                 "max_difference >= 0 is required with features=")
    return (_ptr(nrm), _ptr(flags), _ptr(curv), min_cos, int(signed), float(max_curvature) if curv is not None else 0.0,
            _ptr(features), F, stride, float(max_difference) if features is not None else 0.0)


def _labels_pointer(voxel_labels, L, stand_in):
    """The labels' address for the C entries, where NULL means "no labels": an EMPTY labels tensor, whose own address may
    be NULL, goes in as another valid address with L = 0, of which nothing is read."""
    if voxel_labels is None:
        return None
    return voxel_labels.data_ptr() if L else stand_in.data_ptr()


class GridSegments:
    """The outputs of GridSubsample.segments, int32 (M) each: segment, the segment number of every voxel (-1: in none);
    root, size (voxels), rows (raw rows: the members' voxel_count summed) and label per segment, -1 / 0 / 0 / -1 past the
    last one; stats int32 (8) on the device = {segments, labelled voxels, unlabelled voxels below the emitted ones, filler
    rows, largest size, largest rows, 0, 0}.  After absorb(): absorbed_label int32 (M), the label per segment behind the
    clean-up, and absorb_stats int64 (4) = {small segments, absorbed, orphans, voxels whose label changed}.  On the object
    merge() returned: seg_map int32 (M), the new number of every segment of the object it was called on (-1 past its
    last one), and merge_stats int32 (4) = {groups, segments, active pairs with a != b, groups of more than one
    segment}.  On the object segments(normals=... / features=...) returned: smooth_stats int64 (8) = {candidate pairs,
    joined, refused for a missing normal, by angle, by curvature, by features, labelled voxels without a normal, 0}."""

    seg_map = merge_stats = None                         # set on the object merge() returns, and on no other
    _merged = False
    smooth_stats = None                                  # set by segments(normals= / features=), and by no other call
    _smooth = False

    def __init__(self, num_voxels, device):
        M = int(num_voxels)
        self.shape = (M,)
        self.segment = torch.empty((M,), dtype=torch.int32, device=device)
        self.root = torch.empty((M,), dtype=torch.int32, device=device)
        self.size = torch.empty((M,), dtype=torch.int32, device=device)
        self.rows = torch.empty((M,), dtype=torch.int32, device=device)
        self.label = torch.empty((M,), dtype=torch.int32, device=device)
        self.stats = torch.zeros((8,), dtype=torch.int32, device=device)
        self.workspace = None
        self.absorbed_label = None
        self.absorb_stats = None
        self._absorb_workspace = None
        self._source = None

    def num_segments(self):
        """The number of segments: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def trim(self):
        """Views of the first num_segments() segment rows, as a GridSegments (segment and stats shared; of a merged object
        seg_map and merge_stats too)."""
        S = self.num_segments()
        t = _view(self, GridSegments, slice(S), ("root", "size", "rows", "label", "absorbed_label"),
                  ("segment", "stats", "absorb_stats"), shape=self.shape, workspace=None, _absorb_workspace=None, _source=None)
        if self._merged:                                 # seg_map is a row per segment of the object merge() was called on
            t._merged, t.seg_map, t.merge_stats = True, self.seg_map, self.merge_stats
        if self._smooth:
            t._smooth, t.smooth_stats = True, self.smooth_stats
        return t

    def absorb(self, min_size, drop_orphans=False, out=None):
        """One clean-up pass -> labels int32 (M): every segment of fewer than min_size voxels takes the label most of the
        (member, tap) pairs around it vote for -- only segments that are not small vote, the lowest class wins a tie --
        and one nobody votes for (an orphan) keeps its label, or takes -1 with drop_orphans (include/conv3p.h:
        conv3p_grid_absorb_segments, rules A1-A4).  On the geometric segmentation (voxel_labels=None) every small segment
        is an orphan, so drop_orphans=True marks floating clusters -1.  min_size=1 returns the labelled input.  Not
        iterated: a small segment among small segments is an orphan; segment the result and absorb again for more.  Sets
        absorbed_label and absorb_stats.  out: a contiguous int32 (M,) tensor.  Six launches whatever the data, nothing
        synchronised on."""
        _require_int(min_size, "min_size must be a positive integer", 1, 2 ** 31 - 1)
        _require(isinstance(drop_orphans, bool), "drop_orphans must be a bool")
        _require(self._source is not None, "absorb works on the object segments() returned, not on its trim()")
        _require(not self._merged, "absorb works on what segments() returned: a merged segment may hold "
                 "several classes, which rule A2 excludes")
        _require(not self._smooth, "absorb works on what the plain segments() returned: in a smooth segmentation neighbours of "
                 "one class lie in different segments, which rule A2 excludes; fold small patches in with adjacency() and merge()")
        grid, voxel_labels, L, num_class, connectivity = self._source
        dev = self.segment.device
        M = self.shape[0]
        _require(out is None or _is_tensor(out, torch.int32, (M,), dev),
                 "out must be a contiguous int32 (M,) tensor on the cloud's device")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = torch.empty((M,), dtype=torch.int32, device=dev)
        if self.absorbed_label is None:
            self.absorbed_label = torch.empty((M,), dtype=torch.int32, device=dev)
            self.absorb_stats = torch.zeros((4,), dtype=torch.int64, device=dev)
        if M == 0:
            self.absorb_stats.zero_()
            return out
        lib = _lib.load()
        ws = _grow(self, "_absorb_workspace", int(lib.conv3p_grid_absorb_workspace_bytes(M)), dev)
        neigh = grid.neighbors()
        with torch.cuda.device(dev):
            _call(lib.conv3p_grid_absorb_segments, neigh.data_ptr(), _labels_pointer(voxel_labels, L, self.segment), L,
                  self.segment.data_ptr(), self.size.data_ptr(), self.label.data_ptr(), self.stats.data_ptr(),
                  grid.stats.data_ptr(), M, num_class, connectivity, min_size, int(drop_orphans), out.data_ptr(),
                  self.absorbed_label.data_ptr(), self.absorb_stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        return out

    def geometry(self, weight="voxels", out=None):
        """Where every segment is, how large and how oriented -> SegmentGeometry, a row per segment (include/conv3p.h:
        conv3p_grid_segment_geometry, rules G1-G8; tests/grid_geometry_ref.py): cell_box, the box of the members' cells;
        box, the box of their representatives (data[:, :3]); moments, the exact integer zeroth, first and second moments
        of the cells about the cell box's low corner; centroid in lattice coordinates; eigenvalues (descending) and axes
        (row k the unit eigenvector of eigenvalues[k], largest component positive) of the cells' covariance; extent, the
        minima and maxima of the cell centres along those axes about the centroid -- the oriented box.

        weight "voxels": every member voxel counts once; "rows": as its voxel_count raw rows, so moments[:, 0] is size or
        rows.  Lattice to metres: the lattice is isotropic, one scale and one shift.  With lo the minimum corner of the
        cloud the subsampling was given (in the many-clouds result: of the room voxel_room[root]) and voxel its step, cell
        i spans [lo + i * voxel, lo + (i + 1) * voxel), a centroid c is the point lo + (c + 0.5) * voxel, an eigenvalue l
        is l * voxel^2 square metres, the axes are directions as they stand, and an extent e is e * voxel metres about the
        centroid (the box of the cell CENTRES: add half a cell on every side to cover the cells).

        Works on the object segments() returned: on the many-clouds result (boxes in each room's own lattice) and on a
        trimmed GridSubsample as they stand, and after absorb() it still describes the segmentation as segmented.
        g.project(seg.segment) gives, for every raw row, the row of these tensors that describes it (-1: none).  out: a
        SegmentGeometry of an earlier call with the same number of rows.  Rows past the last segment hold cell_box
        {0, 0, 0, -1, -1, -1} and 0.  Six launches whatever the data, no workspace, nothing synchronised on."""
        _require(isinstance(weight, str) and weight in _GEOMETRY_WEIGHTS, "weight must be \"voxels\" or \"rows\"")
        _require(self._source is not None, "geometry works on the object segments() returned, not on its trim()")
        grid = self._source[0]
        dev = self.segment.device
        M = self.shape[0]
        _require(_is_tensor(grid.data, torch.float32, dev=dev, ndim=2) and grid.data.shape[0] == M
                 and 3 <= grid.data.shape[1] <= 65536,
                 "the subsampling's data must be a contiguous float32 (M, 3 <= K <= 65536) tensor on the segments' device")
        _require_table(dev, (("voxel_cell", grid.voxel_cell, (M, 3)), ("voxel_count", grid.voxel_count, (M,)),
                             ("stats", grid.stats, (8,)), ("segment", self.segment, (M,)), ("stats", self.stats, (8,))))
        if out is not None:
            _require(isinstance(out, SegmentGeometry) and out.shape == (M,) and out.cell_box.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = SegmentGeometry(M, dev)
        if M == 0:
            out.stats.zero_()
            return out
        with torch.cuda.device(dev):
            _call(_lib.load().conv3p_grid_segment_geometry, grid.data.data_ptr(), grid.data.shape[1],
                  grid.voxel_cell.data_ptr(), grid.voxel_count.data_ptr(), self.segment.data_ptr(), self.stats.data_ptr(),
                  grid.stats.data_ptr(), M, _GEOMETRY_WEIGHTS[weight], out.cell_box.data_ptr(), out.box.data_ptr(),
                  out.moments.data_ptr(), out.centroid.data_ptr(), out.eigenvalues.data_ptr(), out.axes.data_ptr(),
                  out.extent.data_ptr(), out.stats.data_ptr(), _stream(dev))
        return out

    def pool(self, values, weight="voxels", return_mean=True, out=None):
        """A row of values per voxel summed over every segment -> SegmentPool: exact int64 fixed-point sums, their weight,
        the mean and the class the sums vote for, per segment, and that class per voxel (include/conv3p.h:
        conv3p_grid_segment_pool_f32 / _i64, rules P1-P6; tests/grid_smooth_ref.py).

        values: a float32 or int64 (L <= M, C <= 128) tensor on the device, for example nrm.normals, g.data[:, 3:6] or
        SceneScores.scores.  Its rows may be strided -- a column slice of a contiguous tensor goes in as it is, its row
        stride is passed -- but a row's channels must be contiguous.  A float32 value x counts as llrint(x * 2^30); a
        voxel with a non-finite value or one beyond |x| <= 256, and a voxel past L, does not contribute.  int64 values are
        summed as they are (SceneScores' sums are in the same fixed point) and take weight "voxels" only.  weight
        "voxels": every voxel counts once; "rows": as its voxel_count raw rows.  mean = sums / (weights * 2^30), float64,
        None with return_mean=False.  label: the channel with the largest sum, the lowest on a tie, -1 for a segment
        without a contributor or with all sums 0; voxel_label: that per voxel, -1 outside every segment, so
        g.project(pool.voxel_label) labels every raw row by its patch -- the "superpoint" clean-up of a prediction.  Works
        on what segments(), the smooth call and merge() returned, on a trimmed GridSubsample and on the many-clouds
        result; not on a trim() of the segments.  out: a SegmentPool of an earlier call with the same shapes.  Four
        launches whatever the data, no workspace, nothing synchronised on."""
        _require(isinstance(weight, str) and weight in _GEOMETRY_WEIGHTS, "weight must be \"voxels\" or \"rows\"")
        _require(isinstance(return_mean, bool), "return_mean must be a bool")
        _require(self._source is not None, "pool works on the object segments() or merge() returned, not on its trim()")
        grid = self._source[0]
        dev = self.segment.device
        M = self.shape[0]
        _require(_is_tensor(values, (torch.float32, torch.int64), dev=dev, ndim=2, contiguous=False) and values.shape[0] <= M
                 and 1 <= values.shape[1] <= 128,
                 "values must be a float32 or int64 (L <= %d, 1 <= C <= 128) tensor on the segments' device" % M)
        L, C = values.shape
        stride = values.stride(0) if L > 1 else C
        _require((C == 1 or values.stride(1) == 1) and stride >= C,
                 "values must have contiguous rows (a column slice of a contiguous tensor is fine)")
        _require(values.dtype == torch.float32 or weight == "voxels", "int64 values take weight \"voxels\" only")
        _require_table(dev, (("voxel_count", grid.voxel_count, (M,)), ("stats", grid.stats, (8,)), ("segment", self.segment, (M,)),
                             ("stats", self.stats, (8,))))
        if out is not None:
            _require(isinstance(out, SegmentPool) and out.shape == (M, C, return_mean) and out.sums.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = SegmentPool(M, C, return_mean, dev)
        out._segments = self
        if M == 0:
            out.stats.zero_()
            return out
        lib = _lib.load()
        entry = lib.conv3p_grid_segment_pool_f32 if values.dtype == torch.float32 else lib.conv3p_grid_segment_pool_i64
        with torch.cuda.device(dev):
            _call(entry, _ptr(values), L, C, stride, self.segment.data_ptr(), self.stats.data_ptr(),
                  grid.voxel_count.data_ptr(), grid.stats.data_ptr(), M, _GEOMETRY_WEIGHTS[weight], out.sums.data_ptr(),
                  out.weights.data_ptr(), _ptr(out.mean), out.label.data_ptr(), out.voxel_label.data_ptr(),
                  out.stats.data_ptr(), _stream(dev))
        return out

    def adjacency(self, connectivity=None, max_edges=None, out=None):
        """Which segments touch -> SegmentAdjacency: the region adjacency graph of this segmentation in CSR form, with the
        exact number of contacts, the border voxels and the summed direction of every edge, and the border counts of every
        segment (include/conv3p.h: conv3p_grid_segment_adjacency, rules E1-E7; tests/grid_adjacency_ref.py).

        connectivity 6, 18 or 26 decides which taps are contacts; None takes the connectivity the segments were made
        with, but the two are independent: two pieces of one class that only share a corner are segments at 6 and
        neighbours at 26.  max_edges is the number of rows of the edge arrays; None takes 2 * M.  A field in which every
        voxel is its own segment has up to 26 * M directed edges, so the default can overflow: then num_edges() is -1,
        every edge row is filler, border is still exact, and a retry with max_edges=adj.edges_bound() always fits.  out: a
        SegmentAdjacency of an earlier call with the same M and max_edges.

        A policy is a torch expression over the edge arrays, and merge() applies it:

            adj = seg.adjacency().trim()                 # every small segment into the neighbour it touches most
            src = adj.src.long()
            most = torch.zeros_like(seg.size).scatter_reduce(0, src, adj.contacts, "amax")
            merged = adj.merge((seg.size[src] < 4) & (adj.contacts == most[src]))

        Works on the object segments() or merge() returned, on a trimmed GridSubsample and on the many-clouds result as
        they stand: the table is per room, so no edge crosses a room.  5 + 6 b launches, b the bytes of M - 1 (fixed by M,
        whatever the data; and the neighbour table's on first use), nothing synchronised on."""
        _require(connectivity is None or (_is_int(connectivity, 6, 26) and connectivity in (6, 18, 26)),
                 "connectivity must be None, 6, 18 or 26")
        _require(self._source is not None, "adjacency works on the object segments() or merge() returned, not on its trim()")
        grid = self._source[0]
        if connectivity is None:
            connectivity = self._source[4]
        dev = self.segment.device
        M = self.shape[0]
        if max_edges is None:
            max_edges = 2 * M
        _require_int(max_edges, "max_edges must be a non-negative integer below 2^31", 0, 2 ** 31 - 1)
        _require_table(dev, (("voxel_cell", grid.voxel_cell, (M, 3)), ("stats", grid.stats, (8,)),
                             ("segment", self.segment, (M,)), ("stats", self.stats, (8,))))
        if out is not None:
            _require(isinstance(out, SegmentAdjacency) and out.shape == (M, max_edges) and out.start.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = SegmentAdjacency(M, max_edges, dev)
        out._segments = self
        out.connectivity = connectivity
        if M == 0:
            _fill_empty(out)
            return out
        lib = _lib.load()
        ws = _grow(out, "workspace", int(lib.conv3p_grid_adjacency_scratch_bytes(M, max_edges)), dev)
        neigh = grid.neighbors()
        with torch.cuda.device(dev):
            _call(lib.conv3p_grid_segment_adjacency, neigh.data_ptr(), self.segment.data_ptr(), self.stats.data_ptr(),
                  grid.stats.data_ptr(), M, connectivity, max_edges, out.start.data_ptr(), _ptr(out.src), _ptr(out.dst),
                  _ptr(out.contacts), _ptr(out.voxels), _ptr(out.offset), _ptr(out.twin), out.border.data_ptr(),
                  out.stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        return out

    def match(self, truth, num_truth, weight="rows", pred_class=None, truth_class=None, num_class=None, iou=(1, 2),
              max_pairs=None, out=None):
        """This segmentation scored against ground-truth instances -> SegmentMatch: the exact overlap table between
        segments and instances in CSR form and its transpose, the best partner of every segment and instance, the
        one-to-one matching at the IoU threshold, and the integer counters behind panoptic quality, precision / recall and
        coverage (include/conv3p_match.h: c3p_grid_match_segments, rules M1-M10; tests/grid_match_ref.py).

        truth: a contiguous int32 tensor of instance ids in [0, num_truth), -1 for unannotated; one per raw row (N,) with
        weight "rows" -- a row's segment is that of its voxel, grid.inverse -- or one per voxel (M,) with "voxels".  An id
        outside [-1, num_truth) is void and counted in stats[5].  pred_class int32 (M,), a row per segment (seg.label,
        pool.label, ...), truth_class int32 (num_truth,) and num_class (1 .. 128) go together: a segment and an instance
        match only within a class, and an instance whose class is outside [0, num_class) is void (an ignored category).
        With none of the three everything has class 0.  iou = (num, den): a pair matches when its IoU is ABOVE num / den,
        compared exactly; 1 <= num < den <= 32768 and num / den >= 1/2, which makes the matching unique (M8).  max_pairs
        is the number of rows of the pair arrays; None takes M.  If there are more pairs num_pairs() is -1, the sizes stay
        exact, and a retry with max_pairs=m.pairs_bound() always fits.  out: a SegmentMatch of an earlier call with the
        same M, num_truth, max_pairs and num_class.

            m = patches.match(room_instances, T, pred_class=pool.label, truth_class=inst_class, num_class=13)
            m.summary()["pq"]                            # the knobs of segments(), agglomerate() and pool(), compared

        Works on the object segments(), merge() or agglomerate().segments returned, not on its trim(), and on the
        many-clouds result as it stands: segment numbers are global and no segment crosses a room.  8 + 9 b launches, b the
        bytes of max(M, num_truth) - 1 (fixed by the shapes, whatever the data), nothing synchronised on."""
        _require(isinstance(weight, str) and weight in _GEOMETRY_WEIGHTS, "weight must be \"rows\" or \"voxels\"")
        _require_int(num_truth, "num_truth must be an integer from 1 to 2^24", 1, _lib.MATCH_MAX_UNITS)
        _require(self._source is not None,
                 "match works on the object segments(), merge() or agglomerate() returned, not on its trim()")
        grid = self._source[0]
        dev = self.segment.device
        M, N, T = self.shape[0], grid.inverse.numel(), num_truth
        units = N if weight == "rows" else M
        _require_tensor(truth, "truth must be a contiguous int32 (%d,) tensor on the segments' device: an instance id per %s"
                        % (units, "raw row" if weight == "rows" else "voxel"), torch.int32, (units,), dev)
        given = [x is not None for x in (pred_class, truth_class, num_class)]
        _require(all(given) or not any(given), "pred_class, truth_class and num_class go together: all three or none")
        if num_class is None:
            num_class = 1
        else:
            _require_int(num_class, "num_class must be an integer from 1 to %d" % _lib.MATCH_MAX_CLASS, 1, _lib.MATCH_MAX_CLASS)
            _require_tensor(pred_class, "pred_class must be a contiguous int32 (%d,) tensor on the segments' device: a row per "
                            "segment" % M, torch.int32, (M,), dev)
            _require_tensor(truth_class, "truth_class must be a contiguous int32 (%d,) tensor on the segments' device: a row per "
                            "instance" % T, torch.int32, (T,), dev)
        _require(isinstance(iou, (tuple, list)) and len(iou) == 2 and _is_int(iou[0], 1, 32767) and _is_int(iou[1], 2, 32768)
                 and iou[0] < iou[1] and 2 * iou[0] >= iou[1],
                 "iou must be (num, den) with 1 <= num < den <= 32768 and num / den at least 1/2")
        if max_pairs is None:
            max_pairs = M
        _require_int(max_pairs, "max_pairs must be a non-negative integer below 2^31", 0, 2 ** 31 - 1)
        _require(M <= _lib.MATCH_MAX_UNITS and N <= _lib.MATCH_MAX_UNITS, "match takes at most 2^24 voxels and 2^24 rows")
        _require_table(dev, (("inverse", grid.inverse, (N,)), ("stats", grid.stats, (8,)), ("segment", self.segment, (M,)),
                             ("stats", self.stats, (8,))))
        if out is not None:
            _require(isinstance(out, SegmentMatch) and out.shape == (M, T, max_pairs, num_class) and out.start.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = SegmentMatch(M, T, max_pairs, num_class, dev)
        out.iou = (iou[0], iou[1])
        if M == 0 or N == 0:
            _fill_empty(out)
            return out
        lib = _lib.load()
        ws = _grow(out, "workspace", int(lib.c3p_grid_match_scratch_bytes(M, N, T, max_pairs)), dev)
        with torch.cuda.device(dev):
            _call(lib.c3p_grid_match_segments, self.segment.data_ptr(), self.stats.data_ptr(), _ptr(grid.inverse),
                  grid.stats.data_ptr(), truth.data_ptr(), M, N, T, _GEOMETRY_WEIGHTS[weight], _ptr(pred_class),
                  _ptr(truth_class), num_class, iou[0], iou[1], max_pairs, out.pred_size.data_ptr(), out.pred_void.data_ptr(),
                  out.truth_size.data_ptr(), out.truth_missed.data_ptr(), _ptr(out.pair_pred), _ptr(out.pair_truth),
                  _ptr(out.pair_inter), out.start.data_ptr(), out.t_start.data_ptr(), _ptr(out.t_pair),
                  out.best_truth.data_ptr(), out.best_truth_inter.data_ptr(), out.best_truth_union.data_ptr(),
                  out.best_pred.data_ptr(), out.best_pred_inter.data_ptr(), out.best_pred_union.data_ptr(),
                  out.pred_match.data_ptr(), out.truth_match.data_ptr(), out.pred_iou_q30.data_ptr(),
                  out.class_stats.data_ptr(), out.stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        return out

    def merge(self, pair_a, pair_b, select=None, out=None):
        """Segments joined along pairs -> a GridSegments: the pairs (pair_a[p], pair_b[p]) with select[p] != 0 (all of them
        with select=None) and both numbers in [0, S) are collapsed by union-find, transitively; the groups are numbered in
        ascending lowest voxel like any segmentation (include/conv3p.h: conv3p_grid_merge_segments, rules U1-U5).

        pair_a, pair_b: contiguous int32 (P,) tensors on the device, for example adj.src and adj.dst: filler rows (-1) are
        ignored, one direction of an edge is enough, and a == b joins nothing.  select: a contiguous int32 or bool (P,)
        tensor, or None.  The result's size and rows are the sums over a group, its root the group's lowest voxel, its
        label that of the member with the most voxels (the lowest number on a tie); it also carries seg_map int32 (M), the
        group of every old segment (-1 past S), and merge_stats int32 (4) = {groups, segments, active pairs with a != b,
        groups of more than one segment}.  With nothing selected it equals this object to the bit.  geometry(),
        adjacency(), merge() and g.project(merged.segment) work on it as on any other; absorb() does not: a merged
        segment may hold several classes.  out: a GridSegments of the same number of rows, not this one.  Seven launches
        whatever the data, nothing synchronised on."""
        _require(self._source is not None, "merge works on the object segments() or merge() returned, not on its trim()")
        dev = self.segment.device
        M = self.shape[0]
        _require_tensor(pair_a, "pair_a must be a contiguous int32 (P,) tensor on the segments' device", torch.int32, dev=dev, ndim=1)
        P = pair_a.numel()
        _require_tensor(pair_b, "pair_b must be a contiguous int32 (P,) tensor on the segments' device, as long as pair_a",
                        torch.int32, (P,), dev)
        if select is not None:
            _require_tensor(select, "select must be None or a contiguous int32 or bool (P,) tensor on the segments' device",
                            (torch.int32, torch.bool), (P,), dev)
        _require_table(dev, (("segment", self.segment, (M,)), ("root", self.root, (M,)), ("size", self.size, (M,)),
                             ("rows", self.rows, (M,)), ("label", self.label, (M,)), ("stats", self.stats, (8,))))
        if out is not None:
            _require(isinstance(out, GridSegments) and out is not self and out.shape == (M,) and out.segment.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = GridSegments(M, dev)
        out._source = (self._source[0], None, 0, self._source[3], self._source[4])
        out._merged = True
        out._smooth, out.smooth_stats = False, None
        if out.seg_map is None:
            out.seg_map = torch.empty((M,), dtype=torch.int32, device=dev)
            out.merge_stats = torch.zeros((4,), dtype=torch.int32, device=dev)
        if M == 0:
            out.stats.zero_()
            out.merge_stats.zero_()
            return out
        if select is not None and select.dtype == torch.bool:
            select = select.to(torch.int32)
        lib = _lib.load()
        ws = _grow(out, "workspace", int(lib.conv3p_grid_merge_scratch_bytes(M)), dev)
        with torch.cuda.device(dev):
            _call(lib.conv3p_grid_merge_segments, self.segment.data_ptr(), self.root.data_ptr(), self.size.data_ptr(),
                  self.rows.data_ptr(), self.label.data_ptr(), self.stats.data_ptr(), _ptr(pair_a), _ptr(pair_b), _ptr(select),
                  P, M, out.seg_map.data_ptr(), out.segment.data_ptr(), out.root.data_ptr(), out.size.data_ptr(),
                  out.rows.data_ptr(), out.label.data_ptr(), out.stats.data_ptr(), out.merge_stats.data_ptr(), ws.data_ptr(),
                  ws.numel(), _stream(dev))
        return out


def match_summary(class_stats, stats):
    """SegmentMatch.summary()'s arithmetic on the integer counters: class_stats rows {TP, FP, FN, sum of iou_q30 over the
    TP, instances, segments} and the 16 stats, as lists of Python ints -> a dict.  Per class, a list each, None where the
    denominator is 0:

        sq = (sum_iou / 2^30) / TP        rq = TP / (TP + FP / 2 + FN / 2)        pq = (sum_iou / 2^30) / (TP + FP / 2 + FN / 2)
        precision = TP / (TP + FP)        recall = TP / (TP + FN)

    and tp, fp, fn.  mean_pq, mean_sq, mean_rq, mean_precision, mean_recall: the means over the classes where the value
    is defined (None with none).  mcov = stats[8] / 2^30 / stats[3], the mean over the instances of the IoU with their
    best segment; mwcov = stats[9] / 2^30 / stats[10], the same weighted by the instances' sizes.  Plain float division
    of exact integers (all below 2^53 at the sizes the call takes), so a perfect segmentation gives exactly 1.0."""
    one = float(1 << 30)
    div = lambda a, b: (a / b) if b else None
    out = {k: [] for k in ("pq", "sq", "rq", "precision", "recall", "tp", "fp", "fn")}
    for tp, fp, fn, siou, _inst, _segs in class_stats:
        half = 2 * tp + fp + fn                          # twice the denominator of rq: an integer
        out["tp"].append(tp)
        out["fp"].append(fp)
        out["fn"].append(fn)
        out["sq"].append(div(siou / one, tp))
        out["rq"].append(div(2 * tp, half))
        out["pq"].append(div(2 * (siou / one), half))
        out["precision"].append(div(tp, tp + fp))
        out["recall"].append(div(tp, tp + fn))
    for k in ("pq", "sq", "rq", "precision", "recall"):
        have = [x for x in out[k] if x is not None]
        out["mean_" + k] = div(sum(have), len(have))
    out["mcov"] = div(stats[8] / one, stats[3])
    out["mwcov"] = div(stats[9] / one, stats[10])
    return out


class SegmentMatch:
    """The outputs of GridSegments.match (include/conv3p_match.h, rules M1-M10); a unit is a raw row or a voxel, as weight
    said.  Per segment, int32 (M): pred_size, its units on annotated ground; pred_void, its units on void ground;
    best_truth, best_truth_inter, best_truth_union, the instance with the largest IoU (the lowest number on a tie; -1, 0, 0
    with none); pred_match, the instance it matches or -1; pred_iou_q30, floor(IoU * 2^30) of the match, 0 without.  Per
    instance, int32 (T): truth_size, truth_missed (its units in no segment), best_pred, best_pred_inter, best_pred_union,
    truth_match.  The table, a row per pair with at least one common unit in ascending (segment, instance), max_pairs
    rows: pair_pred, pair_truth, pair_inter; start int32 (M + 1), the CSR over the segments; t_start int32 (T + 1) and
    t_pair, the pair rows in ascending (instance, segment); rows past the last pair hold -1, -1, 0, -1.  class_stats int64
    (num_class, 6) = {TP, FP, FN, sum of pred_iou_q30 over the TP, instances with a unit, segments of the class}.  stats
    int64 (16) on the device = {pairs P, B = units in a segment on annotated ground, segments, instances with a unit, void
    units, invalid truth ids, units of an instance in no segment, overflow, coverage sum, weighted coverage sum, sum of
    truth_size, 0 ...}; on overflow (P > max_pairs) {-1, B, ..., 1, 0, 0, sum} with every pair row filler, start and t_start
    all 0, every best / match output -1 / 0 and class_stats 0, the sizes still exact."""

    _FILL = (("pred_size", 0), ("pred_void", 0), ("truth_size", 0), ("truth_missed", 0), ("pair_pred", -1), ("pair_truth", -1),
             ("pair_inter", 0), ("start", 0), ("t_start", 0), ("t_pair", -1), ("best_truth", -1), ("best_truth_inter", 0),
             ("best_truth_union", 0), ("best_pred", -1), ("best_pred_inter", 0), ("best_pred_union", 0), ("pred_match", -1),
             ("truth_match", -1), ("pred_iou_q30", 0), ("class_stats", 0), ("stats", 0))
    _PER_SEGMENT = ("pred_size", "pred_void", "best_truth", "best_truth_inter", "best_truth_union", "pred_match", "pred_iou_q30")
    _PER_INSTANCE = ("truth_size", "truth_missed", "best_pred", "best_pred_inter", "best_pred_union", "truth_match")
    _PER_PAIR = ("pair_pred", "pair_truth", "pair_inter", "t_pair")

    def __init__(self, num_voxels, num_truth, max_pairs, num_class, device):
        M, T, P, C = int(num_voxels), int(num_truth), int(max_pairs), int(num_class)
        self.shape = (M, T, P, C)
        for names, n in ((self._PER_SEGMENT, M), (self._PER_INSTANCE, T), (self._PER_PAIR, P)):
            for name in names:
                setattr(self, name, torch.empty((n,), dtype=torch.int32, device=device))
        self.start = torch.empty((M + 1,), dtype=torch.int32, device=device)
        self.t_start = torch.empty((T + 1,), dtype=torch.int32, device=device)
        self.class_stats = torch.zeros((C, 6), dtype=torch.int64, device=device)
        self.stats = torch.zeros((16,), dtype=torch.int64, device=device)
        self.workspace = None
        self.iou = None

    def num_pairs(self):
        """The number of pairs, -1 on overflow: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def pairs_bound(self):
        """B, the units that lie in a segment and on annotated ground: at least the number of pairs, whatever max_pairs
        was, so a match(max_pairs=pairs_bound()) always fits.  A host read."""
        return int(self.stats[1])

    def overflowed(self):
        """Whether the pairs did not fit max_pairs.  A host read."""
        return int(self.stats[7]) != 0

    def trim(self):
        """Views of the first num_pairs() pair rows (none on overflow), as a SegmentMatch (everything else shared)."""
        P = max(self.num_pairs(), 0)
        return _view(self, SegmentMatch, slice(P), self._PER_PAIR,
                     self._PER_SEGMENT + self._PER_INSTANCE + ("start", "t_start", "class_stats", "stats", "iou"),
                     shape=self.shape[:2] + (P,) + self.shape[3:], workspace=None)

    def summary(self):
        """PQ, SQ, RQ, precision and recall per class and as means, and mCov / mWCov: match_summary on the counters.  A
        host read of class_stats and stats."""
        return match_summary(self.class_stats.cpu().tolist(), self.stats.cpu().tolist())


class SegmentAdjacency:
    """The outputs of GridSegments.adjacency.  Per segment: start int32 (M + 1), row s of the CSR is the edges
    [start[s], start[s + 1]); border int32 (M, 4) = {contacts to other segments, (member, tap) pairs towards a voxel in no
    segment, pairs with no neighbour, surface voxels}.  Per directed edge, in ascending (src, dst), max_edges rows: src,
    dst, contacts (the (voxel, tap) pairs from src into dst: the twin's value), voxels (the voxels of src that touch dst:
    not symmetric), offset int32 (max_edges, 3) (the taps' (dx, dy, dz) summed over the contacts: the negative of the
    twin's; a positive z says dst lies above src), twin (the row of the edge (dst, src)); rows past the last edge hold -1,
    -1, 0, 0, 0, -1.  stats int64 (8) on the device = {edges E, B = the sum of voxels, segments, contacts in all, largest
    degree, largest contacts, 0, 0}, or on overflow (E > max_edges) {-1, B, segments, contacts in all, 0, 0, 1, 0} with
    every edge row filler and start all 0."""

    _FILL = (("start", 0), ("src", -1), ("dst", -1), ("contacts", 0), ("voxels", 0), ("offset", 0), ("twin", -1), ("border", 0),
             ("stats", 0))

    def __init__(self, num_voxels, max_edges, device):
        M, E = int(num_voxels), int(max_edges)
        self.shape = (M, E)
        self.start = torch.empty((M + 1,), dtype=torch.int32, device=device)
        self.src = torch.empty((E,), dtype=torch.int32, device=device)
        self.dst = torch.empty((E,), dtype=torch.int32, device=device)
        self.contacts = torch.empty((E,), dtype=torch.int32, device=device)
        self.voxels = torch.empty((E,), dtype=torch.int32, device=device)
        self.offset = torch.empty((E, 3), dtype=torch.int32, device=device)
        self.twin = torch.empty((E,), dtype=torch.int32, device=device)
        self.border = torch.empty((M, 4), dtype=torch.int32, device=device)
        self.stats = torch.zeros((8,), dtype=torch.int64, device=device)
        self.workspace = None
        self.connectivity = None
        self._segments = None

    def num_edges(self):
        """The number of directed edges, -1 on overflow: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def edges_bound(self):
        """B, the number of (voxel, foreign segment) pairs: at least the number of edges, whatever max_edges was, so an
        adjacency(max_edges=edges_bound()) always fits.  A host read."""
        return int(self.stats[1])

    def overflowed(self):
        """Whether the edges did not fit max_edges.  A host read."""
        return int(self.stats[6]) != 0

    def trim(self):
        """Views of the first num_edges() edge rows (none on overflow), as a SegmentAdjacency (start, border and stats
        shared)."""
        E = max(self.num_edges(), 0)
        return _view(self, SegmentAdjacency, slice(E), ("src", "dst", "contacts", "voxels", "offset", "twin"),
                     ("start", "border", "stats", "connectivity", "_segments"), shape=(self.shape[0], E), workspace=None)

    def merge(self, select=None, out=None):
        """The segments joined along the selected edges -> GridSegments: segments.merge(src, dst, select)."""
        _require(self._segments is not None, "merge works on the object adjacency() returned")
        return self._segments.merge(self.src, self.dst, select, out)

    def agglomerate(self, min_size, weight="voxels", same_label=False, min_contacts=1, max_rounds=8, out=None):
        """Small groups of segments folded into the neighbour they touch most, round after round, on the device ->
        SegmentAgglomeration (include/conv3p_graph.h: conv3p_grid_agglomerate_segments, rules H1-H10;
        tests/grid_agglomerate_ref.py).  The ready-made policy and its fixed point: what a loop of adjacency() and merge()
        with a host read per round gives, without the reads and without a second walk over the voxels -- after a merge
        the new graph is this one with its endpoints renamed and its parallel edges summed.

        A group is small when it has fewer than min_size voxels (weight "voxels") or raw rows ("rows").  Every small
        group proposes to the neighbouring group it has the most contacts with -- one that is not small before any small
        one, the lowest number on a tie -- among those with at least min_contacts contacts and, with same_label, the same
        label (a group's label is that of its member with the most voxels).  A round joins all proposals; the rounds end
        when none is left (converged()) or after max_rounds (1 .. 32).  On a plain segmentation whose adjacency has the
        connectivity the segments were made with, neighbours never share a label, so same_label merges nothing there: it
        is for smooth and merged segmentations and for an adjacency at a wider connectivity.

        The result carries segments, a GridSegments exactly like the one merge() returns on the log (geometry, adjacency,
        merge, pool and g.project work on it); voxel_label, its label per voxel, so g.project(res.voxel_label) is the
        cleaned label per raw row; the log of the merges (log_a, log_b, log_round, log_contacts: a dendrogram, and
        merge(log_a, log_b, log_round < k) is the state after k rounds); and the contracted graph start, src, dst,
        contacts, offset, twin over the result's groups, equal to segments.adjacency()'s at this connectivity.  voxels and
        border are not additive under a merge and are not produced: call result.segments.adjacency() for them.

        Works on the object adjacency() returned and on its trim(), for plain, smooth, merged and many-clouds
        segmentations: no edge crosses a room, so nothing merges across rooms.  An adjacency that overflowed is unusable:
        the result is the identity and stats[6] is 1.  out: a SegmentAgglomeration of an earlier call with the same M and
        max_edges.  15 + 6 max_rounds + 6 b launches, b the bytes of M - 1 (fixed by M and max_rounds, whatever the
        data), nothing synchronised on."""
        _require_int(min_size, "min_size must be a positive integer", 1, 2 ** 31 - 1)
        _require(isinstance(weight, str) and weight in _GEOMETRY_WEIGHTS, "weight must be \"voxels\" or \"rows\"")
        _require(isinstance(same_label, bool), "same_label must be a bool")
        _require_int(min_contacts, "min_contacts must be a positive integer", 1, 2 ** 31 - 1)
        _require_int(max_rounds, "max_rounds must be an integer from 1 to 32", 1, 32)
        seg = self._segments
        _require(seg is not None and seg._source is not None,
                 "agglomerate works on the object adjacency() returned, or on its trim()")
        dev = self.start.device
        M, max_edges = self.shape
        _require_table(dev, (("segment", seg.segment, (M,)), ("root", seg.root, (M,)), ("size", seg.size, (M,)),
                             ("rows", seg.rows, (M,)), ("label", seg.label, (M,)), ("stats", seg.stats, (8,)),
                             ("start", self.start, (M + 1,)), ("src", self.src, (max_edges,)), ("dst", self.dst, (max_edges,)),
                             ("contacts", self.contacts, (max_edges,)), ("offset", self.offset, (max_edges, 3))))
        _require(_is_tensor(self.stats, torch.int64, (8,), dev), "stats must be a contiguous int64 (8,) tensor on the segments' device")
        if out is not None:
            _require(isinstance(out, SegmentAgglomeration) and out.shape == (M, max_edges) and out.start.device == dev
                     and out.segments is not seg, "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = SegmentAgglomeration(M, max_edges, dev)
        res = out.segments
        res._source = (seg._source[0], None, 0, seg._source[3], seg._source[4])
        out.connectivity = self.connectivity
        if M == 0:
            _fill_empty(out)
            res.stats.zero_()
            res.merge_stats.zero_()
            return out
        lib = _lib.load()
        ws = _grow(out, "workspace", int(lib.conv3p_grid_agglomerate_scratch_bytes(M, max_edges)), dev)
        with torch.cuda.device(dev):
            _call(lib.conv3p_grid_agglomerate_segments, seg.segment.data_ptr(), seg.root.data_ptr(), seg.size.data_ptr(),
                  seg.rows.data_ptr(), seg.label.data_ptr(), seg.stats.data_ptr(), self.start.data_ptr(), _ptr(self.src),
                  _ptr(self.dst), _ptr(self.contacts), _ptr(self.offset), self.stats.data_ptr(), M, max_edges, min_size,
                  _GEOMETRY_WEIGHTS[weight], int(same_label), min_contacts, max_rounds, out.log_a.data_ptr(),
                  out.log_b.data_ptr(), out.log_round.data_ptr(), out.log_contacts.data_ptr(), res.seg_map.data_ptr(),
                  res.segment.data_ptr(), res.root.data_ptr(), res.size.data_ptr(), res.rows.data_ptr(), res.label.data_ptr(),
                  res.stats.data_ptr(), res.merge_stats.data_ptr(), out.voxel_label.data_ptr(), out.start.data_ptr(),
                  _ptr(out.src), _ptr(out.dst), _ptr(out.contacts), _ptr(out.offset), _ptr(out.twin), out.stats.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream(dev))
        return out


class SegmentAgglomeration:
    """The outputs of SegmentAdjacency.agglomerate (include/conv3p_graph.h, rules H1-H10).  segments: a GridSegments as
    merge() returns it (seg_map, merge_stats; geometry, adjacency, merge, pool work on it).  voxel_label int32 (M): the
    label of every voxel's group, -1 outside every segment.  The log, int32 (M) each, a row per merge in ascending (round,
    log_a): log_a and log_b, the root segments of the proposer and of its target in the numbers of the INPUT segmentation;
    log_round; log_contacts, the contacts between the two groups at that round; rows past the last hold -1, -1, -1, 0.
    The contracted graph over the result's groups, as SegmentAdjacency states it: start int32 (M + 1); src, dst, contacts,
    twin int32 (max_edges), offset int32 (max_edges, 3).  stats int64 (8) on the device = {groups, segments, rounds that
    had a proposal, merges P, small groups left, of those the ones that still have a candidate, input unusable, edges of
    the contracted graph}."""

    _FILL = (("voxel_label", -1), ("log_a", -1), ("log_b", -1), ("log_round", -1), ("log_contacts", 0), ("start", 0),
             ("src", -1), ("dst", -1), ("contacts", 0), ("offset", 0), ("twin", -1), ("stats", 0))

    def __init__(self, num_voxels, max_edges, device):
        M, E = int(num_voxels), int(max_edges)
        self.shape = (M, E)
        self.segments = GridSegments(M, device)
        self.segments._merged = True
        self.segments.seg_map = torch.empty((M,), dtype=torch.int32, device=device)
        self.segments.merge_stats = torch.zeros((4,), dtype=torch.int32, device=device)
        self.voxel_label = torch.empty((M,), dtype=torch.int32, device=device)
        for name in ("log_a", "log_b", "log_round", "log_contacts"):
            setattr(self, name, torch.empty((M,), dtype=torch.int32, device=device))
        self.start = torch.empty((M + 1,), dtype=torch.int32, device=device)
        for name in ("src", "dst", "contacts", "twin"):
            setattr(self, name, torch.empty((E,), dtype=torch.int32, device=device))
        self.offset = torch.empty((E, 3), dtype=torch.int32, device=device)
        self.stats = torch.zeros((8,), dtype=torch.int64, device=device)
        self.workspace = None
        self.connectivity = None

    def num_groups(self):
        """The number of groups, the segments of the result: a host read (a synchronisation)."""
        return int(self.stats[0])

    def num_rounds(self):
        """The rounds that merged something.  A host read."""
        return int(self.stats[2])

    def converged(self):
        """Whether the fixed point was reached: no small group with a candidate is left (and the input was usable).  A
        host read."""
        s = self.stats.cpu()
        return int(s[5]) == 0 and int(s[6]) == 0

    def trim(self):
        """Views of the log's rows and of the contracted graph's edge rows that are in use, as a SegmentAgglomeration
        (segments, voxel_label, start and stats shared).  One host read."""
        s = self.stats.cpu()
        P, E = int(s[3]), int(s[7])
        t = _view(self, SegmentAgglomeration, slice(P), ("log_a", "log_b", "log_round", "log_contacts"),
                  ("segments", "voxel_label", "start", "stats", "connectivity"), shape=(self.shape[0], E), workspace=None)
        for name in ("src", "dst", "contacts", "offset", "twin"):
            setattr(t, name, getattr(self, name)[:E])
        return t


_GEOMETRY_WEIGHTS = {"voxels": 0, "rows": 1}


class SegmentPool:
    """The outputs of GridSegments.pool, a row per segment: sums int64 (M, C), the fixed-point sums (a float32 value x
    counts as llrint(x * 2^30) times the voxel's weight); weights int64 (M), the summed weights of the contributors; mean
    float64 (M, C) = sums / (weights * 2^30), or None; label int32 (M), the channel with the largest sum, the lowest on a
    tie, -1 without a contributor or with all sums 0; and per voxel voxel_label int32 (M) = label[segment], -1 outside
    every segment.  stats int64 (4) on the device = {voxels that contributed, members that did not, segments with a
    label, segments without}.  Rows past the last segment hold 0 and label -1."""

    def __init__(self, num_voxels, channels, with_mean, device):
        M, C = int(num_voxels), int(channels)
        self.shape = (M, C, bool(with_mean))
        self.sums = torch.empty((M, C), dtype=torch.int64, device=device)
        self.weights = torch.empty((M,), dtype=torch.int64, device=device)
        self.mean = torch.empty((M, C), dtype=torch.float64, device=device) if with_mean else None
        self.label = torch.empty((M,), dtype=torch.int32, device=device)
        self.voxel_label = torch.empty((M,), dtype=torch.int32, device=device)
        self.stats = torch.zeros((4,), dtype=torch.int64, device=device)
        self._segments = None

    def num_segments(self):
        """The number of segments of the segmentation that was pooled: a host read (a synchronisation)."""
        return self._segments.num_segments()

    def trim(self):
        """Views of the first num_segments() rows, as a SegmentPool (voxel_label and stats shared)."""
        S = self.num_segments()
        return _view(self, SegmentPool, slice(S), ("sums", "weights", "mean", "label"), ("voxel_label", "stats", "_segments"),
                     shape=(S,) + self.shape[1:])


class SegmentGeometry:
    """The outputs of GridSegments.geometry, a row per segment: cell_box int32 (M, 6) = {low i_x, i_y, i_z, high i_x, i_y,
    i_z} of the members' cells; box float32 (M, 6), the same of their representatives' xyz; moments int64 (M, 10) = {W, m1
    x y z, m2 xx xy xz yy yz zz} of the cells about cell_box's low corner; centroid float64 (M, 3) in lattice
    coordinates; eigenvalues float64 (M, 3), descending; axes float64 (M, 3, 3), row k the unit eigenvector of
    eigenvalues[k]; extent float64 (M, 6) = {low p_0, p_1, p_2, high p_0, p_1, p_2}, the cell centres along the axes about
    the centroid; stats int32 (4) on the device = {segments, segments of one voxel, segments whose smallest eigenvalue
    is 0 (flat or thinner), 0}.  Rows past the last segment hold cell_box {0, 0, 0, -1, -1, -1} and 0."""

    def __init__(self, num_voxels, device):
        M = int(num_voxels)
        self.shape = (M,)
        self.cell_box = torch.empty((M, 6), dtype=torch.int32, device=device)
        self.box = torch.empty((M, 6), dtype=torch.float32, device=device)
        self.moments = torch.empty((M, 10), dtype=torch.int64, device=device)
        self.centroid = torch.empty((M, 3), dtype=torch.float64, device=device)
        self.eigenvalues = torch.empty((M, 3), dtype=torch.float64, device=device)
        self.axes = torch.empty((M, 3, 3), dtype=torch.float64, device=device)
        self.extent = torch.empty((M, 6), dtype=torch.float64, device=device)
        self.stats = torch.zeros((4,), dtype=torch.int32, device=device)

    def num_segments(self):
        """The number of segments: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def trim(self):
        """Views of the first num_segments() rows, as a SegmentGeometry (stats shared)."""
        S = self.num_segments()
        return _view(self, SegmentGeometry, slice(S), ("cell_box", "box", "moments", "centroid", "eigenvalues", "axes", "extent"),
                     ("stats",), shape=(S,))


class GridKnn:
    """The outputs of GridSubsample.knn: index int32 (Q, k), the k nearest voxels of every query in ascending (d2, voxel),
    -1 past the kept ones; d2 float32 (Q, k), +inf there; count int32 (Q), the kept; ring int32 (Q), the largest Chebyshev
    cell distance among them; scanned int32 (Q), the ring the search stopped at; certified int32 (Q), 1 where the kept
    are proven to be the k nearest of the whole room; stats int64 (16) on the device = {queries with k neighbours, with
    fewer, with none, queries that are not live, certified queries, the sum of scanned, queries by ring 0 .. 8, 0}."""

    def __init__(self, num_queries, k, device):
        Q, k = int(num_queries), int(k)
        self.shape = (Q, k)
        self.index = torch.empty((Q, k), dtype=torch.int32, device=device)
        self.d2 = torch.empty((Q, k), dtype=torch.float32, device=device)
        self.count = torch.empty((Q,), dtype=torch.int32, device=device)
        self.ring = torch.empty((Q,), dtype=torch.int32, device=device)
        self.scanned = torch.empty((Q,), dtype=torch.int32, device=device)
        self.certified = torch.empty((Q,), dtype=torch.int32, device=device)
        self.stats = torch.zeros((16,), dtype=torch.int64, device=device)
        self.grid, self.voxel_queries = None, False

    def num_certified(self):
        """The number of certified queries: the one host read (a synchronisation)."""
        return int(self.stats[4])

    def interpolate(self, voxel_scores, k=None, return_scores=False, out=None):
        """Scores per voxel -> a label per query (Q) int32, or (labels, scores float32 (Q, C)) with return_scores: rule 5
        of GridSubsample.interpolate on the first min(k, count) neighbours of the table (include/conv3p_knn.h:
        conv3p_grid_interpolate_knn_f32 / _i64).  k=None: the table's width.  voxel_scores: a contiguous float32 (M, C)
        tensor, C <= 128, or a SceneScores, whose exact int64 sums are read as they are.  Which voxels are neighbours
        was decided by knn()'s valid_labels.  -1 and a zero score row for a query without a neighbour; interp_stats int64
        (2) on the device = {rows interpolated, rows without a neighbour}.  One kernel launch behind a 16-byte memset,
        nothing synchronised on."""
        from .scene import SceneScores
        dev = self.index.device
        Q, width = self.shape
        if k is None:
            k = width
        _require_int(k, "k must be an integer in [1, %d], the table's width" % width, 1, width)
        if isinstance(voxel_scores, SceneScores):
            _require(voxel_scores.device == dev, "voxel_scores must live on the cloud's device")
            scores, entry = voxel_scores.scores, "conv3p_grid_interpolate_knn_i64"
        else:
            _require_tensor(voxel_scores, "voxel_scores must be a contiguous float32 (M, C) tensor on the cloud's device, or a "
                            "SceneScores", torch.float32, dev=dev, ndim=2)
            scores, entry = voxel_scores, "conv3p_grid_interpolate_knn_f32"
        M, C = scores.shape
        _require(1 <= C <= 128, "at most 128 classes (and at least one)")
        _require(out is None or not return_scores or (isinstance(out, (tuple, list)) and len(out) == 2),
                 "out must be (labels, scores) with return_scores")
        lab = sc = None
        if out is not None:
            lab, sc = (out[0], out[1]) if return_scores else (out, None)
            _require_tensor(lab, "out labels must be a contiguous int32 (Q,) tensor on the cloud's device", torch.int32, (Q,), dev)
            _require(not return_scores or _is_tensor(sc, torch.float32, (Q, C), dev),
                     "out scores must be a contiguous float32 (Q, C) tensor on the cloud's device")
        _require(dev.type == "cuda", _NO_CPU)
        if lab is None:
            lab = torch.empty((Q,), dtype=torch.int32, device=dev)
        if return_scores and sc is None:
            sc = torch.empty((Q, C), dtype=torch.float32, device=dev)
        if getattr(self, "interp_stats", None) is None:
            self.interp_stats = torch.zeros((2,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _call(getattr(_lib.load(), entry), _ptr(self.index), _ptr(self.d2), _ptr(self.count), Q, width, k, _ptr(scores), M, C,
                  _ptr(lab), _ptr(sc), self.interp_stats.data_ptr(), _stream(dev))
        return (lab, sc) if return_scores else lab

    def normals(self, viewpoint=None, min_neighbors=6, return_moments=False, out=None):
        """GridSubsample.normals with the table's neighbours as the samples, in rank order, in place of the 27 cells around
        the voxel -> GridNormals (include/conv3p_knn.h: conv3p_grid_normals_knn_f32, rule R2').  For a table of voxel
        queries only (knn() without points); without exclude_self a voxel is its own first sample, as it is among the 27
        cells.  min_neighbors in [3, 16]; viewpoint, return_moments and out as GridSubsample.normals has them.  One kernel
        launch behind a 16-byte memset, nothing synchronised on."""
        g = self.grid
        _require(g is not None and self.voxel_queries, "normals need the table of voxel queries: knn() without points")
        dev = g.data.device
        M, K = g.data.shape
        rooms = getattr(g, "voxel_room", None)
        _require(self.shape[0] == M, "the table was made for another subsampling (%d voxels here)" % M)
        _require_int(min_neighbors, "min_neighbors must be an integer in [3, 16]", 3, 16)
        _require(isinstance(return_moments, bool), "return_moments must be a bool")
        upload = _check_viewpoint(g, viewpoint, dev, rooms)
        _require(_is_tensor(g.data, torch.float32) and K >= 3, "data must be a contiguous float32 (M, K >= 3) tensor")
        if rooms is not None:
            _require_tensor(rooms, "voxel_room must be a contiguous int32 (M,) tensor on the cloud's device", torch.int32, (M,), dev)
        if out is not None:
            _require(isinstance(out, GridNormals) and out.shape == (M, return_moments) and out.normals.device == dev,
                     "out was made for another shape")
        _require(dev.type == "cuda", _NO_CPU)
        if out is None:
            out = GridNormals(M, return_moments, dev)
        if M == 0:
            out.stats.zero_()
            return out
        if upload is not None:
            viewpoint = _upload(torch.tensor([upload], dtype=torch.float32), dev)
        with torch.cuda.device(dev):
            _call(_lib.load().conv3p_grid_normals_knn_f32, g.data.data_ptr(), K, self.index.data_ptr(), self.count.data_ptr(),
                  self.shape[1], g.stats.data_ptr(), _ptr(rooms), _ptr(viewpoint),
                  viewpoint.shape[0] if viewpoint is not None else 0, M, min_neighbors, out.normals.data_ptr(),
                  out.curvature.data_ptr(), out.samples.data_ptr(), out.flags.data_ptr(), _ptr(out.moments),
                  out.stats.data_ptr(), _stream(dev))
        return out


class GridNormals:
    """The outputs of GridSubsample.normals: normals float32 (M, 3), unit vectors or 0; curvature float32 (M) in [0,
    1/3]; samples int32 (M), the occupied cells among the 27 around the voxel; flags int32 (M): 0 a normal, 1 too few
    samples, 2 degenerate moments, -1 a filler row; moments float32 (M, 9) or None; stats int32 (4) on the device =
    {voxels with a normal, too few samples, degenerate, filler}."""

    def __init__(self, num_voxels, with_moments, device):
        M = int(num_voxels)
        self.shape = (M, bool(with_moments))
        self.normals = torch.empty((M, 3), dtype=torch.float32, device=device)
        self.curvature = torch.empty((M,), dtype=torch.float32, device=device)
        self.samples = torch.empty((M,), dtype=torch.int32, device=device)
        self.flags = torch.empty((M,), dtype=torch.int32, device=device)
        self.moments = torch.empty((M, 9), dtype=torch.float32, device=device) if with_moments else None
        self.stats = torch.zeros((4,), dtype=torch.int32, device=device)

    def count(self):
        """The number of voxels with a normal: the one host read (a synchronisation)."""
        return int(self.stats[0])


def _subsample(many, data, room_start, labels, voxel, mode, num_class, max_voxels, out):
    """The body of grid_subsample and, with `many`, of grid_subsample_rooms: every check in the order the calls have always
    made them, the max_voxels default, out reuse, the workspace, the nothing-to-launch fill and the launch.  The rooms
    contribute their room_start, its checks, and their extra outputs and arguments."""
    _require(_is_tensor(data, torch.float32, ndim=2, contiguous=False) and data.shape[1] >= 3,
             "data must be a float32 (N, K >= 3) tensor, xyz first")
    dev = data.device
    N, K = data.shape
    _require(data.is_contiguous(), "data must be contiguous")
    if labels is not None:
        _require(isinstance(labels, torch.Tensor) and labels.dtype in _LABEL_DTYPES, "labels must be uint8, int32 or int64")
        _require_tensor(labels, "labels must be a contiguous (N,) tensor on the data's device", _LABEL_DTYPES, (N,), dev)
    _require(isinstance(voxel, (int, float)) and not isinstance(voxel, bool) and math.isfinite(voxel)
             and math.isfinite(float(np.float32(voxel))) and float(np.float32(voxel)) > 0, "voxel must be finite and positive")
    voxel = float(np.float32(voxel))
    _require(isinstance(mode, str) and mode in _MODES, "mode must be \"mean\" or \"center\"")
    if labels is not None and mode == "mean":
        _require_int(num_class, "num_class must be an integer in [1, %d] for the majority label" % _lib.GRID_MAX_CLASS, 1,
                     _lib.GRID_MAX_CLASS)
    else:
        _require(num_class is None or _is_int(num_class, -math.inf, math.inf), "num_class must be an integer or None")
    _require(N <= _lib.GRID_MAX_ROWS, "at most 2^24 rows")
    _require(K <= 65536, "at most 65536 channels")
    if max_voxels is None:
        max_voxels = N
    _require_int(max_voxels, "max_voxels must be a non-negative integer", 0, 2 ** 31 - 1)
    cls, shape = GridSubsample, (N, max_voxels, K, labels is not None)
    if many:
        _require(_is_tensor(room_start, torch.int32, dev=dev, ndim=1) and room_start.numel() >= 1,
                 "room_start must be a contiguous int32 (R + 1,) tensor on the data's device")
        R = room_start.numel() - 1
        _require(R <= _lib.GRID_ROOMS_MAX_ROOMS, "at most 65536 rooms")
        cls, shape = GridRoomSubsample, shape + (R,)
    if out is not None:
        _require(isinstance(out, cls) and out.shape == shape and out.data.device == dev, "out was made for another shape")
    _require(dev.type == "cuda", "data must live on a HIP device (there is no CPU path)")   # after every other check
    lib = _lib.load()
    need = (lib.conv3p_grid_subsample_rooms_workspace_bytes(N, R, max_voxels) if many else
            lib.conv3p_grid_subsample_workspace_bytes(N, max_voxels))
    if out is None:
        out = GridRoomSubsample(N, R, *shape[1:4], dev, need) if many else GridSubsample(*shape, dev, need)
    elif need:
        _grow(out, "workspace", need, dev)
    out._neigh = None                        # the neighbour table of an earlier call's voxels
    if N == 0 or max_voxels == 0 or (many and R == 0):   # nothing is launched, so nothing is written
        _fill_empty(out)
        return out
    ws = out.workspace
    with torch.cuda.device(dev):
        _call(lib.conv3p_grid_subsample_rooms_f32 if many else lib.conv3p_grid_subsample_f32, data.data_ptr(), _ptr(labels),
              *((room_start.data_ptr(), N, R) if many else (N,)), K, _LABEL_DTYPES[labels.dtype] if labels is not None else 0,
              voxel, _MODES[mode], num_class if num_class is not None else 0, max_voxels, out.data.data_ptr(), _ptr(out.labels),
              out.voxel_row.data_ptr(), out.voxel_count.data_ptr(), out.voxel_cell.data_ptr(),
              *((out.voxel_room.data_ptr(), out.voxel_start.data_ptr()) if many else ()), out.inverse.data_ptr(),
              *((out.room_stats.data_ptr(),) if many else ()), out.stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    return out


class GridRoomSubsample(GridSubsample):
    """The outputs of grid_subsample_rooms: everything a GridSubsample has -- inverse holds GLOBAL voxel numbers, voxel_row
    GLOBAL rows, voxel_cell the cell in the room's own lattice -- and voxel_room int32 (max_voxels), the room of every
    voxel (-1 past the emitted ones), voxel_start int32 (R + 1), the prefix of the emitted voxels per room
    (voxel_start[R] = stats[0]), and room_stats int32 (R, 8), the single-cloud stats of every room.  stats int32 (8) =
    {emitted voxels, occupied voxels, R, rooms with an emitted voxel, rooms with an error of their own, non-finite rows
    inside the rooms, largest member count, error bits: 1 a room's lattice too large, 2 room_start malformed, 4 too
    many cells in all}.  project is GridSubsample's: one call serves every room."""

    _SLICED, _SHARED = GridSubsample._SLICED + ("voxel_room",), GridSubsample._SHARED + ("voxel_start", "room_stats")
    _FILL = GridSubsample._FILL + (("voxel_room", -1), ("voxel_start", 0), ("room_stats", 0))

    def __init__(self, num_rows, num_rooms, max_voxels, K, with_labels, device, workspace_bytes=0):
        GridSubsample.__init__(self, num_rows, max_voxels, K, with_labels, device, workspace_bytes)
        R = int(num_rooms)
        self.shape = self.shape + (R,)
        self.voxel_room = torch.empty((int(max_voxels),), dtype=torch.int32, device=device)
        self.voxel_start = torch.zeros((R + 1,), dtype=torch.int32, device=device)
        self.room_stats = torch.zeros((R, 8), dtype=torch.int32, device=device)

    def trim(self):
        """Views of the first num_voxels() voxels, as a GridRoomSubsample (inverse, stats, voxel_start and room_stats
        shared)."""
        nv = self.num_voxels()
        return _view(self, GridRoomSubsample, slice(nv), self._SLICED, self._SHARED,
                     shape=(self.shape[0], nv) + self.shape[2:], workspace=None)

    def room(self, r):
        """Views of room r's emitted voxels, as a GridSubsample whose stats is room_stats[r].  Reads voxel_start on the
        host (a synchronisation).  inverse is shared: it holds global voxel numbers, so subtract voxel_start[r] to index
        the view."""
        R = self.voxel_start.numel() - 1
        _require_int(r, "r must be a room number in [0, R)", 0, R - 1)
        a, b = (int(x) for x in self.voxel_start[r:r + 2].cpu())
        return _view(self, GridSubsample, slice(a, b), GridSubsample._ROWS, ("inverse",),        # _neigh holds global numbers: not the view's
                     shape=(self.shape[0], b - a) + self.shape[2:4], stats=self.room_stats[r], workspace=None)


def grid_subsample_rooms(data, room_start, labels=None, voxel=0.05, mode="mean", num_class=None, max_voxels=None, out=None):
    """Many clouds in one call -> GridRoomSubsample (include/conv3p.h: conv3p_grid_subsample_rooms_f32).

    data float32 (N, K >= 3) holds the rooms' rows one room after the other; room_start, a contiguous int32 (R + 1,)
    tensor ON THE DEVICE, gives room r the rows [room_start[r], room_start[r + 1]); rows outside belong to no room
    (inverse -1).  Every room is subsampled as grid_subsample does it on the room's own rows -- its own lo and lattice,
    so rooms that overlap in space share no voxel -- and the voxels are numbered room after room; max_voxels (None:
    N) cuts by that global number.  labels, voxel, mode, num_class as grid_subsample; at most 2^24 rows summed over the
    rooms, at most 65536 rooms.  Nothing is synchronised on; stats[7] reports what only the device knows (bit 0 a
    room's lattice past 2^20 cells along an axis or 2^40 in all: that room emits nothing; bit 1 room_start malformed;
    bit 2 more than 2^40 cells over all rooms: nothing emitted).

    voxel_start is the tiling's room_start, and the untrimmed data works, since rows from room_start[R] on belong to
    no room -- a whole area from raw rows to blocks without a host read:

        g = grid_subsample_rooms(area, room_start, area_labels, voxel=0.04, num_class=13)
        sb = scene_blocks_rooms(g.data, g.voxel_start, g.labels, num_point=4096, stride=0.5, cover=True, min_points=1,
                                max_blocks=...)
        scores = SceneScores(g.shape[1], num_class, area.device)       # or g.num_voxels() rows, the one host read
        ...
        labels = g.project(scores.labels())                            # (N) int32 over the raw rows of every room
    """
    return _subsample(True, data, room_start, labels, voxel, mode, num_class, max_voxels, out)


def grid_subsample(data, labels=None, voxel=0.05, mode="mean", num_class=None, max_voxels=None, out=None):
    """One cloud -> GridSubsample, by the eight steps of include/conv3p.h (conv3p_grid_subsample_f32).

    data float32 (N, K >= 3), xyz first; labels (N) uint8 / int32 / int64 or None.  voxel, the lattice step, is taken
    as float32.  mode "mean": every channel averaged over the voxel's members in ascending row, the label their majority
    among 0 <= l < num_class (num_class in [1, 128], required with labels); mode "center": the member nearest the
    voxel's centre, copied with its label (num_class is not used).  max_voxels=None means N, which never cuts.  out: a
    GridSubsample of an earlier call with the same shapes, written into.  Nothing is synchronised on; stats[7] != 0
    reports a lattice of more than 2^20 cells along an axis or 2^40 in all (nothing emitted, inverse all -1)."""
    return _subsample(False, data, None, labels, voxel, mode, num_class, max_voxels, out)
