"""A room to model-sized blocks and block predictions back to a label per room point (include/conv3p.h:
conv3p_scene_blocks_f32, conv3p_scene_vote, conv3p_scene_vote_labels; kernels in csrc/conv3p_scene.hpp -- and the
covering mode conv3p_scene_blocks_cover_f32 with the votes by summed probabilities conv3p_scene_vote_scores_f32,
conv3p_scene_score_labels; kernels in csrc/conv3p_scene_cover.hpp).

The segmentation model takes (B, 4096, 9) blocks (scene_seg/s3dis_provider.py:9, :62-63) and the reference only reads
blocks that PointNet's indoor3d_util prepared (room2blocks_plus_normalized): shift the room to its minimum, tile x-y
with block x block cells every stride, drop cells of fewer than 100 points, sample num_point rows a cell, centre x, y
on the block, append the room-normalised xyz.  That partition is not in the reference tree; include/conv3p.h defines it
bit for bit and tests/scene_ref.py restates it in numpy.  The evaluation loops count accuracy per block row
(eval_and_log_scene_seg_s3dis.py:83-93); SceneVotes carries block predictions back to the room's own rows.

    scene_blocks   one room (N, K) -> SceneBlocks: data (max_blocks, P, K + 3), labels, index (the room row of every
                   emitted row), block_cell, block_count, stats
    scene_blocks_rooms   many rooms (an area, a test split) in ONE call -> SceneRoomBlocks: the concatenation of the
                   single-room results, index holding GLOBAL rows, plus block_room, room_blocks, room_stats
    SceneVotes     votes (N, C) int32 accumulated from (pred, index) pairs -> labels(), counts()
    SceneScores    scores (N, C) int64, the blocks' class probabilities summed in fixed point from (logits, index)
                   pairs -> labels(), counts()

For an evaluation, scene_blocks(..., cover=True) splits a crowded cell into parts instead of sampling it, so every row
of a kept cell is emitted once (and min_points=1 keeps every cell), and SceneScores.add(acts[4], rows) takes the
model's last activations where SceneVotes.add takes their argmax.

From a room to the model and back:

    sb = scene_blocks(room, room_labels, num_point=4096, stride=0.5, step=epoch).trim()
    pv = BatchProvider(sb.data, sb.index, batch_size, training=False, sort_cloud=True)   # index rides as the labels
    votes = SceneVotes(room.shape[0], num_class, room.device)
    per batch:  points, inp, rows = pv.get_batch_point_cloud()       # rows: the room row of every sorted point
                pred = model(points, inp).argmax(-1)                  # e.g. SegmentationHead.evaluate(...)[0]
                votes.add(pred, rows)
    labels = votes.labels()                                          # (N) int32, -1 where no block covered the row

Many rooms at once -- an S3DIS area, SceneNN's test split -- with rows (N, K) the rooms one after the other and
room_start their R + 1 boundaries; one call, one host read, no torch.cat, and one vote table over the N global rows:

    sb = scene_blocks_rooms(rows, room_start, num_point=4096, stride=0.5, min_points=1, cover=True).trim()
    pv = BatchProvider(sb.data, sb.index, batch_size, training=False, sort_cloud=True)
    scores = SceneScores(rows.shape[0], num_class, rows.device)
    per batch:  points, inp, idx = pv.get_batch_point_cloud();  scores.add(model(points, inp), idx)
    labels = scores.labels()                                         # (N) int32 over the global rows of all rooms
    conv3p_seg_confusion over (row_labels, labels): one confusion matrix of the N rows of all rooms

The trimmed data / labels are what BatchProvider(data, labels, ...) takes for training; passing `index` as its
per-point int32 "labels" instead carries the room rows through the provider's sort.  A room resampled with another
`step` draws other rows for the slots that are draws: the scene providers' only augmentation.
"""
import math

import numpy as np
import torch

from . import _lib
from ._host import (_LABEL_DTYPES, _call, _fill_empty, _grow, _is_tensor, _ptr, _require, _require_int, _require_tensor,
                    _stream, _upload, _view)


def default_max_blocks(num_rows, block=1.0, stride=1.0, min_points=100, num_point=None):
    """The bound scene_blocks uses for max_blocks=None, from the shape alone (no look at the data, no sync): a kept
    cell has at least max(1, min_points) members and a row is a member of at most m x m cells, m = ceil(block /
    stride) + 1, so there are at most num_rows m^2 // max(1, min_points) kept cells -- and never more than
    SCENE_MAX_CELLS.  It is a loose bound (outputs are allocated for it): pass max_blocks when the room's extent is
    known.  With num_point given it is the covering mode's bound: the sum of ceil(n_c / P) over the kept cells is at
    most their number plus (the sum of n_c) // P, and the counts sum to at most num_rows m^2."""
    m = int(math.ceil(float(block) / float(stride))) + 1
    if num_point is None:
        return max(1, min(_lib.SCENE_MAX_CELLS, int(num_rows) * m * m // max(1, int(min_points))))
    return max(1, min(_lib.SCENE_MAX_CELLS, int(num_rows) * m * m // max(1, int(min_points)))
               + int(num_rows) * m * m // int(num_point))


class SceneBlocks:
    """The outputs of scene_blocks: data float32 (max_blocks, P, K + 3), points = data[..., 0:3] (a view), labels int32
    (max_blocks, P) or None, index int32 (max_blocks, P), block_cell / block_count int32 (max_blocks), stats int32 (8) =
    {emitted blocks, kept cells, nbx, nby, non-finite rows, cells with 0 < count < min_points, 0, error}.  Blocks past
    the emitted ones hold data 0, labels -1, index -1, block_cell -1, block_count 0.  In the covering mode a block is a
    part of its cell, block_count its distinct members (the first slots) and stats[6] the blocks the room needs."""

    _SLICED, _SHARED = ("data", "labels", "index", "block_cell", "block_count"), ("stats",)     # what a view cuts / shares
    _FILL = (("data", 0), ("labels", -1), ("index", -1), ("block_cell", -1), ("block_count", 0), ("stats", 0))

    def __init__(self, max_blocks, num_point, K, with_labels, device, workspace_bytes=0):
        B, P = int(max_blocks), int(num_point)
        self.shape = (B, P, int(K), bool(with_labels))
        self.data = torch.empty((B, P, K + 3), dtype=torch.float32, device=device)
        self.labels = torch.empty((B, P), dtype=torch.int32, device=device) if with_labels else None
        self.index = torch.empty((B, P), dtype=torch.int32, device=device)
        self.block_cell = torch.empty((B,), dtype=torch.int32, device=device)
        self.block_count = torch.empty((B,), dtype=torch.int32, device=device)
        self.stats = torch.zeros((8,), dtype=torch.int32, device=device)
        self.workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device) if workspace_bytes else None

    @property
    def points(self):
        return self.data[..., 0:3]

    def num_blocks(self):
        """The number of emitted blocks: the one host read (a synchronisation)."""
        return int(self.stats[0])

    def blocks_needed(self):
        """The covering mode's stats[6], the blocks the room needs (a host read): more than num_blocks() when max_blocks
        cut the room.  0 from the plain mode."""
        return int(self.stats[6])

    def trim(self):
        """Views of the first num_blocks() blocks, as a SceneBlocks (stats shared)."""
        nb = self.num_blocks()
        return _view(self, SceneBlocks, slice(nb), self._SLICED, self._SHARED, shape=(nb,) + self.shape[1:], workspace=None)


def _as_f32(x):
    return float(np.float32(x))


def _host_room_start(room_start, N):
    """The checks of a room_start the host can read (a Python sequence, numpy array or CPU tensor) -> it as int64."""
    if isinstance(room_start, torch.Tensor):
        _require(room_start.dtype in (torch.int32, torch.int64), "room_start must hold integers (int32 or int64)")
        rs = room_start.numpy()
    else:
        try:
            rs = np.asarray(room_start)
        except Exception:
            rs = None
        _require(rs is not None and rs.dtype.kind in "iu", "room_start must hold integers")
    _require(rs.ndim == 1 and rs.size >= 1, "room_start must have R + 1 >= 1 entries")
    rs = rs.astype(np.int64)
    _require(int(rs[0]) >= 0 and int(rs[-1]) <= N and bool(np.all(np.diff(rs) >= 0)), "room_start must ascend inside [0, N]")
    _require(rs.size < 2 or int(np.diff(rs).max()) <= _lib.SCENE_MAX_ROWS, "at most 2^24 rows a room")
    return rs


def _blocks(many, data, room_start, labels, num_point, block, stride, min_points, max_blocks, seed, step, out, cover):
    """The body of scene_blocks and, with `many`, of scene_blocks_rooms: every check in the order the calls have always
    made them, the max_blocks default, out reuse, the workspace, the nothing-to-launch fill and the launch.  The rooms
    contribute their room_start, their limits and messages, and their extra outputs and arguments."""
    _require(_is_tensor(data, torch.float32, ndim=2, contiguous=False) and data.shape[1] >= 3,
             "data must be a float32 (N, K >= 3) tensor, xyz first")
    dev = data.device
    N, K = data.shape
    _require(data.is_contiguous(), "data must be contiguous")
    R, rs = None, None
    if many and isinstance(room_start, torch.Tensor) and room_start.device.type != "cpu":
        _require(room_start.dtype == torch.int32 and room_start.dim() == 1 and room_start.numel() >= 1
                 and room_start.is_contiguous() and room_start.device == dev,
                 "a device room_start must be a contiguous int32 (R + 1,) tensor on the data's device")
        R = room_start.numel() - 1
    elif many:
        rs = _host_room_start(room_start, N)
        R = rs.size - 1
    _require(not many or R <= _lib.SCENE_ROOMS_MAX_ROOMS, "at most 65536 rooms")
    if labels is not None:
        _require(isinstance(labels, torch.Tensor) and labels.dtype in _LABEL_DTYPES, "labels must be uint8, int32 or int64")
        _require_tensor(labels, "labels must be a contiguous (N,) tensor on the data's device", _LABEL_DTYPES, (N,), dev)
    _require_int(num_point, "num_point must be an integer in [1, %d]" % _lib.SCENE_MAX_NUM_POINT, 1, _lib.SCENE_MAX_NUM_POINT,
                 allow_bool=True)
    for name, v in (("block", block), ("stride", stride)):
        _require(isinstance(v, (int, float)) and math.isfinite(v) and _as_f32(v) > 0, "%s must be finite and positive" % name)
    block, stride = _as_f32(block), _as_f32(stride)
    _require(stride <= block <= _as_f32(np.float32(2) * np.float32(stride)), "block must lie in [stride, 2 stride]")
    if many:
        _require(N <= _lib.SCENE_ROOMS_MAX_ROWS, "at most 2^26 rows")
    else:
        _require(N <= _lib.SCENE_MAX_ROWS, "at most 2^24 room rows")
    _require(K <= 65536, "at most 65536 channels")
    _require_int(min_points, "min_points must be an int32", -2 ** 31, 2 ** 31 - 1, allow_bool=True)
    _require(isinstance(cover, bool), "cover must be a bool")
    if max_blocks is None:
        bound = (block, stride, min_points, num_point if cover else None)
        max_blocks = (default_max_blocks(N, *bound) if not many else _rooms_bound(N, R, *bound) if rs is None else
                      default_max_blocks_rooms(np.diff(rs).tolist(), *bound))
    _require_int(max_blocks, "max_blocks must be a non-negative integer", 0, 2 ** 31 - 1, allow_bool=True)
    _require(0 <= int(seed) < 2 ** 64 and 0 <= int(step) < 2 ** 64, "seed and step must fit 64 unsigned bits")
    cls, shape = SceneRoomBlocks if many else SceneBlocks, (max_blocks, num_point, K, labels is not None) + ((R,) if many else ())
    if out is not None:
        _require(isinstance(out, cls) and out.shape == shape and out.data.device == dev, "out was made for another shape")
    _require(dev.type == "cuda", "data must live on a HIP device (there is no CPU path)")   # after every other check
    lib = _lib.load()
    if many:
        need = lib.conv3p_scene_blocks_rooms_workspace_bytes(N, R, num_point, max_blocks, block, stride, int(cover))
        call = lib.conv3p_scene_blocks_rooms_f32
    else:
        nbytes, call = ((lib.conv3p_scene_blocks_cover_workspace_bytes, lib.conv3p_scene_blocks_cover_f32) if cover else
                        (lib.conv3p_scene_blocks_workspace_bytes, lib.conv3p_scene_blocks_f32))
        need = nbytes(N, num_point, max_blocks, block, stride)
    if out is None:
        out = cls(*shape[:4], dev, need, *shape[4:])
    elif need:
        _grow(out, "workspace", need, dev)
    if many:
        out._room_blocks_host = None
        out.room_start = _upload(torch.from_numpy(rs.astype(np.int32)), dev) if rs is not None else room_start
    if N == 0 or max_blocks == 0 or R == 0:  # nothing is launched, so nothing is written
        _fill_empty(out)
        return out
    ws = out.workspace
    with torch.cuda.device(dev):
        _call(call, data.data_ptr(), _ptr(labels), *((out.room_start.data_ptr(), N, R) if many else (N,)), K,
              _LABEL_DTYPES[labels.dtype] if labels is not None else 0, block, stride, num_point, min_points, max_blocks,
              *((int(cover),) if many else ()), int(seed), int(step), out.data.data_ptr(), _ptr(out.labels),
              out.index.data_ptr(), out.block_cell.data_ptr(), out.block_count.data_ptr(),
              *((out.block_room.data_ptr(), out.room_blocks.data_ptr(), out.room_stats.data_ptr()) if many else ()),
              out.stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    return out


def scene_blocks(data, labels=None, num_point=4096, block=1.0, stride=1.0, min_points=100, max_blocks=None, seed=0,
                 step=0, out=None, cover=False):
    """One room -> SceneBlocks, by the ten steps of include/conv3p.h (conv3p_scene_blocks_f32), or with cover=True by
    the covering mode's (conv3p_scene_blocks_cover_f32: a cell of n > num_point members becomes ceil(n / num_point)
    blocks that hold each of its rows once; max_blocks=None is then default_max_blocks(..., num_point)).

    data float32 (N, K >= 3), xyz first, z up; labels (N) uint8 / int32 / int64 or None.  block and stride are taken
    as float32, block in [stride, 2 stride].  max_blocks=None: default_max_blocks(N, block, stride, min_points), a
    bound from the shape alone.  (seed, step) select the draws.  out: a SceneBlocks of an earlier call with the same
    shapes, written into.  Nothing is synchronised on; stats[7] != 0 reports a tiling of more than SCENE_MAX_CELLS
    cells (nothing emitted)."""
    return _blocks(False, data, None, labels, num_point, block, stride, min_points, max_blocks, seed, step, out, cover)


class SceneRoomBlocks(SceneBlocks):
    """The outputs of scene_blocks_rooms: SceneBlocks' fields over the blocks of all rooms, room after room -- index
    holds GLOBAL rows, block_cell the cell within the block's room -- plus block_room int32 (max_blocks) (-1 past the
    emitted blocks), room_blocks int32 (R + 1), the prefix of the emitted blocks per room, room_stats int32 (R, 8), the
    single-room stats of every room, and room_start, the device tensor the call used.  stats int32 (8) = {emitted
    blocks, kept cells, R, total cells, non-finite rows, small cells, blocks needed (covering), error bits: 1 a room of
    too many cells, 2 room_start malformed, 4 too many cells in all, 8 an internal error (more member pairs than the
    workspace bound: the result is not to be used)}."""

    _SLICED = SceneBlocks._SLICED + ("block_room",)
    _SHARED = SceneBlocks._SHARED + ("room_blocks", "room_stats", "room_start", "_room_blocks_host")
    _FILL = SceneBlocks._FILL + (("block_room", -1), ("room_blocks", 0), ("room_stats", 0))

    def __init__(self, max_blocks, num_point, K, with_labels, device, workspace_bytes=0, num_rooms=0):
        SceneBlocks.__init__(self, max_blocks, num_point, K, with_labels, device, workspace_bytes)
        R = int(num_rooms)
        self.shape = self.shape + (R,)
        self.block_room = torch.empty((int(max_blocks),), dtype=torch.int32, device=device)
        self.room_blocks = torch.zeros((R + 1,), dtype=torch.int32, device=device)
        self.room_stats = torch.zeros((R, 8), dtype=torch.int32, device=device)
        self.room_start = None
        self._room_blocks_host = None

    def trim(self):
        """Views of the first num_blocks() blocks, as a SceneRoomBlocks (stats and the per-room tensors shared)."""
        nb = self.num_blocks()
        return _view(self, SceneRoomBlocks, slice(nb), self._SLICED, self._SHARED, shape=(nb,) + self.shape[1:], workspace=None)

    def room(self, r):
        """Views of room r's blocks, as a SceneBlocks whose stats is room_stats[r]; index stays global.  The first call
        reads room_blocks to the host (a synchronisation), later ones reuse it."""
        R = self.shape[4]
        _require(isinstance(r, int) and 0 <= r < R, "room must be an integer in [0, %d)" % R)
        if self._room_blocks_host is None:
            self._room_blocks_host = self.room_blocks.tolist()
        b0, b1 = self._room_blocks_host[r], self._room_blocks_host[r + 1]
        return _view(self, SceneBlocks, slice(b0, b1), SceneBlocks._SLICED, (), shape=(b1 - b0,) + self.shape[1:4],
                     stats=self.room_stats[r], workspace=None)


def default_max_blocks_rooms(room_rows, block=1.0, stride=1.0, min_points=100, num_point=None):
    """default_max_blocks summed over rooms of room_rows[r] rows each: what scene_blocks_rooms uses for max_blocks=None
    when the host knows room_start."""
    return max(1, sum(default_max_blocks(n, block, stride, min_points, num_point) for n in room_rows if n > 0))


def _rooms_bound(N, R, block, stride, min_points, num_point):
    """The bound from N and R alone, for a room_start only the device knows: the sum over the rooms of min(65536, n_r m^2
    // need) is at most min(R 65536, N m^2 // need) -- default_max_blocks(N, ...) with its min(65536, .) applied R times
    over -- and the covering mode's sum of n_r m^2 // P is at most N m^2 // P; each room's max(1, .) adds at most R."""
    m = int(math.ceil(float(block) / float(stride))) + 1
    kept = min(R * _lib.SCENE_MAX_CELLS, N * m * m // max(1, int(min_points)))
    return max(1, R + kept + (N * m * m // int(num_point) if num_point is not None else 0))


def scene_blocks_rooms(data, room_start, labels=None, num_point=4096, block=1.0, stride=1.0, min_points=100,
                       max_blocks=None, seed=0, step=0, out=None, cover=False):
    """Many rooms -> SceneRoomBlocks in one call (conv3p_scene_blocks_rooms_f32): the concatenation of scene_blocks(room
    r's rows, ..., seed=seed + r, cover=cover) over the rooms, cut at max_blocks, index holding global rows.

    data float32 (N, K >= 3), the rooms' rows one room after the other; labels (N) or None.  room_start: the R + 1
    boundaries.  A device int32 tensor is used as is (a malformed one is reported in stats[7], bit 1); a Python
    sequence, numpy array or CPU tensor is checked here (ascending, inside [0, N], rooms of at most 2^24 rows) and copied
    once, through pinned memory on the current stream.  max_blocks=None: default_max_blocks summed per room when the host knows room_start, otherwise a bound from N
    and R alone; neither synchronises.  That second bound is very loose -- R + min(65536 R, N m^2 // min_points) + N m^2
    // num_point blocks, and the outputs are allocated for it: 4 M rows at stride 0.5 ask for tens of GB -- so a caller
    with a device room_start should pass max_blocks (from the rooms' extents, or from a first call with max_blocks=1
    and blocks_needed()).  The other arguments are scene_blocks'.  Nothing is synchronised on."""
    return _blocks(True, data, room_start, labels, num_point, block, stride, min_points, max_blocks, seed, step, out, cover)


class _RowTable:
    """What SceneVotes and SceneScores share: a (num_rows, num_class) table on the device that add() accumulates into,
    the labels and counts computed from it on demand (and kept until the table changes), and their workspace.  A subclass
    names its table, the table's dtype, its class limit with the messages, and the two entry points of labels()."""

    def __init__(self, num_rows, num_class, device="cuda:0"):
        _require_int(num_rows, "num_rows must be an integer in [0, 2^31)", 0, 2 ** 31 - 1, allow_bool=True)
        _require_int(num_class, self._CLASS_MESSAGE, 1, self._MAX_CLASS, allow_bool=True)
        self.device = torch.device(device)
        _require(self.device.type == "cuda", self._DEVICE_MESSAGE)
        self.num_rows, self.num_class = num_rows, num_class
        setattr(self, self._TABLE, torch.zeros((num_rows, num_class), dtype=self._DTYPE, device=self.device))
        self._labels = torch.empty((num_rows,), dtype=torch.int32, device=self.device)
        self._counts = torch.zeros((2,), dtype=torch.int64, device=self.device)
        nbytes = getattr(_lib.load(), self._LABELS_ENTRY + "_workspace_bytes")(num_rows, num_class)
        self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if nbytes else None
        self._fresh = False

    def reset(self):
        getattr(self, self._TABLE).zero_()
        self._fresh = False

    def labels(self):
        if self.num_rows and not self._fresh:
            ws = self._workspace
            with torch.cuda.device(self.device):
                _call(getattr(_lib.load(), self._LABELS_ENTRY), getattr(self, self._TABLE).data_ptr(), self.num_rows,
                      self.num_class, self._labels.data_ptr(), self._counts.data_ptr(), ws.data_ptr(), ws.numel(),
                      _stream(self.device))
            self._fresh = True
        return self._labels

    def counts(self):
        self.labels()
        return self._counts


class SceneVotes(_RowTable):
    """Votes of block predictions for the rows of one room: votes int32 (num_rows, num_class) on the device.

    add(pred, index): every element with 0 <= index < num_rows and 0 <= pred < num_class adds one vote -- each emitted
    row votes, so a room row drawn twice votes twice; index -1 (filler blocks) and out-of-range predictions are
    ignored.  Votes accumulate over calls (other steps, overlapping strides) until reset().  labels() -> (num_rows)
    int32, the class with the most votes, the lowest on a tie, -1 without votes; counts() -> int64 device tensor
    {voted rows, unvoted rows} of the last labels() (computed if there was none)."""

    _TABLE, _DTYPE, _MAX_CLASS, _LABELS_ENTRY = "votes", torch.int32, float("inf"), "conv3p_scene_vote_labels"
    _CLASS_MESSAGE = "num_class must be a positive integer"
    _DEVICE_MESSAGE = "votes live on a HIP device (there is no CPU path)"

    def add(self, pred, index):
        for name, t in (("pred", pred), ("index", index)):
            _require_tensor(t, "%s must be a contiguous int32 tensor on the votes' device" % name, torch.int32, dev=self.device)
        _require(pred.numel() == index.numel(), "pred and index must have as many elements")
        self._fresh = False
        if pred.numel() == 0 or self.num_rows == 0:
            return
        with torch.cuda.device(self.device):
            _call(_lib.load().conv3p_scene_vote, pred.data_ptr(), index.data_ptr(), pred.numel(), self.num_rows,
                  self.num_class, self.votes.data_ptr(), _stream(self.device))


class SceneScores(_RowTable):
    """Summed class probabilities of block predictions for the rows of one room: scores int64 (num_rows, num_class) on
    the device, in fixed point -- a vote adds llrintf(softmax(logits)[c] * SCALE) to its room row's class c, so the
    sums are exact and do not depend on the order of the rows or of the calls.

    add(logits, index): logits float32 (..., num_class), the model's last activations; index int32 with as many rows.
    A row with 0 <= index < num_rows and finite logits votes; vote_stats int64 (2) accumulates {rows that voted, rows
    with a valid index refused for a non-finite logit}.  Scores accumulate over calls until reset().  labels() ->
    (num_rows) int32, the class with the largest score, the lowest on a tie, -1 where no row voted; counts() -> int64
    device tensor {voted rows, unvoted rows} of the last labels() (computed if there was none).  scores / SCALE is the
    sum of the probabilities."""

    SCALE = 1 << 30
    _TABLE, _DTYPE, _MAX_CLASS, _LABELS_ENTRY = "scores", torch.int64, 128, "conv3p_scene_score_labels"
    _CLASS_MESSAGE = "num_class must be an integer in [1, 128]"
    _DEVICE_MESSAGE = "scores live on a HIP device (there is no CPU path)"

    def __init__(self, num_rows, num_class, device="cuda:0"):
        _RowTable.__init__(self, num_rows, num_class, device)
        self.vote_stats = torch.zeros((2,), dtype=torch.int64, device=self.device)

    def reset(self):
        _RowTable.reset(self)
        self.vote_stats.zero_()

    def add(self, logits, index):
        _require(_is_tensor(logits, torch.float32, dev=self.device, min_dim=1) and logits.shape[-1] == self.num_class,
                 "logits must be a contiguous float32 (..., num_class) tensor on the scores' device")
        _require_tensor(index, "index must be a contiguous int32 tensor on the scores' device", torch.int32, dev=self.device)
        _require(logits.numel() == index.numel() * self.num_class, "logits and index must have as many rows")
        self._fresh = False
        if index.numel() == 0 or self.num_rows == 0:
            return
        with torch.cuda.device(self.device):
            _call(_lib.load().conv3p_scene_vote_scores_f32, logits.data_ptr(), index.data_ptr(), index.numel(),
                  self.num_rows, self.num_class, self.scores.data_ptr(), self.vote_stats.data_ptr(), _stream(self.device))
