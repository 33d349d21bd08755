"""The inputs of the segment-matching tests: a case is what c3p_grid_match_segments reads, as numpy arrays -- segment
(M), S, inverse (N), the emitted voxels, truth per row and per voxel, T, and optionally classes.  Small by design: the
shapes are the smallest at which the kernels can still go wrong (runs that cross a wave of 64 and a workgroup of 256, one
hot slot, every unit its own pair, rows of the table longer than a thread walks alone)."""
import numpy as np

I32 = np.int32


def make(segment, S, inverse, truth_rows, T, truth_voxels=None, pred_class=None, truth_class=None, num_class=1, emitted=None):
    segment = np.asarray(segment, I32)
    M = segment.shape[0]
    inverse = np.asarray(inverse, I32)
    if truth_voxels is None:                             # a voxel takes the truth of its lowest row, -1 without one
        truth_voxels = np.full(M, -1, I32)
        for r in range(inverse.shape[0] - 1, -1, -1):
            if 0 <= inverse[r] < M:
                truth_voxels[inverse[r]] = truth_rows[r]
    return dict(segment=segment, S=int(S), inverse=inverse, emitted=M if emitted is None else emitted,
                truth_rows=np.asarray(truth_rows, I32), truth_voxels=np.asarray(truth_voxels, I32), T=int(T),
                pred_class=None if pred_class is None else np.asarray(pred_class, I32),
                truth_class=None if truth_class is None else np.asarray(truth_class, I32), num_class=num_class)


def truth_of(c, weight):
    return c["truth_rows"] if weight == "rows" else c["truth_voxels"]


def rows_per_voxel(M, per):
    return np.repeat(np.arange(M, dtype=I32), per)


def planted(n_units, seed, S=7, T=5, classes=False, shuffle=True, scatter=False):
    """n_units voxels with one row each, segments and instances drawn as overlapping intervals, some void, some outside
    every segment, some rows without a voxel.  scatter: the units in random order, so that nearly every unit ends a run."""
    rng = np.random.default_rng(seed)
    M = n_units
    segment = np.sort(rng.integers(0, S, M)).astype(I32)
    truth = np.sort(rng.integers(0, T, M)).astype(I32)
    if shuffle:
        truth = np.roll(truth, M // 3)
    segment[rng.random(M) < 0.1] = -1
    truth[rng.random(M) < 0.1] = -1
    if scatter:
        order = rng.permutation(M)
        segment, truth = segment[order], truth[order]
    inverse = np.arange(M, dtype=I32)
    inverse[rng.random(M) < 0.05] = -1
    kw = {}
    if classes:
        kw = dict(pred_class=rng.integers(-1, 4, M).astype(I32), truth_class=rng.integers(-1, 4, T).astype(I32), num_class=3)
    return make(segment, S, inverse, truth, T, **kw)


def one_pair(n_units):
    """Every unit in the pair (0, 0): one slot takes every add."""
    return make(np.zeros(n_units, I32), 1, np.arange(n_units, dtype=I32), np.zeros(n_units, I32), 1)


def all_pairs(n):
    """Every unit its own pair: segment v, instance v reversed -- P == n, and no two consecutive units share a pair."""
    return make(np.arange(n, dtype=I32), n, np.arange(n, dtype=I32), np.arange(n, dtype=I32)[::-1].copy(), n)


def long_rows(k=300):
    """Segment 0 overlaps k instances and instance 0 overlaps k segments: rows the whole wave walks.  Voxel v < k is in
    segment 0 with truth v; voxel k + v is in segment v with truth 0.  Sizes grow with v so that the IoUs differ."""
    seg = np.concatenate([np.zeros(k, I32), np.arange(k, dtype=I32)])
    tru = np.concatenate([np.arange(k, dtype=I32), np.zeros(k, I32)])
    per = np.concatenate([1 + np.arange(k) % 5, 1 + np.arange(k) % 7]).astype(np.int64)
    inverse = np.repeat(np.arange(2 * k, dtype=I32), per)
    return make(seg, k, inverse, tru[inverse], k)


def ties():
    """Instance 0 of 8 units split 4 / 4 by segments 0 and 1; segment 2 of 8 units split 4 / 4 by instances 1 and 2: two
    equal best IoUs on either side, the lowest number wins."""
    seg = np.array([0] * 4 + [1] * 4 + [2] * 8, I32)
    tru = np.array([0] * 8 + [1] * 4 + [2] * 4, I32)
    return make(seg, 3, np.arange(16, dtype=I32), tru, 3)


def edge(name, n=200):
    c = planted(n, 11)
    if name == "S1":
        return make(np.where(c["segment"] >= 0, 0, -1), 1, c["inverse"], c["truth_rows"], c["T"])
    if name == "T1":
        return make(c["segment"], c["S"], c["inverse"], np.where(c["truth_rows"] >= 0, 0, -1), 1)
    if name == "truth_void":
        return make(c["segment"], c["S"], c["inverse"], np.full(n, -1, I32), c["T"])
    if name == "no_segments":
        return make(np.full(n, -1, I32), 0, c["inverse"], c["truth_rows"], c["T"])
    if name == "top_ids":                                # ids equal to T - 1 and S - 1, and ids just outside
        tru = c["truth_rows"].copy()
        tru[::7] = c["T"] - 1
        tru[3::11] = c["T"]
        tru[5::13] = -2
        seg = c["segment"].copy()
        seg[::5] = c["S"] - 1
        seg[2::9] = c["S"]                               # past S: in no segment
        return make(seg, c["S"], c["inverse"], tru, c["T"])
    if name == "no_inverse":
        return make(c["segment"], c["S"], np.full(n, -1, I32), c["truth_rows"], c["T"], truth_voxels=c["truth_voxels"])
    raise KeyError(name)


EDGES = ("S1", "T1", "truth_void", "no_segments", "top_ids", "no_inverse")
UNIT_COUNTS = (1, 63, 64, 65, 1025, 20000)


def boxes_scene(boxes=4, rooms=1, labels=3):
    """Separated boxes of 5 x 5 x 5 voxels of 0.1, 8 rows a voxel on a lattice clear of the cell walls, box b at x = 1.5 b;
    the instance id is the box, the label b % labels.  rooms > 1: the same boxes again per room, instance ids going on, with
    room_start.  -> data float32 (N, 3), instance int32 (N), label int32 (N), room_start int32 or None."""
    a = 0.025 + 0.05 * np.arange(10)
    cube = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    data, inst, lab = [], [], []
    for r in range(rooms):
        for b in range(boxes):
            data.append(cube + np.array([1.5 * b, 0.0, 0.0]))
            inst.append(np.full(cube.shape[0], r * boxes + b, I32))
            lab.append(np.full(cube.shape[0], b % labels, I32))
    n = boxes * cube.shape[0]
    start = None if rooms == 1 else (np.arange(rooms + 1) * n).astype(I32)
    return np.concatenate(data).astype(np.float32), np.concatenate(inst), np.concatenate(lab), start


def boxes_lattice(boxes=4):
    """boxes_scene(boxes) as grid_subsample at voxel 0.1 sees it: the occupancy (nx, 5, 5) of its lattice of cells, box b in
    the cells 15 b .. 15 b + 4 along x; the instance of a cell is cell_x // 15."""
    occ = np.zeros((15 * (boxes - 1) + 5, 5, 5), bool)
    for b in range(boxes):
        occ[15 * b:15 * b + 5] = True
    return occ


def redrawn_labels(cells, seed, labels=3, share=0.05):
    """A label per voxel from its cell: its box's (cell_x // 15 % labels), with a share of the voxels redrawn at random."""
    rng = np.random.default_rng(seed)
    lab = (np.asarray(cells)[:, 0] // 15 % labels).astype(I32)
    hit = rng.random(lab.shape[0]) < share
    lab[hit] = rng.integers(0, labels, int(hit.sum())).astype(I32)
    return lab


MODEL_STEP_SEED = 3
