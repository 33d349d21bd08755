"""The clouds of the ring fallback's tests (tests/test_grid_interp_rings_host.py on the numpy references,
tests/test_grid_interp_rings.py on the device).  Every cloud has a row at the origin, so the lattice starts there and a
row built for cell (i, j, l) lies in it: rows are placed at least a tenth of a cell inside their cell."""
import numpy as np

F = np.float32
VOXEL = 0.1


def rows_in_cells(ijk, per, rng, voxel=VOXEL, K=4):
    """per rows in every cell of ijk (n, 3), cell after cell, K - 3 random channels behind xyz; cell (0, 0, 0) must be
    among them: its first row is moved to the origin."""
    ijk = np.repeat(np.asarray(ijk, np.float64), per, axis=0)
    xyz = (ijk + 0.1 + 0.8 * rng.random(ijk.shape)) * voxel
    first = np.nonzero((ijk == 0).all(axis=1))[0]
    xyz[first[0]] = 0.0
    return np.concatenate([xyz, rng.random((xyz.shape[0], K - 3))], axis=1).astype(F)


def block(nx, ny, nz, at=(0, 0, 0)):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(at)


def slabs(gap, seed, near_rows=3, ny=4, nz=4, near_cells=None):
    """A near slab one cell thick at x = 0 and a far slab two cells thick at x = gap + 1, gap + 2: the near slab's rows
    are at Chebyshev distance gap + 1 of the nearest far cell.  near_cells: only that many cells of the near slab."""
    rng = np.random.default_rng(seed)
    near = block(1, ny, nz)[:near_cells]
    far = block(2, ny, nz, at=(gap + 1, 0, 0))
    data = np.concatenate([rows_in_cells(near, near_rows, rng), rows_in_cells(np.concatenate([[[0, 0, 0]], far]), 2, rng)[2:]])
    return data[rng.permutation(data.shape[0])]


def near_is_unvoted(voxel_cell, num_voxels):
    """valid_labels for slabs: the voxels of the slab at x = 0 have no vote."""
    return np.where(np.asarray(voxel_cell)[:num_voxels, 0] == 0, -1, 5).astype(np.int32)


def lattice(n, seed, per=2):
    """Every cell of an n^3 lattice occupied."""
    rng = np.random.default_rng(seed)
    data = rows_in_cells(block(n, n, n), per, rng, K=6)
    return data[rng.permutation(data.shape[0])]


def some_voted(num_voxels, share, seed):
    rng = np.random.default_rng(seed)
    valid = np.full(num_voxels, -1, np.int32)
    valid[rng.permutation(num_voxels)[:max(1, int(share * num_voxels))]] = 3
    return valid


def centres(n, voxel=0.25):
    """mode center, voxel 0.25: a row on every cell's centre of an n^3 lattice (and one at the origin); every coordinate
    is a multiple of 1/8, so every d2 is exact and symmetric voxels tie exactly."""
    xyz = np.concatenate([[[0.0, 0.0, 0.0]], (block(n, n, n) + 0.5) * voxel])
    assert np.array_equal(xyz * 8, np.round(xyz * 8))
    return np.concatenate([xyz, np.linspace(0, 1, xyz.shape[0])[:, None]], axis=1).astype(F)


def cells_valid(voxel_cell, num_voxels, cells):
    """valid_labels with a vote on exactly the given cells."""
    cell = np.asarray(voxel_cell)[:num_voxels]
    hit = (cell[:, None, :] == np.asarray(cells)[None, :, :]).all(axis=2).any(axis=1)
    assert hit.sum() == len(cells)
    return np.where(hit, 2, -1).astype(np.int32)


def corner(seed):
    """Rows in cell (0, 0, 0), whose ring cells are negative on three sides, and two voted cells at Chebyshev distance 3:
    (0, 3, 1) is where the lower bound of the empty column (0, 2) of ring 2 lands -- the next column, its z inside the
    run -- and (3, 0, 1) where the columns (2, y) land: the next x.  A walk that compared z alone would take both at ring 2."""
    rng = np.random.default_rng(seed)
    return rows_in_cells([[0, 0, 0], [0, 3, 1], [3, 0, 1]], 4, rng)


def sparse(n, fill, seed, per=2):
    """A random share of the cells of an n^3 lattice, cell (0, 0, 0) among them."""
    rng = np.random.default_rng(seed)
    cells = block(n, n, n)
    keep = np.concatenate([[0], 1 + rng.permutation(n ** 3 - 1)[:int(fill * n ** 3)]])
    data = rows_in_cells(cells[np.sort(keep)], per, rng, K=6)
    return data[rng.permutation(data.shape[0])]
