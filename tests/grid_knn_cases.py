"""The cases of the k-nearest-voxel search's tests (tests/test_grid_knn_host.py on the numpy references,
tests/test_grid_knn.py on the device): the clouds of tests/grid_interp_rings_cases.py as they are, two rooms that overlap in
space, and a cloud with non-finite rows and cut voxels."""
import numpy as np

from tests import grid_interp_rings_cases as cases
from tests import grid_ref as gr

F = np.float32
KS, RINGS = (1, 3, 8, 16), (1, 2, 4, 8)


def build(name):
    """-> dict: data (N, K) float32, voxel, mode, room_start int32 or None, max_voxels or None, valid: a function of
    (voxel_cell, num_voxels, M) -> int32 (M)."""
    c = dict(voxel=cases.VOXEL, mode="mean", room_start=None, max_voxels=None)
    pad = lambda v, M: np.concatenate([v, np.full(M - v.size, -1, np.int32)])
    voted = lambda seed: (lambda cell, nv, M: pad(cases.some_voted(nv, 0.3, seed), M))
    if name == "centres":                                # exact ties: the order by u
        c.update(data=cases.centres(6), voxel=0.25, mode="center", valid=voted(41))
    elif name == "lattice":
        c.update(data=cases.lattice(5, 42), valid=voted(43))
    elif name == "sparse":
        c.update(data=cases.sparse(12, 0.05, 44), valid=voted(45))
    elif name == "slabs":
        c.update(data=cases.slabs(3, 46), valid=lambda cell, nv, M: pad(cases.near_is_unvoted(cell, nv), M))
    elif name == "corner":
        c.update(data=cases.corner(47), valid=lambda cell, nv, M: pad(cases.cells_valid(cell, nv, [[0, 3, 1], [3, 0, 1]]), M))
    elif name == "rooms":                                # two rooms that overlap in space share nothing
        a, b = cases.lattice(4, 48), cases.sparse(6, 0.3, 49)
        c.update(data=np.concatenate([a, b]), room_start=np.array([0, a.shape[0], a.shape[0] + b.shape[0]], np.int32),
                 valid=voted(50))
    elif name == "nonfinite":                            # NaN / inf rows and rows of cut voxels: inverse == -1
        data, _ = gr.cloud(600, 6, 51, extent=(0.8, 0.8, 0.5))
        data[[3, 399], [0, 2]] = [np.nan, np.inf]
        data[77, 1] = -np.inf
        c.update(data=data, max_voxels=150, valid=voted(52))
    else:
        raise KeyError(name)
    return c


NAMES = ("centres", "lattice", "sparse", "slabs", "corner", "rooms", "nonfinite")


def subsample_ref(c):
    """The numpy subsampling of a case -> its dict (voxel_room / voxel_start None for one cloud)."""
    from tests import grid_rooms_ref as grr
    if c["room_start"] is None:
        sub = gr.grid_subsample_ref(c["data"], None, voxel=c["voxel"], mode=c["mode"], max_voxels=c["max_voxels"])
        sub["voxel_room"] = sub["voxel_start"] = None
        return sub
    return grr.grid_subsample_rooms_ref(c["data"], c["room_start"], None, voxel=c["voxel"], mode=c["mode"], max_voxels=c["max_voxels"])


def displaced(voxel_data, voxel, seed, reach=1.5):
    """voxel_data with xyz moved by up to +/- reach voxels, seeded: representatives that have left their cells."""
    out = np.array(voxel_data, F)
    rng = np.random.default_rng(seed)
    out[:, :3] = (out[:, :3] + (rng.random((out.shape[0], 3)) * 2 - 1) * reach * voxel).astype(F)
    return out


def checkerboard(n=8, voxel=0.25):
    """One row at the centre of every cell (2a, 2b, 0), a, b < n, z identical in all rows: a sheet every voxel of which is
    alone in its 27 cells."""
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xyz = np.stack([(2 * a.reshape(-1) + 0.5) * voxel, (2 * b.reshape(-1) + 0.5) * voxel, np.full(n * n, 0.5 * voxel)], axis=1)
    xyz = xyz - xyz.min(axis=0)                          # the lattice starts at the first row
    return xyz.astype(F)
