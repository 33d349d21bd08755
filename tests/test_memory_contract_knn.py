"""The memory contract of conv3p_grid_knn_f32 (-m gpu): its scratch at exactly conv3p_grid_knn_scratch_bytes(Q, num_rooms),
between the guards of tests/memory_rig.py's Arena, and dirty.  include/conv3p_knn.h is not read by the rig's region finder,
so the C entry is called here as a C caller would call it.
  R0  one byte short is refused with CONV3P_ERR_INVALID_ARGUMENT, the status the header documents; the outputs, pre-filled
      with a sentinel, the scratch and the guards are unchanged;
  R1  after a run both guards are intact;
  R2  runs on a scratch pre-filled with 0x00, with 0xFF and with the leftover of another cloud's run give bit-identical
      outputs, equal to the Python call's (whose scratch is the object's own).
The shapes: one cloud and many, one ring (no list is read) and eight, voxel queries and raw rows -- a list of Q entries at
the end of the scratch is where a size function and a kernel could disagree."""
import numpy as np
import pytest
import torch

from tests import grid_knn_cases as kc
from tests import memory_rig as rig

pytestmark = pytest.mark.gpu
OUTPUTS = ("index", "d2", "count", "ring", "scanned", "certified", "stats")


def call(lib, g, d, rows, k, rings, voxel, out, scratch_ptr, scratch_bytes):
    """conv3p_grid_knn_f32 on the subsampling g as GridSubsample.knn calls it, with the scratch given -> the status."""
    from pointwise_amd._host import _ptr, _stream
    M, K = g.data.shape
    room, start = getattr(g, "voxel_room", None), getattr(g, "voxel_start", None)
    query, qv = (d, g.inverse) if rows else (g.data, None)
    with torch.cuda.device(d.device):
        return lib.conv3p_grid_knn_f32(_ptr(query), query.shape[0], query.shape[1], _ptr(qv), _ptr(g.data), K, _ptr(g.neighbors()),
                                       _ptr(g.voxel_cell), _ptr(room), _ptr(start), start.numel() - 1 if room is not None else 0,
                                       g.stats.data_ptr(), M, None, voxel, k, rings, 0, *(getattr(out, n).data_ptr() for n in OUTPUTS),
                                       scratch_ptr, scratch_bytes, _stream(d.device))


@pytest.mark.parametrize("name,rows,rings", [("sparse", True, 8), ("sparse", False, 1), ("rooms", True, 4), ("rooms", False, 8),
                                              ("nonfinite", True, 2)])
def test_the_scratch_at_its_declared_size_between_guards_and_dirty(name, rows, rings):
    from pointwise_amd import _lib, grid
    lib = _lib.load()
    dev = torch.device("cuda:0")
    c = kc.build(name)
    d = torch.from_numpy(np.ascontiguousarray(c["data"])).to(dev)
    kw = dict(voxel=c["voxel"], mode=c["mode"], max_voxels=c["max_voxels"])
    many = c["room_start"] is not None
    g = grid.grid_subsample_rooms(d, torch.from_numpy(c["room_start"]).to(dev), None, **kw) if many else grid.grid_subsample(d, None, **kw)
    other = grid.grid_subsample(torch.flip(d, [0]).contiguous(), None, voxel=c["voxel"] * 1.5)      # another cloud, for the leftover
    Q, k = (d.shape[0] if rows else g.data.shape[0]), 8
    need = lib.conv3p_grid_knn_scratch_bytes(Q, g.voxel_start.numel() - 1 if many else 0)
    assert need > 0 and need % 256 == 0
    expected = g.knn(c["voxel"], d if rows else None, k=k, rings=rings)
    torch.cuda.synchronize()
    arena = rig.Arena(need, dev, "conv3p_grid_knn_f32 scratch")
    # R0: one byte short
    out = grid.GridKnn(Q, k, dev)
    for n in OUTPUTS:
        getattr(out, n).view(torch.uint8).fill_(rig.SENTINEL)
    arena.fill(0x3c)
    assert call(lib, g, d, rows, k, rings, c["voxel"], out, arena.body.data_ptr(), need - 1) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert arena.intact() is None and bool((arena.body == 0x3c).all())
    for n in OUTPUTS:
        assert bool((getattr(out, n).view(torch.uint8) == rig.SENTINEL).all()), n
    # R1, R2
    for fill in ("0x00", "0xFF", "leftover"):
        if fill == "leftover":                           # what a run on another cloud left, whatever that is
            junk = grid.GridKnn(Q, k, dev)
            assert other.data.shape[0] == d.shape[0] and (rows or g.data.shape[0] == d.shape[0])       # the same Q: the same list
            assert call(lib, other, torch.flip(d, [0]).contiguous(), rows, k, 8, c["voxel"] * 1.5, junk, arena.body.data_ptr(),
                        need) == _lib.OK
        else:
            arena.fill(rig.FILLS[fill])
        out = grid.GridKnn(Q, k, dev)
        for n in OUTPUTS:
            getattr(out, n).view(torch.uint8).fill_(rig.SENTINEL)
        assert call(lib, g, d, rows, k, rings, c["voxel"], out, arena.body.data_ptr(), need) == _lib.OK
        torch.cuda.synchronize()
        assert arena.intact() is None, (fill, arena.intact())
        for n in OUTPUTS:
            assert rig._same(getattr(out, n).cpu(), getattr(expected, n).cpu()), (fill, n)
