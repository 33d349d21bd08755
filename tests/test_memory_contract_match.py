"""The memory contract of c3p_grid_match_segments (-m gpu): its workspace at exactly c3p_grid_match_scratch_bytes(M, N, T,
max_pairs), between the guards of tests/memory_rig.py's Arena, and dirty.  include/conv3p_match.h is not read by the rig's
region finder, so the C entry is called here as a C caller would call it.
  R0  one byte short is refused with CONV3P_ERR_INVALID_ARGUMENT, the status the header documents; the outputs, pre-filled
      with a sentinel, the workspace and the guards are unchanged;
  R1  after a run both guards are intact;
  R2  runs on a workspace pre-filled with 0x00, with 0xFF and with the leftover of another case's run give bit-identical
      outputs, equal to the Python call's (whose workspace is the object's own).
The shapes: every unit its own pair with P == max_pairs (the table and the four key buffers are full to their last row),
the same one row short (the overflow path), and a planted case with few pairs in a large table."""
import pytest
import torch

from tests import grid_match_cases as mc
from tests import grid_match_ref as mr
from tests import memory_rig as rig
from tests.test_grid_match import on_device

pytestmark = pytest.mark.gpu


def call(lib, g, seg, truth, T, weight, max_pairs, out, ws_ptr, ws_bytes):
    """c3p_grid_match_segments as GridSegments.match calls it, without classes, with the workspace given -> the status."""
    from pointwise_amd._host import _ptr, _stream
    dev = truth.device
    with torch.cuda.device(dev):
        return lib.c3p_grid_match_segments(seg.segment.data_ptr(), seg.stats.data_ptr(), _ptr(g.inverse), g.stats.data_ptr(),
                                           truth.data_ptr(), seg.shape[0], g.inverse.numel(), T, 1 if weight == "rows" else 0,
                                           None, None, 1, 1, 2, max_pairs, *(_ptr(getattr(out, n)) for n in mr.OUTPUTS),
                                           ws_ptr, ws_bytes, _stream(dev))


@pytest.mark.parametrize("name,weight,short", [("all pairs", "rows", 0), ("all pairs", "voxels", 1), ("planted", "rows", 0)])
def test_the_workspace_at_its_declared_size_between_guards_and_dirty(name, weight, short):
    from pointwise_amd import _lib, grid
    lib = _lib.load()
    dev = torch.device("cuda:0")
    c = mc.all_pairs(4097) if name == "all pairs" else mc.planted(4097, 5)
    other = mc.planted(4097, 6, S=4097, T=c["T"], scatter=True)                # another case of the same shapes, for the leftover
    M, N, T = c["segment"].shape[0], c["inverse"].shape[0], c["T"]
    max_pairs = M - short
    g, seg = on_device(c)
    og, oseg = on_device(other)
    truth = torch.from_numpy(mc.truth_of(c, weight)).to(dev)
    otruth = torch.from_numpy(mc.truth_of(other, weight)).to(dev)
    need = lib.c3p_grid_match_scratch_bytes(M, N, T, max_pairs)
    assert need > 0 and need % 256 == 0
    expected = seg.match(truth, T, weight=weight, max_pairs=max_pairs)
    assert expected.overflowed() == bool(short and name == "all pairs")
    torch.cuda.synchronize()
    arena = rig.Arena(need, dev, "c3p_grid_match_segments workspace")

    def fresh():
        out = grid.SegmentMatch(M, T, max_pairs, 1, dev)
        for n in mr.OUTPUTS:
            getattr(out, n).view(torch.uint8).fill_(rig.SENTINEL)
        return out
    # R0: one byte short
    out = fresh()
    arena.fill(0x3c)
    assert call(lib, g, seg, truth, T, weight, max_pairs, out, arena.body.data_ptr(), need - 1) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert arena.intact() is None and bool((arena.body == 0x3c).all())
    for n in mr.OUTPUTS:
        assert bool((getattr(out, n).view(torch.uint8) == rig.SENTINEL).all()), n
    # R1, R2
    for fill in ("0x00", "0xFF", "leftover"):
        if fill == "leftover":                           # what a run on another case left, whatever that is
            assert call(lib, og, oseg, otruth, T, weight, max_pairs, fresh(), arena.body.data_ptr(), need) == _lib.OK
        else:
            arena.fill(rig.FILLS[fill])
        out = fresh()
        assert call(lib, g, seg, truth, T, weight, max_pairs, out, arena.body.data_ptr(), need) == _lib.OK
        torch.cuda.synchronize()
        assert arena.intact() is None, (fill, arena.intact())
        for n in mr.OUTPUTS:
            assert rig._same(getattr(out, n).cpu(), getattr(expected, n).cpu()), (fill, n)
