"""CPU tests (not gpu) of the Morton order: the numpy statement of the definition (tests/morton_ref.py) against the naive
one, the figures the order was chosen by, the new symbol and flag of the C ABI with the status codes decided before any
HIP call, and the Python check of sort_method."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import prestep_numpy
from pointwise_amd import _lib, prestep, provider, synth
from tests import morton_ref as ref


def _random_with_duplicate():
    p = np.random.default_rng(11).uniform(-2, 3, size=(200, 3)).astype(np.float32)
    p[150] = p[17]
    return p


def _planar():
    p = np.random.default_rng(12).uniform(0, 1, size=(97, 3)).astype(np.float32)
    p[:, 1] = np.float32(0.25)
    return p


CORNERS = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
CLOUDS = {
    "duplicate": _random_with_duplicate,
    "nonfinite": ref.nonfinite_cloud,
    "planar": _planar,
    "all_equal": lambda: np.full((33, 3), 0.7, dtype=np.float32),
    "single": lambda: np.array([[1.5, -2.0, 3.0]], dtype=np.float32),
    "corners": lambda: np.array(CORNERS, dtype=np.float32)[[5, 0, 7, 2, 1, 6, 3, 4]],
}


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_the_numpy_statement_equals_the_naive_one(name):
    cloud = CLOUDS[name]()
    assert ref.codes(cloud).tolist() == ref.naive_codes(cloud)
    order = ref.order(cloud)
    assert order.dtype == np.int32 and order.tolist() == ref.naive_order(cloud)
    assert sorted(order.tolist()) == list(range(cloud.shape[0]))
    if name == "duplicate":
        assert ref.codes(cloud)[150] == ref.codes(cloud)[17]
        assert order.tolist().index(17) + 1 == order.tolist().index(150)         # the tie goes by the original index
    if name == "nonfinite":
        assert order[-3:].tolist() == [3, 10, 20] and (ref.codes(cloud)[[3, 10, 20]] == ref.FAR).all()
    if name == "planar":
        assert not (ref.codes(cloud) & np.uint64(0x492492492492)).any()          # no y bit (3k + 1) is ever set
    if name in ("all_equal", "single"):
        assert order.tolist() == list(range(cloud.shape[0])) and not ref.codes(cloud).any()
    if name == "corners":
        assert [tuple(int(c) for c in r) for r in cloud[order]] == CORNERS


def test_the_figures_the_order_was_chosen_by():
    """Sixteen bits an axis separate every point of the models' clouds; the lattice clouds exercise the tie rule and the
    far corner's code; and no cloud's Morton order could be mistaken for its xyz order."""
    def tied(cloud):
        return cloud.shape[0] - np.unique(ref.codes(cloud)).size         # rows whose code an earlier row has already
    for batch in (synth.modelnet_like(2, 2048, 1), synth.room_like(2, 4096, 2), synth.room_like(1, 8192, 3),
                  synth.uniform_cube(2, 300, 4)):
        for cloud in batch:
            assert tied(cloud) == 0
    lat = synth.lattice(2, 2048, seed=4)
    assert [tied(c) for c in lat] == [128, 134]
    assert (ref.codes(lat[0]) == ref.FAR).any() and not (ref.codes(lat[1]) == ref.FAR).any()
    for batch in (synth.modelnet_like(2, 2048, 1), synth.room_like(2, 4096, 2), synth.uniform_cube(2, 300, 4), lat):
        xyz = np.stack([np.lexsort((c[:, 2], c[:, 1], c[:, 0])) for c in batch])
        assert np.array_equal(prestep_numpy.sort_point_cloud_xyz(batch), ref.gather(batch, xyz))
        assert (ref.batch_order(batch) != xyz).mean() > 0.98


def test_symbol_and_flag_are_exported_and_declared():
    lib = _lib.load()
    assert "conv3p_sort_morton_order_f32" in _lib.SYMBOLS
    assert _lib.SYMBOLS["conv3p_sort_morton_order_f32"] == _lib.SYMBOLS["conv3p_sort_xyz_order_f32"]
    assert lib.conv3p_sort_morton_order_f32.argtypes is not None
    assert _lib.PROVIDER_MORTON == 8 and lib.conv3p_abi_version() == 5
    for n in ("sort_order_morton", "sort_point_cloud_morton", "sort_point_cloud_morton2"):
        assert callable(getattr(prestep, n))


def test_sort_order_status_codes_before_any_launch():
    f = _lib.load().conv3p_sort_morton_order_f32
    p = ctypes.c_void_p(4096)
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    assert f(p, -1, 4, 3, p, None) == INV and f(p, 1, -1, 3, p, None) == INV and f(p, 1, 4, 2, p, None) == INV
    assert f(None, 1, 4, 3, p, None) == INV and f(p, 1, 4, 3, None, None) == INV
    assert f(None, 0, 4, 3, None, None) == _lib.OK and f(None, 3, 0, 3, None, None) == _lib.OK
    assert f(p, 1, 8193, 3, p, None) == UNS


def _call(**kw):
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    a = dict(data=p, labels=p, S=10, Nsrc=64, K=3, lb=1, pp=0, perm=None, plen=0, start=0, B=4, N=64, flags=12, sigma=0.01,
             clip=0.05, seed=1, step=2, cs=None, noise=None, points=p, input=p, lout=p, cso=None, no=None, oo=None, bad=p,
             ws=p, wsb=1 << 20)
    a.update(kw)
    return lib.conv3p_provider_batch_f32(*[a[k] for k in (
        "data", "labels", "S", "Nsrc", "K", "lb", "pp", "perm", "plen", "start", "B", "N", "flags", "sigma", "clip", "seed",
        "step", "cs", "noise", "points", "input", "lout", "cso", "no", "oo", "bad", "ws", "wsb")], None)


def test_provider_status_codes_before_any_launch():
    """Bogus (never dereferenced) pointers, as tests/test_provider_host.py: everything here is decided before a HIP
    call.  With a sufficient workspace flags = 12 gets exactly as far as flags = 4: past every check, to the point where
    B * N == 0 returns OK and a missing output is looked at."""
    INV, UNS, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    assert _call(flags=8) == INV and _call(flags=8 | 1) == INV and _call(flags=8 | 3) == INV    # MORTON qualifies SORT
    assert _call(flags=16) == INV and _call(flags=12 | 16) == INV
    f = _lib.load().conv3p_provider_workspace_bytes
    assert f(4, 64, 12) == f(4, 64, 4) > 0 and f(4, 64, 8) == 0 and f(1, 8193, 12) == 0
    for flags in (4, 12, 15):
        assert _call(flags=flags, wsb=f(4, 64, flags) - 1) == WS and _call(flags=flags, ws=None) == WS
        assert _call(flags=flags, wsb=f(4, 64, flags), B=0, data=None) == _lib.OK
        assert _call(flags=flags, wsb=f(4, 64, flags), points=None) == INV
        assert _call(flags=flags, Nsrc=9000, N=9000) == UNS and _call(flags=flags, Nsrc=9000, N=9000, wsb=0) == UNS


def test_an_unknown_sort_method_is_a_value_error_on_the_cpu():
    data, lab = torch.zeros(5, 16, 3), torch.zeros(5, dtype=torch.int64)
    for kw in (dict(sort_method="hilbert"), dict(sort_method="hilbert", sort_cloud=True), dict(sort_method=None)):
        with pytest.raises(ValueError, match="sort_method"):
            provider.assemble_batch(data, lab, 2, **kw)
    with pytest.raises(ValueError, match="sort_method"):
        provider.BatchProvider(np.zeros((4, 8, 3), np.float32), np.zeros(4, np.uint8), 2, sort_method="hilbert", device="cpu")
    for method in provider.SORT_METHODS:                     # a known method goes on to the device check, as before
        with pytest.raises(provider.Conv3pInvalidArgument, match="HIP device"):
            provider.assemble_batch(data, lab, 2, sort_cloud=True, sort_method=method)
