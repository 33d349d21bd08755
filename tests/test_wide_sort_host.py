"""CPU tests (not gpu) of the wide sort (include/conv3p.h: conv3p_sort_order_f32, conv3p_provider_batch_wide_f32 and their
_bytes functions): the symbols and constants, the status codes and their order -- all decided before any HIP call, so
bogus (never dereferenced) pointers are fine -- the workspace sizes, and the Python checks that come before device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, prestep, provider

INV, UNS, WS, OK = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.OK
P = ctypes.c_void_p(4096)


def test_symbols_constants_and_abi_version():
    lib = _lib.load()
    for n in ("conv3p_sort_order_workspace_bytes", "conv3p_sort_order_f32", "conv3p_provider_wide_workspace_bytes",
              "conv3p_provider_batch_wide_f32"):
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    assert _lib.SYMBOLS["conv3p_provider_batch_wide_f32"] == _lib.SYMBOLS["conv3p_provider_batch_f32"]
    assert (_lib.SORT_XYZ, _lib.SORT_MORTON) == (0, 1) and _lib.WIDE_SORT_MAX_POINTS == 65536
    assert lib.conv3p_abi_version() == 5 and _lib.ABI_VERSION == 5
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"             # the launches are outside the bracket
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conv3p.h")).read()
    assert "#define CONV3P_SORT_XYZ 0" in header and "#define CONV3P_SORT_MORTON 1" in header
    for n in ("sort_order", "sort_point_cloud", "sort_point_cloud2"):
        assert callable(getattr(prestep, n))


def test_sort_order_workspace_bytes():
    f = _lib.load().conv3p_sort_order_workspace_bytes
    for method in (0, 1):
        key = (16, 8)[method]
        assert f(0, 5, method) == 0 and f(-1, 5, method) == 0 and f(5, 0, method) == 0 and f(5, -1, method) == 0
        assert f(1, 65537, method) == 0 and f(1, 65536, method) >= 65536 * key
        for N in (1, 64, 300, 8192, 8193, 20000, 65536):
            sizes = [f(B, N, method) for B in (1, 2, 3, 16)]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
            assert sizes[0] >= N * key                                       # the cloud's keys live there
    assert f(1, 64, 2) == 0 and f(1, 64, -1) == 0                           # an unknown method


def test_provider_wide_workspace_bytes():
    f = _lib.load().conv3p_provider_wide_workspace_bytes
    old = _lib.load().conv3p_provider_workspace_bytes
    assert f(4, 64, 0) == 0 and f(4, 64, 3) == 0 and f(4, 64, 8) == 0       # flags without _SORT
    assert f(0, 64, 4) == 0 and f(4, 0, 4) == 0 and f(-1, 64, 4) == 0 and f(1, 65537, 4) == 0
    for flags in (4, 12, 15):
        for N in (64, 8192, 8193, 65536):
            sizes = [f(B, N, flags) for B in (1, 2, 5)]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
            assert sizes[0] >= N * (12 + 4 + (8 if flags & 8 else 16))       # stage, order, keys
    assert old(1, 8193, 4) == 0 and old(1, 8193, 12) == 0                   # the one-launch call's is what it was


def test_sort_order_status_codes_and_their_order():
    lib = _lib.load()
    f, nbytes = lib.conv3p_sort_order_f32, lib.conv3p_sort_order_workspace_bytes
    big = 1 << 30
    for method in (0, 1):
        assert f(P, -1, 4, 3, method, P, P, big, None) == INV and f(P, 1, -1, 3, method, P, P, big, None) == INV
        assert f(P, 1, 4, 2, method, P, P, big, None) == INV
        assert f(None, 1, 4, 3, method, P, P, big, None) == INV and f(P, 1, 4, 3, method, None, P, big, None) == INV
        assert f(None, 0, 4, 3, method, None, None, 0, None) == OK and f(None, 3, 0, 3, method, None, None, 0, None) == OK
        assert f(P, 1, 65537, 3, method, P, P, big, None) == UNS
        for N in (4, 9000, 65536):
            need = nbytes(2, N, method)
            assert f(P, 2, N, 3, method, P, P, need - 1, None) == WS and f(P, 2, N, 3, method, P, None, need, None) == WS
        # INVALID before UNSUPPORTED before WORKSPACE
        assert f(None, 1, 65537, 3, method, P, None, 0, None) == INV and f(P, 1, 65537, 2, method, P, None, 0, None) == INV
        assert f(P, 1, 65537, 3, method, P, None, 0, None) == UNS
    for method in (2, -1, 7):
        assert f(P, 1, 4, 3, method, P, P, big, None) == INV
        assert f(P, 0, 4, 3, method, P, P, big, None) == INV                # ... also before B * N == 0
        assert f(P, 1, 65537, 3, method, P, P, big, None) == INV


def _call(fn="conv3p_provider_batch_wide_f32", **kw):
    a = dict(data=P, labels=P, S=10, Nsrc=64, K=3, lb=1, pp=0, perm=None, plen=0, start=0, B=4, N=64, flags=7, sigma=0.01,
             clip=0.05, seed=1, step=2, cs=None, noise=None, points=P, input=P, lout=P, cso=None, no=None, oo=None, bad=P,
             ws=P, wsb=1 << 30)
    a.update(kw)
    return getattr(_lib.load(), fn)(*[a[k] for k in (
        "data", "labels", "S", "Nsrc", "K", "lb", "pp", "perm", "plen", "start", "B", "N", "flags", "sigma", "clip", "seed",
        "step", "cs", "noise", "points", "input", "lout", "cso", "no", "oo", "bad", "ws", "wsb")], None)


def test_provider_wide_status_codes_and_their_order():
    f = _lib.load().conv3p_provider_wide_workspace_bytes
    for flags in (0, 1, 2, 3):
        assert _call(flags=flags) == INV and _call(flags=flags, B=0) == INV  # _SORT is required
    assert _call(flags=8) == INV and _call(flags=8 | 3) == INV              # _MORTON qualifies _SORT
    assert _call(flags=16 | 4) == INV and _call(flags=32 | 12) == INV
    for name in ("data", "points", "input", "bad"):
        assert _call(**{name: None}) == INV
    assert _call(labels=None) == INV and _call(lout=None) == INV
    for kw in (dict(B=-1), dict(N=-1), dict(K=2), dict(N=65), dict(start=-1), dict(lb=2), dict(clip=0.0),
               dict(sigma=-1.0), dict(perm=ctypes.c_void_p(4096), plen=3)):
        assert _call(**kw) == INV, kw
    for flags in (4, 12, 15):
        assert _call(flags=flags, B=0, data=None) == OK and _call(flags=flags, N=0, data=None) == OK
        for N in (64, 9000, 65536):
            need = f(4, N, flags)
            assert _call(flags=flags, Nsrc=N, N=N, wsb=need - 1) == WS and _call(flags=flags, Nsrc=N, N=N, ws=None) == WS
        assert _call(flags=flags, Nsrc=65537, N=65537) == UNS and _call(flags=flags, Nsrc=65537, N=65537, wsb=0) == UNS
        assert _call(flags=flags, Nsrc=65537, N=65537, points=None) == INV  # INVALID first
        # what must not move: the one-launch entry point refuses the same clouds above 8192 and any further flag bit
        assert _call("conv3p_provider_batch_f32", flags=flags, Nsrc=9000, N=9000) == UNS
        assert _call("conv3p_provider_batch_f32", flags=flags | 16) == INV


def test_an_unknown_sort_method_is_a_value_error_before_device_work():
    x = torch.zeros(2, 16, 3)                                               # on the CPU: a known method gets to the device check
    for fn, args in ((prestep.sort_order, (x,)), (prestep.sort_point_cloud, (x,)),
                     (prestep.sort_point_cloud2, (x, torch.zeros(2, 16)))):
        for method in ("hilbert", None, 1):
            with pytest.raises(ValueError, match="sort_method"):
                fn(*args, sort_method=method)
        for method in ("xyz", "morton"):
            with pytest.raises(Exception, match="HIP device") as e:
                fn(*args, sort_method=method)
            assert not isinstance(e.value, ValueError)
    data, lab = torch.zeros(5, 16, 3), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="sort_method"):
        provider.assemble_batch(data, lab, 2, sort_cloud=True, sort_method="hilbert", wide_sort=True)
    with pytest.raises(provider.Conv3pInvalidArgument, match="HIP device"):
        provider.assemble_batch(data, lab, 2, sort_cloud=True, wide_sort=True)


def test_wide_sort_is_a_setting_appended_last_and_not_state():
    import inspect
    for fn in (provider.BatchBuffers.__init__, provider.assemble_batch, provider.BatchProvider.__init__):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "wide_sort" and params[-1].default is False
    bp = provider.BatchProvider.__new__(provider.BatchProvider)             # no device here: the state without the buffers
    bp.seed, bp.epoch, bp.cur_batch, bp.wide_sort = 3, 1, 2, True
    assert bp.state_dict() == {"seed": 3, "epoch": 1, "cur_batch": 2}
    with pytest.raises(ValueError, match="sort_method"):
        provider.BatchProvider(np.zeros((4, 8, 3), np.float32), np.zeros(4, np.uint8), 2, sort_method="hilbert",
                               wide_sort=True, device="cpu")
