"""CPU tests (not gpu) of the batch provider: the C ABI exports and binds its two symbols under the unchanged ABI
version and profile-kind list, the status codes decided before any HIP call, the Python argument checks, and the numpy
restatement of the draw recipe (tests/provider_ref.py): ranges, moments, distinct counters."""
import ctypes

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, provider
from pointwise_amd.conv3p_op import Conv3pInvalidArgument

from tests import provider_ref as ref


def test_symbols_are_bound_and_abi_and_profile_kinds_are_unchanged():
    lib = _lib.load()
    for n in ("conv3p_provider_workspace_bytes", "conv3p_provider_batch_f32"):
        assert n in _lib.SYMBOLS and getattr(lib, n).argtypes is not None
    names = [lib.conv3p_profile_name(k).decode() for k in range(lib.conv3p_profile_kinds())]
    assert len(names) == 20 and names[-1] == "seg_head_kernel"
    assert lib.conv3p_abi_version() == 5 and _lib.ABI_VERSION == 5
    import pointwise_amd
    assert pointwise_amd.assemble_batch is provider.assemble_batch and pointwise_amd.BatchProvider is provider.BatchProvider
    for n in ("next_epoch", "has_next_batch", "next_batch", "get_batch_point_cloud", "state_dict", "load_state_dict"):
        assert callable(getattr(provider.BatchProvider, n))


def test_workspace_bytes():
    f = _lib.load().conv3p_provider_workspace_bytes
    assert f(32, 2048, 0) == 0 and f(32, 2048, 3) == 0                   # only the sort stages rows
    assert f(32, 2048, 4) >= 32 * 2048 * 12 and f(32, 2048, 4) % 256 == 0
    assert f(1, 8192, 7) >= 8192 * 12
    assert f(1, 8193, 4) == 0 and f(0, 5, 4) == 0 and f(5, 0, 4) == 0


def _call(**kw):
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    a = dict(data=p, labels=p, S=10, Nsrc=64, K=3, lb=1, pp=0, perm=None, plen=0, start=0, B=4, N=64, flags=7, sigma=0.01,
             clip=0.05, seed=1, step=2, cs=None, noise=None, points=p, input=p, lout=p, cso=None, no=None, oo=None, bad=p,
             ws=p, wsb=1 << 20)
    a.update(kw)
    return lib.conv3p_provider_batch_f32(*[a[k] for k in (
        "data", "labels", "S", "Nsrc", "K", "lb", "pp", "perm", "plen", "start", "B", "N", "flags", "sigma", "clip", "seed",
        "step", "cs", "noise", "points", "input", "lout", "cso", "no", "oo", "bad", "ws", "wsb")], None)


def test_status_codes_before_any_launch():
    """Everything here is decided before a HIP call: bogus (never dereferenced) pointers are fine."""
    INV, UNS, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    for name in ("data", "points", "input", "bad"):
        assert _call(**{name: None}) == INV
    assert _call(labels=None) == INV and _call(lout=None) == INV          # one without the other
    for kw in (dict(B=-1), dict(N=-1), dict(K=2), dict(N=65), dict(start=-1), dict(flags=8), dict(lb=2), dict(clip=0.0),
               dict(clip=float("nan")), dict(sigma=-1.0), dict(perm=ctypes.c_void_p(4096), plen=3),
               dict(perm=ctypes.c_void_p(4096), plen=8, start=5)):
        assert _call(**kw) == INV, kw
    assert _call(clip=0.0, flags=5, wsb=0, ws=None) == WS                 # the clip is not looked at without JITTER
    assert _call(B=0, data=None) == _lib.OK and _call(N=0, data=None) == _lib.OK
    assert _call(Nsrc=9000, N=9000) == UNS and _call(Nsrc=9000, N=9000, wsb=0) == UNS   # before WORKSPACE
    assert _call(wsb=8) == WS and _call(ws=None) == WS and _call(ws=ctypes.c_void_p(4097)) == WS


def test_python_argument_checks():
    """Tensors on the CPU: every check but the device's comes first, so each message is reachable without a GPU."""
    data, lab = torch.zeros(5, 16, 3), torch.zeros(5, dtype=torch.int64)
    cases = [("float32", (data.double(), lab, 2), {}), ("float32", (torch.zeros(5, 16, 2), lab, 2), {}),
             ("float32", (torch.zeros(5, 16), lab, 2), {}), ("uint8, int32 or int64", (data, lab.float(), 2), {}),
             ("labels must be", (data, torch.zeros(4, dtype=torch.int64), 2), {}),
             ("labels must be", (data, torch.zeros(5, 15, dtype=torch.uint8), 2), {}),
             ("num_points", (data, lab, 2), dict(num_points=17)), ("batch_size", (data, lab, -1), {}),
             ("start", (data, lab, 2), dict(start=-1)),
             ("perm must be", (data, lab, 2), dict(perm=torch.zeros(5, dtype=torch.int64))),
             ("past perm", (data, lab, 3), dict(perm=torch.zeros(5, dtype=torch.int32), start=3)),
             ("clip", (data, lab, 2), dict(jitter=True, clip=0.0)), ("clip", (data, lab, 2), dict(jitter=True, clip=-1.0)),
             ("sigma", (data, lab, 2), dict(jitter=True, sigma=-0.1)),
             ("cos_sin given without", (data, lab, 2), dict(cos_sin=torch.zeros(2, 2, dtype=torch.float64))),
             ("cos_sin must be", (data, lab, 2), dict(rotate=True, cos_sin=torch.zeros(3, 2, dtype=torch.float64))),
             ("cos_sin must be", (data, lab, 2), dict(rotate=True, cos_sin=torch.zeros(2, 2))),
             ("noise must be", (data, lab, 2), dict(jitter=True, noise=torch.zeros(2, 16, 2, dtype=torch.float64))),
             ("seed and step", (data, lab, 2), dict(seed=-1)), ("seed and step", (data, lab, 2), dict(step=2 ** 64)),
             ("HIP device", (data, lab, 2), {})]
    for msg, a, kw in cases:
        with pytest.raises(Conv3pInvalidArgument, match=msg):
            provider.assemble_batch(*a, **kw)
    with pytest.raises(Conv3pInvalidArgument):
        provider.BatchProvider(np.zeros((4, 8, 3), np.float32), np.zeros(4, np.uint8), 0, device="cpu")
    with pytest.raises(Conv3pInvalidArgument):
        provider.BatchProvider(np.zeros((4, 8, 3), np.float32), np.zeros(4, np.uint8), 2, num_points=9, device="cpu")


def test_uniforms_stay_inside_their_intervals():
    top = np.uint32(0xFFFFFFFF)
    assert ref.uniform53(0, 0) == 0.0 and 0.0 < ref.uniform53(top, top) < 1.0
    assert ref.uniform53(top, top) == 1.0 - 2.0 ** -53
    u1, u2, u3, u4 = ref.box_muller_uniforms(np.array([[0, 0, 0, 0], [top, top, top, top]], dtype=np.uint32))
    assert u1[0] == 2.0 ** -32 and u3[0] == 2.0 ** -32 and u1[1] == 1.0 and u3[1] == 1.0      # no log(0)
    assert u2[0] == 0.0 and u4[0] == 0.0 and u2[1] < 1.0 and u4[1] < 1.0
    n = ref.normals_from_words(np.array([[0, 0, 0, 0], [top, top, top, top]], dtype=np.uint32))
    assert np.isfinite(n).all() and np.abs(n).max() <= np.sqrt(2 * 32 * np.log(2))
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2 ** 32, size=(1000, 2), dtype=np.uint64).astype(np.uint32)
    u = ref.uniform53(w[:, 0], w[:, 1])
    assert (u >= 0).all() and (u < 1).all()


def test_restated_normals_have_the_moments_of_a_standard_normal():
    """10^6 normals of seed 2024, step 3: 84 samples x 3969 rows x 3 (deterministic: a fixed function of the seed)."""
    z = ref.draw_noise(2024, 3, np.arange(84), 3969).reshape(-1)
    n = z.size
    assert n >= 10 ** 6
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert np.abs(z).max() <= np.sqrt(2 * 32 * np.log(2))
    a = ref.draw_angles(2024, 3, np.arange(1000))
    assert (a >= 0).all() and (a < 2 * np.pi).all() and abs(a.mean() - np.pi) < 5 * (2 * np.pi / np.sqrt(12)) / np.sqrt(1000)


def test_counters_of_angle_jitter_and_dropout_are_pairwise_distinct():
    S, N, seed, step = 5, 7, 9, 11
    seen = set()
    total = 0
    for c in ref.angle_counters(seed, step, np.arange(S)):
        seen.add(tuple(int(v) for v in c))
        total += 1
    for s in range(S):
        for c in ref.jitter_counters(seed, step, s, N):
            seen.add(tuple(int(v) for v in c))
            total += 1
    M, H = 32, 512                                             # the tail's mask: (e >> 2, 0, step low, step high)
    for blk in range(M * H // 4):
        seen.add((blk, 0, step & 0xFFFFFFFF, step >> 32))
        total += 1
    assert len(seen) == total
    assert all(c[1] == 0xFFFFFFFF for c in map(tuple, ref.angle_counters(seed, step, np.arange(S))))
    assert all(1 <= c[1] <= S for s in range(S) for c in map(tuple, ref.jitter_counters(seed, step, s, N)))
