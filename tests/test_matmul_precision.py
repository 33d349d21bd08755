"""Opt-in bf16 precision of the matrix-core path's filter contractions (CONV3P_CACHE_MATMUL_BF16 of include/conv3p.h;
NeighborCache(matmul_precision="medium")).  The first tests need no GPU (header / constants, the code object, the
attribute); the rest run on the GPU against the float64 sums over the oracle's pair lists
(parity_util.exact_from_oracle_lists) and against the "highest" results of the same cache."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pointwise_amd import _lib, conv3p_op as op, synth
from tests.parity_util import exact_from_oracle_lists, make_case, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOX = 0.1
# ceiling of parity_util.rel_err (max abs error over max(1, max |ref|)) against the exact sums
CEIL = 2e-2


# ------------------------------------------------------------------ no GPU
def test_header_bits_equal_the_python_constants_and_are_disjoint_from_the_other_flags():
    with open(os.path.join(ROOT, "include", "conv3p.h")) as f:
        defs = dict(re.findall(r"#define (CONV3P_CACHE_\w+) (\d+)\b", f.read()))
    assert int(defs["CONV3P_CACHE_MATMUL_BF16"]) == _lib.CACHE_MATMUL_BF16 == 64
    others = 0
    for name, v in defs.items():
        if "MATMUL" not in name:
            others |= int(v)
    assert others & _lib.CACHE_MATMUL_BF16 == 0


def test_code_object_holds_the_bf16_kernels_without_spills():
    """The bf16 instantiations of deep_gemm (forward and grad_input) and deep_dw for the cfg5 class (128, 256) and the
    (256, 256) class are in the code object, every one with no spilled register and no private segment."""
    from pointwise_amd import build
    res = build.kernel_resources()
    # deep_gemm_kernel<KDIM, NDIM, BWD, WIDE, PREC> / deep_dw_kernel<CIN, COUT, PREC>, PREC 1 = bf16
    for must in ["deep_gemm_kernelILi%dELi%dELb%dELb1ELi1EE" % (k, n, bwd)
                 for k, n, bwd in ((128, 256, 0), (256, 128, 1), (256, 256, 0), (256, 256, 1))] + \
                ["deep_dw_kernelILi%dELi%dELi1EE" % (ci, co) for ci, co in ((128, 256), (256, 256))]:
        hit = [r for r in res if must in r[0]]
        assert hit, must + ": kernel not found in the code object"
        for name, _, vspill, sspill, private in hit:
            assert (vspill, sspill, private) == (0, 0, 0), (name, vspill, sspill, private)


def test_matmul_precision_attribute_rejects_unknown_modes():
    cache = op.NeighborCache.__new__(op.NeighborCache)     # (the attribute alone: no device buffer)
    for mode in ("highest", "medium"):
        cache.matmul_precision = mode
        assert cache.matmul_precision == mode
    for bad in ("high", "low", "MEDIUM", "", None, 1):
        with pytest.raises(op.Conv3pInvalidArgument):
            cache.matmul_precision = bad


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, cache, mode, P, X, W, dY, s):
    cache.matmul_precision = mode
    tp, tx, tw, tdy = _t(dev, P), _t(dev, X), _t(dev, W), _t(dev, dY)
    y = op.conv3p(tp, tx, tw, s, VOX, cache=cache)
    dx, dw = op.conv3p_grad(tdy, tp, tx, tw, s, VOX, cache=cache)
    torch.cuda.synchronize()
    return y, dx, dw


def _exact(P, X, W, dY, s):
    parts = [exact_from_oracle_lists(P[b], X[b], W, dY[b], s, VOX) for b in range(P.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), sum(p[2] for p in parts)


def _errs(got, ref):
    return [rel_err(g.cpu().numpy(), r) for g, r in zip(got, ref)]


def _profile(lib, fn):
    lib.conv3p_profile_reset()
    lib.conv3p_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.conv3p_profile_enable(0)
    seen = {}
    for k in range(lib.conv3p_profile_kinds()):
        n = ctypes.c_uint64(0)
        lib.conv3p_profile_read(k, ctypes.byref(n), None)
        seen[lib.conv3p_profile_name(k).decode()] = n.value
    lib.conv3p_profile_reset()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("s", [(1, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("ci,co", [(128, 256), (64, 128), (3, 64), (37, 2), (7, 43), (256, 128)])
def test_medium_against_the_exact_sums(dev, ci, co, s):
    """Room-like data, several tiles per cloud, both ops: medium <= 2e-2 on y, dX and dW, and different from "highest"
    on y (the bf16 kernels ran).  Observed on the first run (MI355X), y / dX / dW: 128->256 2.4e-3 / 1.9e-3 / 1.7e-3
    (stride 2: 2.1e-3 / 2.3e-3 / 1.7e-3), 64->128 2.3e-3 / 2.8e-3 / 2.2e-3, 3->64 2.8e-3 / 1.9e-3 / 1.8e-3, 37->2
    2.8e-3 / 1.1e-3 / 2.1e-3 (stride 2: dW 3.2e-3), 7->43 2.0e-3 / 2.3e-3 / 2.0e-3, 256->128 2.1e-3 / 2.3e-3 / 1.9e-3;
    "highest": at most 2.3e-6."""
    B, N = 2, 700
    P = synth.room_like(B, N, 950, extent=(1.0, 1.0, 1.5))
    X = synth.features(B, N, ci, 951, points=P)
    W = synth.filter_weights(3, 3, 3, ci, co, 952)
    dY = synth.upstream_grad(B, N, co, 953)
    ref = _exact(P, X, W, dY, s)
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    highest = _run(dev, cache, "highest", P, X, W, dY, s)
    got = _run(dev, cache, "medium", P, X, W, dY, s)
    assert not torch.equal(got[0], highest[0])
    for name, e in zip(("y", "dX", "dW"), _errs(got, ref)):
        assert e <= CEIL, (name, e)


@pytest.mark.gpu
def test_profile_shows_which_kernels_ran(dev):
    lib = _lib.load()
    B, N, ci, co = 1, 512, 128, 256
    P, X, W, dY = make_case("room", B, N, ci, co, seed=960)
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    for mode in ("highest", "medium"):
        seen = _profile(lib, lambda: _run(dev, cache, mode, P, X, W, dY, (1, 1, 1)))
        bf16 = (seen["deep_gemm_bf16_kernel"], seen["deep_dw_bf16_kernel"])
        fp32 = (seen["deep_gemm_kernel"], seen["deep_dw_kernel"])
        if mode == "highest":
            assert fp32 == (2, 1) and bf16 == (0, 0), (mode, seen)
        else:
            assert bf16 == (2, 1) and fp32 == (0, 0), (mode, seen)


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co,s,dtype", [(3, 9, 1, np.float32), (9, 9, 2, np.float32), (36, 13, 1, np.float32),
                                           (32, 64, 1, np.float64)])
def test_modes_are_a_bitwise_no_op_off_the_matrix_core_path(dev, ci, co, s, dtype):
    """Register-path shapes and fp64 ignore the bits: every mode gives the "highest" bits."""
    B, N = 2, 1024
    P, X, W, dY = make_case("room", B, N, ci, co, seed=970, dtype=dtype)
    cache = op.NeighborCache(B, N, torch.from_numpy(P).dtype, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    ref = _run(dev, cache, "highest", P, X, W, dY, (s, s, s))
    for u, v in zip(_run(dev, cache, "medium", P, X, W, dY, (s, s, s)), ref):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_switching_modes_on_one_cache_leaks_nothing_and_runs_reproduce(dev):
    """highest -> medium -> highest on one cache: the third call equals the first bit for bit (no packed filter, no
    mark left behind); two medium runs are bitwise equal."""
    B, N, ci, co = 2, 700, 64, 128
    P, X, W, dY = make_case("room", B, N, ci, co, seed=980)
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    first = _run(dev, cache, "highest", P, X, W, dY, (1, 1, 1))
    med = _run(dev, cache, "medium", P, X, W, dY, (1, 1, 1))
    third = _run(dev, cache, "highest", P, X, W, dY, (1, 1, 1))
    for u, v in zip(first, third):
        assert torch.equal(u, v)
    assert not torch.equal(first[0], med[0])
    again = _run(dev, cache, "medium", P, X, W, dY, (1, 1, 1))
    for u, v in zip(med, again):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_non_finite_values_in_medium_mode_reach_only_their_neighbours(dev):
    """Tiles that meet Inf / NaN go to the exact generic kernel in every mode: the non-finite outputs are exactly the
    reference's, the finite ones within the medium ceiling."""
    from oracle import oracle
    B, N, ci, co = 1, 300, 32, 64
    P, X, W, dY = make_case("room", B, N, ci, co, seed=1040)
    X = X.copy(); dY = dY.copy()
    X[0, 17, 3] = np.inf
    X[0, 200, 0] = np.nan
    dY[0, 99, 5] = np.inf
    s = (1, 1, 1)
    with np.errstate(all="ignore"):
        y_ref = oracle.forward(P, X, W, s, VOX)
        dx_ref, dw_ref = oracle.backward(dY, P, X, W, s, VOX)
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    got = _run(dev, cache, "medium", P, X, W, dY, s)
    for g, ref in zip(got, (y_ref, dx_ref, dw_ref)):
        g = g.cpu().numpy()
        bad_ref = ~np.isfinite(ref)
        assert bad_ref.any() and not bad_ref.all()
        assert np.array_equal(~np.isfinite(g), bad_ref)
        ok = ~bad_ref
        assert np.max(np.abs(g[ok] - ref[ok])) <= CEIL * max(1.0, np.max(np.abs(ref[ok])))


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co,N", [(320, 320, 2048), (32, 64, 9000)])
def test_blocked_layers_and_several_search_groups_honour_the_mode(dev, ci, co, N):
    """A layer of more than 256 channels (channel blocks on the matrix-core kernels) and a cloud searched in several
    groups (N > 8192) run the bf16 kernels and stay within the ceiling."""
    lib = _lib.load()
    B = 1
    P = synth.modelnet_like(B, N, seed=990) if ci > 256 else synth.room_like(B, N, 990, extent=(2.0, 2.0, 1.5))
    X = synth.features(B, N, ci, 991, points=P)
    W = synth.filter_weights(3, 3, 3, ci, co, 992)
    dY = synth.upstream_grad(B, N, co, 993)
    ref = _exact(P, X, W, dY, (1, 1, 1))
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    highest = _run(dev, cache, "highest", P, X, W, dY, (1, 1, 1))
    out = []
    seen = _profile(lib, lambda: out.append(_run(dev, cache, "medium", P, X, W, dY, (1, 1, 1))))
    assert seen["deep_gemm_bf16_kernel"] >= 2 and seen["deep_dw_bf16_kernel"] >= 1, seen
    assert seen["deep_gemm_kernel"] == 0 and seen["deep_dw_kernel"] == 0, seen
    assert not torch.equal(out[0][0], highest[0])
    for name, e in zip(("y", "dX", "dW"), _errs(out[0], ref)):
        assert e <= CEIL, (name, e)


@pytest.mark.gpu
def test_invalid_precision_is_rejected(dev):
    B, N, ci, co = 1, 256, 64, 64
    with pytest.raises(op.Conv3pInvalidArgument):
        op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co, matmul_precision="low")
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=1, max_taps=27, max_cin=ci, max_cout=co)
    with pytest.raises(op.Conv3pInvalidArgument):
        cache.matmul_precision = "high"
    assert cache.matmul_precision == "highest"
