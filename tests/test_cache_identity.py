"""NeighborCache(trust_tensor_identity=True) (-m gpu): the cache may vouch for a points tensor (CONV3P_CACHE_POINTS_UNCHANGED)
only while its buffer holds that tensor's geometry.  Two sequences that used to break it: a cache_prepare of other
clouds between two op calls on the same tensor, and an op call that fails after the tensor was recorded."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pointwise_amd import _lib, conv3p_op as op
from tests.parity_util import TOL, make_case, rel_err

pytestmark = pytest.mark.gpu
VOX = 0.1
S = (1, 1, 1)
FILT = (3, 3, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _clouds(dev):
    B, N = 2, 512
    PX, X, W, dY = make_case("modelnet", B, N, 3, 9, FILT, seed=3100)
    PY = make_case("modelnet", B, N, 3, 9, FILT, seed=3101)[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cache = op.NeighborCache(B, N, torch.float32, dev, slots=2, max_taps=27, max_cin=3, max_cout=9, trust_tensor_identity=True)
    return (PX, X, W, dY), (t(PX), t(PY), t(X), t(W), t(dY)), cache


def _final_call_matches(dev, host, tens, cache):
    """The op on cloud X through `cache` against the stateless op (bit for bit) and the oracle."""
    PX, X, W, dY = host
    tpx, _, tx, tw, tdy = tens
    y = op.conv3p(tpx, tx, tw, S, VOX, cache=cache)
    dx, dw = op.conv3p_grad(tdy, tpx, tx, tw, S, VOX, cache=cache)
    y0 = op.conv3p(tpx, tx, tw, S, VOX)
    dx0, dw0 = op.conv3p_grad(tdy, tpx, tx, tw, S, VOX)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(dx, dx0) and torch.equal(dw, dw0), "cached result differs from the stateless one"
    tol_y, tol_w = TOL[np.dtype(np.float32)]
    rdx, rdw = oracle.backward(dY, PX, X, W, S, VOX)
    assert rel_err(y.cpu().numpy(), oracle.forward(PX, X, W, S, VOX)) <= tol_y
    assert rel_err(dx.cpu().numpy(), rdx) <= tol_y
    assert rel_err(dw.cpu().numpy(), rdw) <= tol_w


@pytest.mark.parametrize("prepare", ["cache_prepare", "cache_prepare_multi"])
def test_prepare_of_other_clouds_voids_the_identity_record(dev, prepare):
    """conv3p(X, cache), then a prepare of clouds Y in the same cache, then conv3p(X, cache) again: the last call must
    not promise unchanged points -- the cache holds Y's geometry."""
    host, tens, cache = _clouds(dev)
    tpx, tpy, tx, tw, _ = tens
    op.conv3p(tpx, tx, tw, S, VOX, cache=cache)
    if prepare == "cache_prepare":
        op.cache_prepare(tpy, FILT, S, VOX, cache)
    else:
        op.cache_prepare_multi(tpy, FILT, [S, (2, 2, 2)], VOX, cache)
    _final_call_matches(dev, host, tens, cache)


def test_failed_call_does_not_record_its_points(dev):
    """conv3p(Y, cache), then a call on X that the library refuses (voxel size 0), then conv3p(X, cache): the failed call
    validated nothing, so X must not count as the tensor the cache holds."""
    host, tens, cache = _clouds(dev)
    tpx, tpy, tx, tw, _ = tens
    op.conv3p(tpy, tx, tw, S, VOX, cache=cache)
    with pytest.raises(op.Conv3pInvalidArgument):
        op.conv3p(tpx, tx, tw, S, 0.0, cache=cache)
    _final_call_matches(dev, host, tens, cache)
