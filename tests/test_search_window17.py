"""The fused search's window tables hold 16 + 1 buckets per one-voxel interval and the look-up adds a second window only
where the rounding fuzz carries it over a bucket boundary (conv3p_search_fused.hpp, the superset argument above
fused_mask).  A neighbour lost to the dropped bucket would sit at the far end of a tap interval, so the clouds here are
built from such neighbours: around every centre p, points at p + (k step - full/2 + {0, 1}) voxel on each axis -- both
edges of every tap interval -- moved by 0, +-1, +-4 ulps and by +-(voxel/16 +- 1 ulp), the width of a base bucket.
Populations must equal the oracle's integer for integer, one forward + backward must stay within the stated tolerances
(tests/parity_util.py), at several coordinate magnitudes (the look-up slack scales with |p|: at 1e4 the search takes every
valid candidate), over clouds whose tiles span 5 .. 30 voxels (tables at the base resolution and coarsened one to three
times), through the three-tap look-ups and the general loop, with a tile of one repeated point and with non-finite points.
Every case asserts that the oracle finds more than the self pairs."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pointwise_amd import _lib, conv3p_op as op, synth
from tests.parity_util import TOL, exact_from_oracle_lists, rel_err

pytestmark = pytest.mark.gpu
VOX = 0.1
B = 2
# per-axis moves of a placed neighbour: (multiples of voxel / 16, ulps)
MOVES = [(0, 0), (0, 1), (0, -1), (0, 4), (0, -4), (1, 1), (1, -1), (-1, 1), (-1, -1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def _ulps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


def boundary_cloud(N, span, ext_xyz, step_xyz, offset, rng):
    """One cloud of N points inside a cube of `span` voxels at `offset`: groups of a centre and seven neighbours, each
    neighbour on an edge of a tap interval of the centre on every axis (a tap that keeps it inside the cube; tap
    (ext - 1) / 2 .. always does for a centre 0.6 voxel inside), moved by one of MOVES."""
    v = float(np.float32(VOX))
    pts = np.empty((N, 3), dtype=np.float32)
    n = 0
    while n < N:
        c = (offset + rng.uniform(0.6, span - 0.6, size=3) * v).astype(np.float32)
        pts[n] = c
        n += 1
        for _ in range(min(7, N - n)):
            for a in range(3):
                full = (ext_xyz[a] - 1) * step_xyz[a] + 1
                edges = [k * step_xyz[a] - full / 2.0 + hi for k in range(ext_xyz[a]) for hi in (0, 1)]
                inside = [d for d in edges if offset + 0.05 * v <= float(c[a]) + d * v <= offset + (span - 0.05) * v]
                d = inside[rng.integers(len(inside))]
                sixteenths, ulps = MOVES[rng.integers(len(MOVES))]
                pts[n, a] = _ulps(np.float32(float(c[a]) + d * v + sixteenths * v / 16.0), ulps)
            n += 1
    return pts[rng.permutation(N)]


def make_inputs(P, fzyx, seed):
    N = P.shape[1]
    X = synth.features(B, N, 3, seed + 1, points=P, dtype=np.float32)
    W = synth.filter_weights(*fzyx, 3, 9, seed + 2, dtype=np.float32)
    dY = synth.upstream_grad(B, N, 9, seed + 3, dtype=np.float32)
    return X, W, dY


def run_hip(dev, P, X, W, dY, s):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tx, tw, tdy = t(P), t(X), t(W), t(dY)
    cnt = op.neighbor_count(tp, W.shape[:3], s, VOX)
    y = op.conv3p(tp, tx, tw, s, VOX)
    dx, dw = op.conv3p_grad(tdy, tp, tx, tw, s, VOX)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), y.cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy()


def check_case(dev, P, fzyx, s, seed, dense=False):
    """dense: the cloud holds a pile of identical points, whose N^2 same-tap terms put the reference's own fp32
    grad_filter further than 2e-5 from the exact sums over ITS pair lists; the bar is then 4 x that error, as in
    tests/test_gpu_parity.py::check_against."""
    X, W, dY = make_inputs(P, fzyx, seed)
    cnt_ref = oracle.neighbor_count(P, fzyx, s, VOX)
    assert 2 * int(cnt_ref.sum()) >= 3 * P.shape[0] * P.shape[1], "the oracle finds hardly more than the self pairs"
    y_ref = oracle.forward(P, X, W, s, VOX)
    dx_ref, dw_ref = oracle.backward(dY, P, X, W, s, VOX)
    cnt, y, dx, dw = run_hip(dev, P, X, W, dY, s)
    tol_y, tol_w = TOL[np.dtype(np.float32)]
    if dense:
        dw_exact = sum(exact_from_oracle_lists(P[b], X[b], W, dY[b], s, VOX)[2] for b in range(P.shape[0]))
        tol_w = max(tol_w, 4.0 * rel_err(dw_ref, dw_exact))
    assert np.array_equal(cnt, cnt_ref), "neighbour / tap decisions differ from the CPU reference"
    assert rel_err(y, y_ref) <= tol_y, ("y", rel_err(y, y_ref))
    assert rel_err(dx, dx_ref) <= tol_y, ("dX", rel_err(dx, dx_ref))
    assert rel_err(dw, dw_ref) <= tol_w, ("dW", rel_err(dw, dw_ref))


def boundary_batch(N, span, ext_xyz, step_xyz, offset, seed):
    rng = np.random.default_rng(seed)
    return np.stack([boundary_cloud(N, span, ext_xyz, step_xyz, offset, rng) for _ in range(B)])


@pytest.mark.parametrize("offset", [0.0, 1.0e2, 1.0e4])
@pytest.mark.parametrize("span", [5, 7, 13, 30])
@pytest.mark.parametrize("stride", [1, 2, 3, 4])
@pytest.mark.parametrize("N", [192, 320])
def test_neighbours_on_the_edges_of_every_tap_interval(dev, N, stride, span, offset):
    """3 x 3 x 3 taps (the nine-look-up form): 3 and 5 tiles per cloud, tiles of at most `span` voxels -- span 5 keeps
    the base resolution, 7 / 13 / 30 coarsen the tables of the wider tiles once, twice, three times."""
    s = (stride,) * 3
    seed = 4000 + 17 * N + 5 * stride + span
    P = boundary_batch(N, span, (3, 3, 3), s, offset, seed)
    check_case(dev, P, (3, 3, 3), s, seed)


@pytest.mark.parametrize("offset", [0.0, 1.0e2])
@pytest.mark.parametrize("span", [5, 13])
@pytest.mark.parametrize("s_xyz", [(2, 2, 2), (4, 2, 2)])
def test_general_look_up_loop_with_two_and_four_taps_per_axis(dev, s_xyz, span, offset):
    """A 2 x 4 x 4 filter (z, y, x) at even strides: every dilated extent is odd, so the stencil takes the fused search,
    through the general loop over the per-tap lower edges."""
    fzyx, ext_xyz = (2, 4, 4), (4, 4, 2)
    seed = 5000 + 7 * s_xyz[0] + span
    P = boundary_batch(320, span, ext_xyz, s_xyz, offset, seed)
    check_case(dev, P, fzyx, s_xyz, seed)


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_a_tile_of_one_repeated_point(dev, stride):
    """130 copies of one point fill at least one whole tile of the sorted cloud: a table whose every point shares one
    bucket per axis, next to tiles that span the cube."""
    s = (stride,) * 3
    seed = 6000 + stride
    rng = np.random.default_rng(seed)
    clouds = []
    for _ in range(B):
        c = boundary_cloud(190, 7, (3, 3, 3), s, 0.0, rng)
        clouds.append(np.concatenate([c, np.repeat(c[:1], 130, axis=0)])[rng.permutation(320)])
    check_case(dev, np.stack(clouds), (3, 3, 3), s, seed, dense=True)


@pytest.mark.parametrize("stride", [1, 3])
def test_non_finite_points_among_the_edge_neighbours(dev, stride):
    """Cloud 0 carries NaN / Inf points: no window holds them, they get empty masks as centres, and every other point
    keeps the populations, outputs and gradients it has without them (the oracle runs on the finite points)."""
    s, N, seed = (stride,) * 3, 320, 7000 + stride
    P = boundary_batch(N, 7, (3, 3, 3), s, 0.0, seed)
    X, W, dY = make_inputs(P, (3, 3, 3), seed)
    bad = np.array([5, 64, 131, 200, 319])
    P2 = P.copy()
    P2[0, bad[0], 0] = np.nan
    P2[0, bad[1], 1] = np.inf
    P2[0, bad[2], 2] = -np.inf
    P2[0, bad[3], :] = np.nan
    P2[0, bad[4], :] = np.inf
    keep = [np.setdiff1d(np.arange(N), bad), np.arange(N)]
    cnt, y, dx, dw = run_hip(dev, P2, X, W, dY, s)
    tol_y, tol_w = TOL[np.dtype(np.float32)]
    dw_ref = np.zeros(W.shape, dtype=np.float64)
    for b in range(B):
        k = keep[b]
        c = lambda a: np.ascontiguousarray(a[b:b + 1, k])
        cnt_ref = oracle.neighbor_count(c(P), (3, 3, 3), s, VOX)
        assert 2 * int(cnt_ref.sum()) >= 3 * len(k)
        assert np.array_equal(cnt[b, k], cnt_ref[0])
        y_ref = oracle.forward(c(P), c(X), W, s, VOX)
        dx_ref, dw_b = oracle.backward(c(dY), c(P), c(X), W, s, VOX)
        assert rel_err(y[b, k], y_ref[0]) <= tol_y and rel_err(dx[b, k], dx_ref[0]) <= tol_y
        dw_ref += dw_b
    assert not cnt[0, bad].any() and not y[0, bad].any()
    assert rel_err(dw, dw_ref) <= tol_w, ("dW", rel_err(dw, dw_ref))
