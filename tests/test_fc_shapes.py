"""GPU tests of the dense head's FC kernels (csrc/conv3p_head.hpp, the fused twins of csrc/conv3p_optim.hpp) over the
launch planner's whole space: the case table of tests/fc_ref.py, which tests/test_fc_plan_host.py shows to reach every
branch of fc_plan / fc_waves / the dW kernel's STEPS.

Tolerances.  None is a free-standing number:
  * integer inputs in [-3, 3]: every product and partial sum is an integer below 2^24, so every summation order gives
    the same float32 -- the comparison with the int64 matmul is exact (zero tolerance);
  * full-mantissa inputs: a sum of n float32 products in any order is within gamma_n sum |a||b| of the exact one,
    gamma_n = n u / (1 - n u), u = 2^-24 (fc_ref.gamma), applied per element;
  * SELU: SELU_ULPS units in the last place of |y|.  HIP's math documentation states the bound e of the device expm1f
    that expm1_t calls (the bound would then be e + 2: two constants, two products); it does not ship with ROCm and
    was not at hand when these tests were written, so the bound is MEASURED instead: the kernel's SELU of the integers
    -104 .. 0 (M = 1, exact pre-activations) against float64 numpy (scale * alpha * expm1 in double) is off by at most
    0.960 ulp on an MI355X (test_selu_of_exact_integers prints the figure and asserts it has not grown); SELU_ULPS is
    that worst case, rounded up in its third decimal, plus 1 ulp.
"""
import numpy as np
import pytest

from tests import fc_ref
from tests.fc_ref import case_id

SELU_MEASURED_ULPS = 0.961        # worst |y - selu64(v)| / ulp(|y|) over v = -104 .. 0 on an MI355X (see the docstring)
SELU_ULPS = SELU_MEASURED_ULPS + 1.0
SENTINEL = -7.5                   # no integer result and no guard value can equal it
GUARD_ROWS = 2

SERVED = fc_ref.CASES + fc_ref.BORDER_INSIDE
FLOAT_CASES = [c for c in fc_ref.CASES if c[1] <= 8193]


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)             # (a copy: the shared references are read-only)


def same(got, want):
    """A device tensor against a numpy array: dtype, shape and every value (an Inf equals an Inf of its sign, a NaN
    nothing), compared on the device."""
    import torch
    return got.dtype == torch.float32 and want.dtype == np.float32 and torch.equal(got, to(got.device, want))


class Guarded:
    """A contiguous (rows, cols) float32 output inside a larger buffer: GUARD_ROWS rows' worth of SENTINEL before and
    after it, and SENTINEL in it (a store past either end, or an element never written, shows)."""

    def __init__(self, dev, rows, cols):
        import torch
        self.buf = torch.full(((rows + 2 * GUARD_ROWS) * cols,), SENTINEL, dtype=torch.float32, device=dev)
        self.lo, self.hi = GUARD_ROWS * cols, (GUARD_ROWS + rows) * cols
        self.t = self.buf[self.lo:self.hi].view(rows, cols)

    def guards_untouched(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------- (a) exact, and (g) borders
@pytest.mark.gpu
@pytest.mark.parametrize("case", SERVED, ids=case_id)
def test_integer_inputs_give_the_int64_results_bit_for_bit(dev, case):
    """act = 0 on integers in [-3, 3]: y (with and without bias), dx, dW, db equal the int64 matmuls exactly.  The rows
    of fc_ref.BORDER_INSIDE are one step inside each border of the backward's LDS limit."""
    from pointwise_amd import head
    M, K, N = case
    c = fc_ref.int_case(M, K, N)
    x, W, b, dy = (to(dev, a) for a in (c.x, c.W, c.b, c.dy))
    y = head.fully_connected(x, W, b, selu=False)
    assert same(y, c.v)
    assert same(head.fully_connected(x, W, None, selu=False), c.v_nobias)
    dx, dW, db = head.fully_connected_grad(x, W, y, dy, selu=False)
    assert same(dx, c.dx) and same(dW, c.dW) and same(db, c.db)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SERVED, ids=case_id)
def test_gradients_without_dx_into_caller_given_tensors(dev, case):
    """need_dx = False, dW_out / db_out given and pre-filled with a sentinel, between guard rows of the same sentinel:
    dW and db are exact, every element is written, nothing around them is."""
    from pointwise_amd import head
    M, K, N = case
    c = fc_ref.int_case(M, K, N)
    x, W, y, dy = (to(dev, a) for a in (c.x, c.W, c.v, c.dy))
    gW, gb = Guarded(dev, K, N), Guarded(dev, 1, N)
    none, dW2, db2 = head.fully_connected_grad(x, W, y, dy, selu=False, need_dx=False, dW_out=gW.t, db_out=gb.t[0])
    assert none is None and dW2 is gW.t
    assert same(gW.t, c.dW) and same(gb.t[0], c.db)
    assert gW.guards_untouched() and gb.guards_untouched()


def selu_ulps(y, v):
    """max |y - selu(v)| in units of the float32 spacing at |selu(v)| (v exact, selu in float64)."""
    want = fc_ref.selu64(v)
    return float((np.abs(y.astype(np.float64) - want) / fc_ref.ulp32(want)).max())


@pytest.mark.gpu
def test_selu_of_exact_integers(dev):
    """The measurement behind SELU_ULPS: M = 1, K = 1, x = 1, W = -104 .. 0 (exp underflows past -104), no bias."""
    from pointwise_amd import head
    v = np.zeros(112, dtype=np.float32)
    v[:105] = np.arange(-104, 1)
    y = head.fully_connected(to(dev, np.ones((1, 1), np.float32)), to(dev, v[None, :]), None, selu=True).cpu().numpy()[0]
    worst = selu_ulps(y, v)
    print("SELU of the integers -104 .. 0: worst %.3f ulp of |y| against float64" % worst)
    assert worst <= SELU_MEASURED_ULPS


@pytest.mark.gpu
@pytest.mark.parametrize("case", SERVED, ids=case_id)
def test_selu_of_exact_preactivations(dev, case):
    """act = 1 on the integer inputs: the pre-activation is exact, so y differs from float64 selu(v) only by the
    activation's own rounding, SELU_ULPS ulp of |y|."""
    from pointwise_amd import head
    M, K, N = case
    c = fc_ref.int_case(M, K, N)
    y = head.fully_connected(to(dev, c.x), to(dev, c.W), to(dev, c.b), selu=True).cpu().numpy()
    worst = selu_ulps(y, c.v)
    print("%s: worst %.3f ulp" % (case_id(case), worst))
    assert worst <= SELU_ULPS


# ---------------------------------------------------------------------------------------- (b) the slope
@pytest.mark.gpu
def test_selu_slope_bit_for_bit(dev):
    """M = 1, act = 1: db[n] = 0 + dy[n] * slope(y[n]) with the slope's two float32 roundings (fc_ref.selu_slope32), at
    the values of y where a different rounding, a flushed subnormal or a comparison written the other way shows."""
    from pointwise_amd import head
    K, N = 8, 256
    rng = np.random.default_rng(5)
    c = np.float32(fc_ref.SELU_SCALE * fc_ref.SELU_ALPHA)
    tiny = np.float32(-1.4e-45)
    assert tiny < 0 and tiny.view(np.uint32) == 0x80000001
    special = np.array([0.0, -0.0, tiny, -c, np.nextafter(-c, np.float32(0)), np.nextafter(-c, np.float32(-np.inf)),
                        np.nan, np.inf, -np.inf, -1.0, 1.0, np.float32(-1.7580993), np.float32(-1e-30)], dtype=np.float32)
    y = (rng.standard_normal(N) * 2).astype(np.float32)
    y[:special.size] = special
    y[64:128] = -np.abs(rng.standard_normal(64)).astype(np.float32)            # selu's negative range (-c, 0)
    dy = rng.standard_normal(N).astype(np.float32)
    assert (dy != 0).all()
    x, W = rng.standard_normal((1, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    _, dW, db = head.fully_connected_grad(to(dev, x), to(dev, W), to(dev, y[None, :]), to(dev, dy[None, :]), selu=True,
                                          need_dx=False)
    with np.errstate(invalid="ignore"):
        want = np.float32(0) + fc_ref.dz32(y, dy, True)                          # fc_dz_kernel: s = 0.0f; s += g
    got = db.cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert got[7] == dy[7] * np.float32(fc_ref.SELU_SCALE) and np.isinf(got[8]) and np.sign(got[8]) == -np.sign(dy[8])
    assert got[2] == np.float32(dy[2] * c) and got[3] == 0 and got[1] == dy[1] * np.float32(fc_ref.SELU_SCALE)
    # dW = x^T dz with one batch row: a single product per element, and the NaN stays in its column
    dWn = dW.cpu().numpy()
    with np.errstate(invalid="ignore"):
        dz = fc_ref.dz32(y, dy, True)
        wantW = (x[0][:, None] * dz[None, :]).astype(np.float32)
    assert np.array_equal(np.isnan(dWn), np.isnan(wantW)) and np.array_equal(dWn[:, ~nan], wantW[:, ~nan])


# ---------------------------------------------------------------------------------------- (c) full-mantissa floats
@pytest.mark.gpu
@pytest.mark.parametrize("act", [False, True], ids=["identity", "selu"])
@pytest.mark.parametrize("case", FLOAT_CASES, ids=case_id)
def test_standard_normal_inputs_within_the_gamma_bounds(dev, case, act):
    """Per element, with gamma_n = n u / (1 - n u), u = 2^-24, and everything on the right in float64:
        y  (act = 0)   gamma_{K+1} (|x| |W| + |b|);   act = 1: SCALE ALPHA (SELU's largest slope) times that, plus
                       SELU_ULPS ulp of |y|
        dx             gamma_N |dz| |W^T|
        dW             gamma_M |x^T| |dz|
        db             gamma_M sum_m |dz|
    dz is the kernel's own float32 rule (fc_ref.dz32) on the kernel's y, so only the accumulation is judged.  A bf16
    or tf32 product would be off by 2^-9 or 2^-11 of sum |a||b| against gamma_{K+1} <= 2^-10.9 at K = 8193 and
    2^-16 at K = 256: this is the check that the products are true fp32."""
    from pointwise_amd import head
    M, K, N = case
    rng = np.random.default_rng([M, K, N, 1])
    x, W, dy = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (K, N), (M, N)))
    b = rng.standard_normal(N).astype(np.float32)
    x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    yt = head.fully_connected(to(dev, x), to(dev, W), to(dev, b), selu=act)
    y = yt.cpu().numpy()
    v = x64 @ W64 + b64
    bound = fc_ref.gamma(K + 1) * (np.abs(x64) @ np.abs(W64) + np.abs(b64))
    if act:
        want = fc_ref.selu64(v)
        bound = fc_ref.SELU_SCALE * fc_ref.SELU_ALPHA * bound + SELU_ULPS * fc_ref.ulp32(want)
    else:
        want = v
    assert (np.abs(y - want) <= bound).all(), float((np.abs(y - want) / bound).max())
    dx, dW, db = head.fully_connected_grad(to(dev, x), to(dev, W), yt, to(dev, dy), selu=act)
    dz = fc_ref.dz32(y, dy, act).astype(np.float64)
    for name, got, ref, bnd in (("dx", dx, dz @ W64.T, fc_ref.gamma(N) * (np.abs(dz) @ np.abs(W64.T))),
                                ("dW", dW, x64.T @ dz, fc_ref.gamma(M) * (np.abs(x64.T) @ np.abs(dz))),
                                ("db", db, dz.sum(axis=0), fc_ref.gamma(M) * np.abs(dz).sum(axis=0))):
        err = np.abs(got.cpu().numpy() - ref)
        assert (err <= bnd).all(), (name, float(err.max()))


# ---------------------------------------------------------------------------------------- (d) subnormals
@pytest.mark.gpu
@pytest.mark.parametrize("ex,ew", [(-100, -30), (-130, 3)], ids=["subnormal-products", "subnormal-inputs"])
def test_subnormal_products_and_inputs_are_not_flushed(dev, ex, ew):
    """K = 4.  x = i 2^ex, W = j 2^ew with small integers i, j: 2^-100 2^-30 has subnormal products and sums, 2^-130 is a
    subnormal input (times 8).  The sums are integer multiples of 2^(ex+ew) with a few bits: float32 holds them
    exactly, so y, dx (from dy like x) and dW (from dy like W) must equal the float64 results bit for bit."""
    from pointwise_amd import head
    M, K, N = 3, 4, 8
    rng = np.random.default_rng(9)
    ints = lambda *s: rng.integers(1, 4, size=s) * rng.choice([-1, 1], size=s)
    x = (ints(M, K) * 2.0 ** ex).astype(np.float32)
    W = (ints(K, N) * 2.0 ** ew).astype(np.float32)
    dy_small = (ints(M, N) * 2.0 ** ex).astype(np.float32)
    dy_large = (ints(M, N) * 2.0 ** ew).astype(np.float32)

    def exact32(a64):
        a32 = a64.astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), a64) and (a32 != 0).any()
        return a32
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    assert 2.0 ** (ex + ew) < 2.0 ** -126 and (x != 0).all() and (W != 0).all()   # every product is subnormal
    y = head.fully_connected(to(dev, x), to(dev, W), None, selu=False)
    want_y = exact32(x64 @ W64)
    assert same(y, want_y)
    dx, _, db = head.fully_connected_grad(to(dev, x), to(dev, W), y, to(dev, dy_small), selu=False)
    assert same(dx, exact32(dy_small.astype(np.float64) @ W64.T)) and same(db, exact32(dy_small.astype(np.float64).sum(axis=0)))
    _, dW, _ = head.fully_connected_grad(to(dev, x), to(dev, W), y, to(dev, dy_large), selu=False)
    assert same(dW, exact32(x64.T @ dy_large.astype(np.float64)))


# ---------------------------------------------------------------------------------------- (e) non-finite values
def small_ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def nonzero(a):
    a[a == 0] = 1
    return a


def planted_sum(a, b):
    """sum_i a[..., i] * b[..., i] in float64, written out elementwise (no BLAS): the row or column a planted Inf enters."""
    with np.errstate(invalid="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64)).sum(axis=-1).astype(np.float32)


@pytest.mark.gpu
def test_inf_in_the_last_row_of_w_reaches_one_column_of_y(dev):
    """W[K-1][n0] = +Inf with K odd and the last K-chunk of odd length (13 of kc = 32): the forward's padded MFMA step
    re-reads that row against x == 0.  y[:, n0] = +-Inf by the sign of x[:, K-1]; every other element is exact."""
    from pointwise_amd import head
    M, K, N, n0 = 5, 77, 16, 5
    assert fc_ref.plan_row(M, K, N).last == 13
    rng = np.random.default_rng(21)
    x, W, b = small_ints(rng, M, K), small_ints(rng, K, N), small_ints(rng, N)
    nonzero(x[:, K - 1])
    W[K - 1, n0] = np.inf
    Wz = W.copy()
    Wz[K - 1, n0] = 0
    want = (fc_ref.imatmul(x, Wz) + b.astype(np.int64)).astype(np.float32)
    want[:, n0] = planted_sum(x, W[None, :, n0]) + b[n0]
    assert np.isinf(want[:, n0]).all() and np.array_equal(np.sign(want[:, n0]), np.sign(x[:, K - 1]))
    assert same(head.fully_connected(to(dev, x), to(dev, W), to(dev, b), selu=False), want)


@pytest.mark.gpu
def test_inf_in_the_last_column_of_w_reaches_one_column_of_dx(dev):
    """W[k0][N-1] = -Inf with N / 8 = 3 steps of 8 padded ones: fc_dx_kernel's clamped steps re-read the row's last
    columns against dz == 0.  dx[:, k0] = -+Inf by the sign of dy[:, N-1]; the rest of dx, dW and db are exact."""
    from pointwise_amd import head
    M, K, N, k0 = 5, 50, 24, 17
    rng = np.random.default_rng(22)
    x, W, dy = small_ints(rng, M, K), small_ints(rng, K, N), small_ints(rng, M, N)
    nonzero(dy[:, N - 1])
    W[k0, N - 1] = -np.inf
    Wz = W.copy()
    Wz[k0, N - 1] = 0
    want = fc_ref.imatmul(dy, Wz.T).astype(np.float32)
    want[:, k0] = planted_sum(dy, W[None, k0, :])
    assert np.isinf(want[:, k0]).all() and np.array_equal(np.sign(want[:, k0]), -np.sign(dy[:, N - 1]))
    dx, dW, db = head.fully_connected_grad(to(dev, x), to(dev, W), to(dev, np.zeros_like(dy)), to(dev, dy), selu=False)
    assert same(dx, want)
    assert same(dW, fc_ref.imatmul(x.T, dy).astype(np.float32)) and same(db, dy.sum(axis=0))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused-step"])
@pytest.mark.parametrize("M", [7, 40, 70])
def test_inf_in_the_last_row_of_x_reaches_one_row_of_dw(dev, M, fused):
    """x[M-1][k0] = +Inf: the dW kernels read the rows of a padded batch (7 of 32, 40 of 64, 70 of 128) from row M - 1,
    against dz == 0.  dW[k0][:] = +-Inf by the sign of dy[M-1][:]; the rest of dW, dx and db are exact.  Through
    fused_fc_step with lr = 0 and momentum = 0 from zero accumulators the accumulators ARE dW and db."""
    import torch
    from pointwise_amd import head
    from pointwise_amd.optim import MomentumOptimizer
    K, N, k0 = 50, 24, 17
    rng = np.random.default_rng(23 + M)
    x, W, b, dy = small_ints(rng, M, K), small_ints(rng, K, N), small_ints(rng, N), small_ints(rng, M, N)
    nonzero(dy[M - 1, :])
    x[M - 1, k0] = np.inf
    xz = x.copy()
    xz[M - 1, k0] = 0
    want = fc_ref.imatmul(xz.T, dy).astype(np.float32)
    want[k0, :] = planted_sum(dy.T, x[None, :, k0])
    assert np.isinf(want[k0, :]).all() and np.array_equal(np.sign(want[k0, :]), np.sign(dy[M - 1, :]))
    want_dx, want_db = fc_ref.imatmul(dy, W.T).astype(np.float32), dy.sum(axis=0)
    xt, Wt, bt, dyt, yt = to(dev, x), to(dev, W), to(dev, b), to(dev, dy), to(dev, np.zeros_like(dy))
    if fused:
        opt = MomentumOptimizer([Wt, bt], 0.0, 0.0)
        dx = opt.fused_fc_step(xt, Wt, bt, yt, dyt, selu=False)
        dW, db = opt.accums
    else:
        dx, dW, db = head.fully_connected_grad(xt, Wt, yt, dyt, selu=False)
    assert same(dW, want), int(torch.isnan(dW).sum())
    assert same(dx, want_dx) and same(db, want_db)


# ---------------------------------------------------------------------------------------- (f) independence
@pytest.mark.gpu
def test_rows_scratch_stream_and_repetition_do_not_change_a_bit(dev):
    import torch
    from pointwise_amd import head
    from pointwise_amd._host import _HEADS
    M, K, N = 128, 200, 40
    rng = np.random.default_rng(31)
    x, W, b, dy = (to(dev, rng.standard_normal(s).astype(np.float32)) for s in ((M, K), (K, N), (N,), (M, N)))

    def run():
        y = head.fully_connected(x, W, b, selu=True)
        return (y,) + tuple(head.fully_connected_grad(x, W, y, dy, selu=True))
    first = run()
    for a, c in zip(first, run()):                                             # a second call
        assert torch.equal(a, c)
    for buf in _HEADS.values():                                                # whatever the scratch held before
        buf.fill_(0xFF)
    for a, c in zip(first, run()):
        assert torch.equal(a, c)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for buf in _HEADS.values():
            buf.fill_(0xFF)
        other = run()
    side.synchronize()
    for a, c in zip(first, other):
        assert torch.equal(a, c)
    y, dx = first[0], first[1]
    for m in range(M):                                                         # row m alone, as a batch of one
        y1 = head.fully_connected(x[m:m + 1], W, b, selu=True)
        dx1, _, _ = head.fully_connected_grad(x[m:m + 1], W, y1, dy[m:m + 1], selu=True)
        assert torch.equal(y1, y[m:m + 1]) and torch.equal(dx1, dx[m:m + 1]), m


# ---------------------------------------------------------------------------------------- (g) the empty batch
@pytest.mark.gpu
def test_empty_batch_gives_zero_gradients(dev):
    """M = 0: dW = x^T dz and db = sum_m dz are empty sums, dx has no rows."""
    import torch
    from pointwise_amd import head
    K, N = 70, 24
    x, y, dy = (torch.empty((0, c), dtype=torch.float32, device=dev) for c in (K, N, N))
    W = torch.ones((K, N), dtype=torch.float32, device=dev)
    gW, gb = Guarded(dev, K, N), Guarded(dev, 1, N)
    dx, dW, db = head.fully_connected_grad(x, W, y, dy, selu=True, dW_out=gW.t, db_out=gb.t[0])
    assert tuple(dx.shape) == (0, K) and dW is gW.t
    assert bool((gW.t == 0).all()) and bool((gb.t == 0).all())
    assert gW.guards_untouched() and gb.guards_untouched()
    assert tuple(head.fully_connected(x, W, None, selu=True).shape) == (0, N)


# ---------------------------------------------------------------------------------------- (h) the fused step
@pytest.mark.gpu
@pytest.mark.parametrize("case", SERVED, ids=case_id)
def test_fused_fc_step_equals_grad_then_step_over_the_table(dev, case):
    """tests/test_optim.py's test_fused_fc_step_equals_grad_then_step over every row of the table: W, b, both
    accumulators and dx after fused_fc_step against fully_connected_grad followed by step on copies, bit for bit, from
    non-zero accumulators; then without a bias and without dx."""
    import torch
    from pointwise_amd import head
    from pointwise_amd.optim import MomentumOptimizer
    M, K, N = case
    g = torch.Generator().manual_seed(M * 7 + K)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, W, b, dy = rnd(M, K), rnd(K, N) * 0.05, rnd(N), rnd(M, N)
    aW, ab = rnd(K, N), rnd(N)
    y = head.fully_connected(x, W, b, selu=True)
    W2, b2 = W.clone(), b.clone()
    lr, mom = 0.05, 0.9
    opt, opt2 = MomentumOptimizer([W, b], lr, mom), MomentumOptimizer([W2, b2], lr, mom)
    for o in (opt, opt2):
        o.accums[0].copy_(aW)
        o.accums[1].copy_(ab)
    dx2, dW, db = head.fully_connected_grad(x, W2, y, dy, selu=True)         # dx2: from the OLD W
    opt2.step([dW, db])
    dx = opt.fused_fc_step(x, W, b, y, dy, selu=True)
    assert not torch.equal(opt2.accums[0], aW)
    assert torch.equal(dx, dx2)
    assert torch.equal(opt.accums[0], opt2.accums[0]) and torch.equal(opt.accums[1], opt2.accums[1])
    assert torch.equal(W, W2) and torch.equal(b, b2)
    assert opt.global_step == 0 and opt2.global_step == 1                    # the fused call is not a step() by itself
    del dx, dx2, dW, aW, opt2, W2
    W3, W4 = W.clone(), W.clone()
    o3, o4 = MomentumOptimizer([W3], lr, mom), MomentumOptimizer([W4], lr, mom)
    y3 = head.fully_connected(x, W3, None, selu=False)
    _, dW3, _ = head.fully_connected_grad(x, W4, y3, dy, selu=False, need_dx=False)
    o4.step([dW3])
    assert o3.fused_fc_step(x, W3, None, y3, dy, selu=False, need_dx=False) is None
    assert torch.equal(W3, W4) and torch.equal(o3.accums[0], o4.accums[0]) and not torch.equal(W3, W)
