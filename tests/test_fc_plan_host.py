"""CPU tests (not gpu) of the dense head's launch planner: tests/fc_ref.py's mirror of fc_plan / fc_waves / the dW
kernel's STEPS and LDS is pinned to the library where the library exposes it (conv3p_fc_workspace_bytes, the status
codes decided before any launch), and the case table of tests/test_fc_shapes.py is shown to reach every branch of
that planner.  Nothing here launches: the pointers are fake, as in tests/test_optim_host.py, and only refused shapes
are handed to the entry points."""
import ctypes
import itertools

import numpy as np
import pytest

from pointwise_amd import _lib

from tests import fc_ref

FAKE = ctypes.c_void_p(256)                      # aligned, non-null, never dereferenced


def rows():
    return [fc_ref.plan_row(*c) for c in fc_ref.CASES]


def test_every_table_row_is_served_and_small_enough():
    for r in rows() + [fc_ref.plan_row(*c) for c in fc_ref.BORDER_INSIDE]:
        assert r.served, r
        assert r.K * r.N * 4 <= 100e6 and 9 * r.K + 3 < 2 ** 24, r        # W within ~100 MB; integer sums exact in float32
        assert fc_ref.lds_forward(r.kc) <= 64 * 1024 and fc_ref.lds_dx(r.K, r.N) <= fc_ref.K_MAX_LDS, r
        assert fc_ref.lds_dw(r.M, r.N) <= fc_ref.K_MAX_LDS, r
    assert (32, 73728, 512) not in fc_ref.CASES                            # the model's shape is test_head.py's
    for c in fc_ref.BORDER_OUTSIDE:
        assert fc_ref.fc_plan(*c) is not None and not fc_ref.backward_served(*c), c


def test_case_table_covers_the_plan_space():
    t = rows()
    has = lambda pred: any(pred(r) for r in t)
    values = lambda f: {getattr(r, f) for r in t}
    assert values("steps") == {16, 32, 64}
    assert values("nw_dx") == {4, 5, 6, 7, 8} and values("nw_dw") == {4, 5, 6, 7, 8}
    assert values("slots_dx") == {256, 512} and values("slots_dw") == {256, 512}
    assert has(lambda r: r.slots_dx == 256 and r.nw_dx > 4) and has(lambda r: r.slots_dw == 256 and r.nw_dw > 4)
    assert has(lambda r: r.kc == 32) and has(lambda r: 32 < r.kc < 480)
    assert has(lambda r: r.kc == 480 and r.K > 480 * 256)
    assert has(lambda r: r.last == 1 and r.chunks > 1) and has(lambda r: r.last % 2 == 1 and r.last > 1)
    assert has(lambda r: r.chunks < 16) and has(lambda r: 17 <= r.chunks <= 64)
    assert has(lambda r: r.chunks > 64 and (r.chunks - 1) % 64 != 63)
    assert has(lambda r: r.chunks != 256 and r.chunks > 64)
    assert values("mblocks") == {1, 2, 3, 4}
    for N in (504, 512, 520):
        assert has(lambda r: r.N == N), N
    assert {r.nblocks for r in t if r.N in (504, 512, 520)} == {1, 2}
    assert {8, 16, 24, 1016, 1024} <= values("N")
    assert has(lambda r: r.N in (8, 16, 24) and r.N // 8 < fc_ref.K_DX_DEPTH)
    for steps in (16, 32, 64):
        assert has(lambda r: r.steps == steps and r.M % 2 == 1 and r.M > 1), steps
    assert {1, 31, 32, 33, 63, 64, 65, 127, 128} <= values("M")
    assert has(lambda r: r.K < 32)
    assert has(lambda r: r.K % 32 != 0 and r.K > 32 * r.nw_dx and r.K > 32 * r.nw_dw)


def finish_wave_sums(chunks, wave):
    """Which chunks fc_finish_kernel's wave adds in its 4-sum loop and in its remainder loop (conv3p_head.hpp:117-124)."""
    c, four, rest = wave, [], []
    while c + 48 < chunks:
        four += [c, c + 16, c + 32, c + 48]
        c += 64
    while c < chunks:
        rest.append(c)
        c += 16
    return four, rest


def test_case_table_runs_the_finish_kernels_loops_together():
    """Some row has a wave with both loops non-empty, some row a wave with only the remainder, and every chunk is added
    exactly once (the restatement of the loop is itself checked here)."""
    both = only_rest = False
    for r in rows():
        seen = []
        for w in range(16):
            four, rest = finish_wave_sums(r.chunks, w)
            seen += four + rest
            both |= bool(four) and bool(rest)
            only_rest |= not four and bool(rest)
        assert sorted(seen) == list(range(r.chunks)), r
    assert both and only_rest


def test_two_roundings_of_the_slope_constant_coincide():
    """float(SCALE * ALPHA) (what selu_slope adds) and float(SCALE) * float(ALPHA) are the same float32: exchanging
    them in the kernel cannot change a bit, so no test can tell them apart."""
    a = np.float32(fc_ref.SELU_SCALE * fc_ref.SELU_ALPHA)
    b = np.float32(fc_ref.SELU_SCALE) * np.float32(fc_ref.SELU_ALPHA)
    assert a.view(np.uint32) == b.view(np.uint32)


def test_workspace_bytes_is_the_mirrors():
    lib = _lib.load()
    Ms = (-1, 0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)
    Ks = (-1, 0, 1, 3, 31, 32, 33, 4160, 8191, 8192, 8193, 8194, 8704, 70000, 122880, 122881, 123001, 200000)
    Ns = (-8, 0, 4, 8, 12, 16, 24, 40, 312, 320, 504, 512, 516, 520, 632, 640, 1016, 1024, 1028, 1032)
    shapes = list(itertools.product(Ms, Ks, Ns)) + fc_ref.CASES + fc_ref.BORDER_INSIDE + fc_ref.BORDER_OUTSIDE
    for M, K, N in shapes:
        got = lib.conv3p_fc_workspace_bytes(M, K, N)
        assert got == fc_ref.workspace_bytes(M, K, N), (M, K, N)
        assert (got == 0) == (fc_ref.fc_plan(M, K, N) is None), (M, K, N)
        if got:
            kc, chunks, mblocks, _ = fc_ref.fc_plan(M, K, N)
            assert got % fc_ref.K_ALIGN == 0 and 0 <= got - max(chunks * mblocks * 32 * N, M * N) * 4 < fc_ref.K_ALIGN


def entry_points(lib):
    """name -> call(M, K, N) with fake pointers and the workspace size the library asks for (at least one line)."""
    def forward(M, K, N):
        return lib.conv3p_fc_forward_f32(FAKE, FAKE, FAKE, M, K, N, 1, FAKE, FAKE,
                                         max(lib.conv3p_fc_workspace_bytes(M, K, N), 256), None)

    def backward(M, K, N):
        return lib.conv3p_fc_backward_f32(FAKE, FAKE, FAKE, FAKE, M, K, N, 1, FAKE, FAKE, FAKE, FAKE,
                                          max(lib.conv3p_fc_workspace_bytes(M, K, N), 256), None)

    def step(M, K, N):
        return lib.conv3p_fc_backward_step_f32(FAKE, FAKE, FAKE, FAKE, FAKE, M, K, N, 1, FAKE, FAKE, FAKE,
                                               ctypes.c_float(0.001), ctypes.c_float(0.9), FAKE,
                                               max(lib.conv3p_fc_workspace_bytes(M, K, N), 256), None)
    return {"forward": forward, "backward": backward, "backward_step": step}


def test_shapes_outside_fc_plan_are_refused_by_all_three_entry_points():
    lib = _lib.load()
    for name, call in entry_points(lib).items():
        for M, K, N in ((32, 64, 12), (32, 64, 516), (1, 64, 4), (32, 64, 1028), (32, 64, 1032), (129, 64, 8), (129, 64, 512)):
            assert fc_ref.fc_plan(M, K, N) is None
            assert call(M, K, N) == _lib.ERR_UNSUPPORTED, (name, M, K, N)


@pytest.mark.parametrize("K", [40, 4096])
def test_backward_refuses_exactly_the_dw_tiles_that_do_not_fit(K):
    """Both sides of the two LDS borders, (M 32 | 33) x (N 632 | 640 | 1024) and (M 64 | 65) x (N 312 | 320), and the
    corners of the two refused regions: where the mirror says the dW tile exceeds 160 KiB both backward entry points
    say UNSUPPORTED (before any launch: the pointers are fake) although the workspace query is non-zero and the
    forward's own checks pass.  The served side of each border needs a device: test_fc_shapes.py runs it."""
    lib = _lib.load()
    calls = entry_points(lib)
    refused = served = 0
    for M, N in itertools.product((1, 32, 33, 64, 65, 128), (8, 312, 320, 632, 640, 1024)):
        want = not fc_ref.backward_served(M, K, N)
        assert want == ((33 <= M <= 64 and N > 632) or (65 <= M <= 128 and N > 312)), (M, N)
        assert lib.conv3p_fc_workspace_bytes(M, K, N) > 0                  # the query does not reflect the two regions
        if not want:
            served += 1
            continue
        refused += 1
        for name in ("backward", "backward_step"):
            assert calls[name](M, K, N) == _lib.ERR_UNSUPPORTED, (name, M, K, N)
    assert refused == 12 and served == 24
    for c in fc_ref.BORDER_OUTSIDE:
        for name in ("backward", "backward_step"):
            assert calls[name](*c) == _lib.ERR_UNSUPPORTED, (name, c)
