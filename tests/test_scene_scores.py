"""Votes by summed class probabilities on the device (-m gpu): conv3p_scene_vote_scores_f32 against a float64 softmax sum
(tests/scene_cover_ref.py) within votes_i * (32 * 2^-24 + 2^-31) per room row -- the float32 softmax bound
tests/test_seg_head.py holds the same expf to, plus the rounding to fixed point -- its exactness under permutation and
splitting of the rows compared for equality, and conv3p_scene_score_labels compared for equality with the integer argmax."""
import numpy as np
import pytest

from tests import scene_cover_ref as cref

ROWS = (1, 63, 64, 65, 1000)
CLASSES = (1, 2, 13, 41, 128)
N = 37                                         # room rows: few, so that many block rows vote for each


@pytest.fixture(scope="module")
def dev():
    import torch
    from pointwise_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


def make_case(rows, C):
    """Logits spanning +-80 with rows of equal logits and rows with NaN / +-Inf; indices with -1, past the end, and a
    run of rows all voting for room row 5."""
    rng = np.random.default_rng(1000 * rows + C)
    x = (rng.uniform(-80, 80, size=(rows, C)) * rng.choice([1.0, 0.1, 0.01], size=(rows, 1))).astype(np.float32)
    x[rng.random(rows) < 0.1] = np.float32(rng.uniform(-80, 80))             # equal logits
    index = rng.integers(-1, N + 2, size=rows).astype(np.int32)
    index[rows // 3:rows // 3 + rows // 4] = 5
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for r in range(7 + k, rows, 29):
            x[r, (r * 7) % C] = bad
    if rows > 40:
        index[7], index[8], index[36] = 3, -1, N                            # a refused row, and bad rows that are not counted
    return x, index


def add(dev, sc, x, index):
    import torch
    sc.add(torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(index)).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("rows", ROWS)
def test_scores_against_float64_and_exactness(dev, rows, C):
    from pointwise_amd import scene
    x, index = make_case(rows, C)
    ok, refused = cref.voters(x, index, N)
    want, votes = cref.scores_ref64(x, index, N)
    sc = scene.SceneScores(N, C, dev)
    add(dev, sc, x, index)
    got = sc.scores.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (N, C)
    err = np.abs(got / float(cref.SCALE) - want).max(axis=1)
    print("rows=%d C=%d  max |scores / 2^30 - ref| / votes %.3e (bound %.3e)" % (
        rows, C, (err / np.maximum(votes, 1)).max(), cref.SCORE_TOL))
    assert np.all(err <= votes * cref.SCORE_TOL)                            # rows without votes: exactly 0
    assert sc.vote_stats.tolist() == [int(ok.sum()), int(refused.sum())]
    if rows > 40:
        assert int(refused.sum()) > 0 and int((~ok).sum()) > int(refused.sum())   # refused rows, and rows that do not count
    # the same rows permuted, and in two calls: bit-equal
    perm = np.random.default_rng(rows + C).permutation(rows)
    sp = scene.SceneScores(N, C, dev)
    add(dev, sp, x[perm], index[perm])
    assert np.array_equal(sp.scores.cpu().numpy(), got) and sp.vote_stats.tolist() == sc.vote_stats.tolist()
    if rows > 1:
        s2 = scene.SceneScores(N, C, dev)
        add(dev, s2, x[:rows // 2], index[:rows // 2])
        add(dev, s2, x[rows // 2:].reshape(1, rows - rows // 2, C), index[rows // 2:].reshape(1, -1))   # any leading shape
        assert np.array_equal(s2.scores.cpu().numpy(), got) and s2.vote_stats.tolist() == sc.vote_stats.tolist()
    # labels: exactly the integer argmax of the device's own scores
    lab, st = cref.score_labels_ref(got)
    assert np.array_equal(sc.labels().cpu().numpy(), lab) and sc.counts().tolist() == st.tolist()
    assert np.array_equal(lab >= 0, votes > 0)
    sc.reset()
    assert not sc.scores.any() and sc.vote_stats.tolist() == [0, 0]
    assert sc.counts().tolist() == [0, N] and np.all(sc.labels().cpu().numpy() == -1)


@pytest.mark.gpu
def test_refused_rows_leave_the_scores_untouched(dev):
    from pointwise_amd import scene
    x, index = make_case(1000, 13)
    ok, refused = cref.voters(x, index, N)
    assert refused.sum() >= 50
    sc, only = scene.SceneScores(N, 13, dev), scene.SceneScores(N, 13, dev)
    add(dev, sc, x, index)
    add(dev, only, x[ok], index[ok])                                        # the voting rows alone
    assert np.array_equal(sc.scores.cpu().numpy(), only.scores.cpu().numpy())
    assert only.vote_stats.tolist() == [int(ok.sum()), 0]
    bad = scene.SceneScores(N, 13, dev)
    add(dev, bad, x[refused], index[refused])                               # the refused rows alone
    assert not bad.scores.any() and bad.vote_stats.tolist() == [0, int(refused.sum())]
    assert bad.counts().tolist() == [0, N]


@pytest.mark.gpu
def test_all_rows_for_one_room_row_and_equal_logits(dev):
    from pointwise_amd import scene
    C, rows = 13, 1000
    x = np.full((rows, C), 3.25, np.float32)
    index = np.full(rows, 2, np.int32)
    sc = scene.SceneScores(4, C, dev)
    add(dev, sc, x, index)
    got = sc.scores.cpu().numpy()
    each = int(np.rint(np.float32(np.float32(1) / np.float32(13)) * np.float32(2.0 ** 30)))
    assert got[2].tolist() == [rows * each] * C and not got[[0, 1, 3]].any()   # exp(0) = 1 exactly: the bits are known
    assert sc.labels().tolist() == [-1, -1, 0, -1] and sc.counts().tolist() == [1, 3]   # a tie: the lowest class
    one = scene.SceneScores(4, 1, dev)
    add(dev, one, np.array([[-80.0], [80.0], [0.0]], np.float32), np.array([1, 1, 3], np.int32))
    assert one.scores.cpu().numpy().reshape(-1).tolist() == [0, 2 << 30, 0, 1 << 30]
    assert one.labels().tolist() == [-1, 0, -1, 0]


@pytest.mark.gpu
def test_labels_on_hand_written_scores(dev):
    import torch
    from pointwise_amd import scene
    rows = [[0, 0, 0, 0], [5, 9, 9, 1], [3, 3, 3, 3], [0, 0, 0, 1], [1 << 62, 0, (1 << 62) + 1, 0], [0, 7, 0, 7],
            [(1 << 40) + 1, 1 << 40, 0, 0]]
    sc = scene.SceneScores(len(rows), 4, dev)
    sc.scores.copy_(torch.tensor(rows, dtype=torch.int64))
    assert sc.labels().tolist() == [-1, 1, 0, 3, 2, 1, 0] and sc.counts().tolist() == [6, 1]
    assert np.array_equal(cref.score_labels_naive(np.array(rows, np.int64)), sc.labels().cpu().numpy())
    one = scene.SceneScores(3, 1, dev)
    one.scores.copy_(torch.tensor([[4], [0], [1]], dtype=torch.int64))
    assert one.labels().tolist() == [0, -1, 0] and one.counts().tolist() == [2, 1]
    big = np.random.default_rng(9).integers(0, 1 << 50, size=(5000, 41))
    big[np.random.default_rng(10).random(big.shape) < 0.6] = 0
    big[::7] = 0
    sc = scene.SceneScores(5000, 41, dev)
    sc.scores.copy_(torch.from_numpy(big))
    lab, st = cref.score_labels_ref(big)
    assert np.array_equal(sc.labels().cpu().numpy(), lab) and sc.counts().tolist() == st.tolist() and st[1] >= 700


@pytest.mark.gpu
def test_add_checks_its_arguments(dev):
    import torch
    from pointwise_amd import scene
    from pointwise_amd.conv3p_op import Conv3pInvalidArgument
    sc = scene.SceneScores(10, 13, dev)
    x, i = torch.zeros((4, 13), device=dev), torch.zeros((4,), dtype=torch.int32, device=dev)
    for a, b in ((x.double(), i), (x, i.long()), (x[:, :12], i), (x, i[:3]), (x.cpu(), i), (x, i.cpu()),
                 (torch.zeros((4, 26), device=dev)[:, ::2], i), (x.numpy(force=True), i)):
        with pytest.raises(Conv3pInvalidArgument):
            sc.add(a, b)
    assert not sc.scores.any() and sc.vote_stats.tolist() == [0, 0]
    sc.add(x[:0], i[:0])                                                     # nothing to do
    assert sc.vote_stats.tolist() == [0, 0]
