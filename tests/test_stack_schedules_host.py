"""The schedule generator of tests/stack_schedule.py on the CPU: deterministic, legal under the contract of
Conv3pStack.prefetch(), and -- over the committed seed list, at every schedule length a mode of
tests/test_stack_schedules.py uses -- reaching every listed situation.  The GPU test runs exactly these schedules."""
import pytest

from tests import stack_schedule as S


def _all_schedules():
    for length in sorted(set(S.MODE_LENGTHS.values())):
        for seed in S.SEEDS:
            yield seed, length, S.generate(seed, length)


def test_generator_is_deterministic():
    for seed, length, (sched, tally) in _all_schedules():
        again, tally2 = S.generate(seed, length)
        assert sched == again and tally == tally2, (seed, length)
        assert len(sched) == length
    assert S.generate(S.SEEDS[0], 36)[0] != S.generate(S.SEEDS[1], 36)[0]


def _check_legal(sched, shapes=S.POOL_SHAPES):
    """The rules restated without the generator's model: tensors as (index, generation), prefetches in order of age."""
    gen = [0] * len(shapes)
    dropped = set()
    out = []                  # outstanding prefetches, oldest first
    held = None               # tensor of the forward that has had no backward yet

    def tensor(i):
        if i in dropped:
            dropped.discard(i)
            gen[i] += 1
        return (i, gen[i])

    for n, op in enumerate(sched):
        kind = op[0]
        assert kind in ("forward", "backward", "prefetch", "tune", "prepare", "rewrite", "drop"), (n, op)
        if kind == "forward":
            t = tensor(op[1])
            if t in out:
                out.remove(t)
            elif len(out) == 2:
                del out[0]
            held = t
        elif kind == "backward":
            assert held is not None, (n, "backward without a forward that has had none")
            assert op[1] in range(S.N_UPSTREAM)
            held = None
        elif kind == "prefetch":
            t = tensor(op[1])
            if t not in out:
                del out[:max(0, len(out) + 1 - (1 if held is not None else 2))]
                out.append(t)
        elif kind == "rewrite":
            assert shapes[op[1]] == shapes[op[2]], (n, "rewrite across shapes")
            t = tensor(op[1])
            assert t not in out, (n, "rewritten between its prefetch and the forward that consumes it")
            assert t != held, (n, "rewritten between its forward and that forward's backward")
        elif kind == "drop":
            dropped.add(op[1])
        elif kind == "prepare":
            assert op[1] in range(S.N_SHAPES)
        assert len(out) <= (1 if held is not None else 2)


def test_every_schedule_is_legal():
    for seed, length, (sched, tally) in _all_schedules():
        _check_legal(sched)
        assert S.replay(sched) == tally, (seed, length)
    for name, sched in S.NAMED.items():
        _check_legal(sched)
        S.replay(sched)


def test_illegal_schedules_are_recognised():
    for bad in ([("backward", 0)],
                [("forward", 0), ("backward", 0), ("backward", 0)],
                [("prefetch", 1), ("rewrite", 1, 2)],
                [("forward", 1), ("rewrite", 1, 2)],
                [("rewrite", 0, 3)]):
        with pytest.raises(S.IllegalSchedule):
            S.replay(bad)
        with pytest.raises(AssertionError):
            _check_legal(bad)
    # superseded, consumed or finished: the tensor is the caller's again
    for good in ([("prefetch", 0), ("prefetch", 1), ("prefetch", 2), ("rewrite", 0, 1)],
                 [("forward", 3), ("prefetch", 0), ("prefetch", 1), ("rewrite", 0, 1)],
                 [("prefetch", 0), ("forward", 0), ("backward", 1), ("rewrite", 0, 2)],
                 [("prefetch", 0), ("prefetch", 1), ("forward", 2), ("rewrite", 0, 1)]):
        S.replay(good)
        _check_legal(good)


@pytest.mark.parametrize("mode", sorted(S.MODE_LENGTHS))
def test_committed_seeds_reach_every_situation(mode):
    total = S.coverage(S.SEEDS, S.MODE_LENGTHS[mode])
    assert set(total) == set(S.SITUATIONS)
    missing = [k for k in S.SITUATIONS if total[k] == 0]
    assert not missing, (mode, missing)
    assert 25 <= S.MODE_LENGTHS[mode] <= 40


def test_named_regression_schedules_are_the_ones_read_from_the_code():
    A, B, C = 0, 1, 2
    assert S.POOL_SHAPES[A] == S.POOL_SHAPES[B] == S.POOL_SHAPES[C]
    f, b, p = (lambda i: ("forward", i)), ("backward", 0), (lambda i: ("prefetch", i))
    assert S.NAMED["prefetch_never_takes_the_cache_of_the_batch_in_flight"] == [f(A), p(B), p(C), b]
    assert S.NAMED["prefetch_never_takes_the_cache_of_a_prefetched_batch_in_flight"] == [p(A), p(B), f(A), p(C), b]
    assert S.NAMED["prefetch_record_is_voided_when_its_cache_goes_to_another_batch"] == [p(A), p(B), f(C), b, f(B)]
    # the first two reach a prefetch between forward and backward that supersedes another; the third a forward that
    # matches neither of two outstanding prefetches, then the forward of the one that survived
    t = S.replay(S.NAMED["prefetch_never_takes_the_cache_of_the_batch_in_flight"])
    assert t["prefetch_between_forward_and_backward"] == 1
    t = S.replay(S.NAMED["prefetch_record_is_voided_when_its_cache_goes_to_another_batch"])
    assert t["two_prefetches_outstanding"] == 1 and t["forward_matches_no_prefetch_while_one_outstanding"] == 1
