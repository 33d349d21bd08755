"""Seeded call schedules for Conv3pStack (pure Python: no torch, no GPU), for tests/test_stack_schedules.py (the runner,
-m gpu) and tests/test_stack_schedules_host.py (determinism, legality, coverage of the committed seeds).

A schedule is a list of operations over a small pool of batches (tensors of points), each a tuple:

    ("forward", i)      forward of pool tensor i
    ("backward", k)     backward of the last forward, with upstream gradient number k (0 or 1) of its shape
    ("prefetch", i)
    ("tune", i)
    ("prepare", s)      prepare(B, N) with shape number s of the pool
    ("rewrite", i, j)   pool batch j's ORIGINAL points copied into tensor i in place (same object, same address, new content)
    ("drop", i)         the caller gives up its reference to tensor i (the stack may still hold it); the tensor is rebuilt
                        from its content -- a NEW object -- when an operation next needs it

Legality is the contract of Conv3pStack.prefetch()'s docstring and nothing more:
  * backward needs a forward that has not had a backward yet;
  * a tensor is not rewritten between its prefetch and the forward that consumes it, unless that prefetch has been
    superseded (see below), nor between the forward it fed and that forward's backward (the backward reads it);
  * everything else is allowed: any number of prefetches at any point, a prefetch of the batch in flight, a forward of a
    batch other than the prefetched one, forwards in a row, prefetches nobody consumes, tune() and prepare() anywhere.

`Model` is the contract's view of which prefetches are outstanding.  The stack has two neighbour caches; the batch between
forward() and backward() keeps one of them, so two prefetches can be outstanding while no batch is in flight and one while
one is.  A prefetch that finds no cache free supersedes the OLDEST outstanding one, and so does a forward that matches no
prefetch while two are outstanding.  Prefetches are matched by the identity of the tensor object: the prefetch of a tensor
the caller has dropped since can never be consumed, it only occupies its cache until it is superseded.

Every schedule comes with a tally of the SITUATIONS it reaches; the committed SEEDS reach every one of them at every
schedule length a mode uses (asserted on the CPU), so the GPU test neither filters nor skips a schedule."""
import random

# (B, N) numbers of the pool tensors: three batches of shape 0 and two of shape 1 -- a change of shape reallocates a cache
# and joins the side stream, batches that share a shape make stale geometry give wrong numbers instead of an error
POOL_SHAPES = (0, 0, 0, 1, 1)
N_SHAPES = 2
N_UPSTREAM = 2

SITUATIONS = (
    "prefetch_between_forward_and_backward",
    "two_prefetches_outstanding",
    "third_prefetch_while_two_outstanding",
    "forward_matches_no_prefetch_while_one_outstanding",
    "forward_matches_older_of_two_prefetches",
    "forward_without_backward_then_prefetch",
    "shape_change_with_prefetch_outstanding",
    "shape_change_right_after_backward",
    "rewrite_of_previous_step_tensor",
    "tune_after_first_step",
    "prepare_after_first_step",
    "forward_after_prefetch_of_dropped_tensor",
)

SEEDS = (2, 3, 5, 8, 13, 20, 21, 34)
# operations per schedule, by mode of tests/test_stack_schedules.py
MODE_LENGTHS = {
    "cls": 36, "seg": 36, "op-by-op": 36, "op-by-op-batched-prefetch": 36, "unfused-selu": 36, "fused-forward": 30,
    "fallback-in16": 36,
}

# The two defects read from the op-by-op path before this file existed, as hand-written schedules (A, B, C = tensors 0, 1, 2,
# which share a shape).  Their names say what they pin.
NAMED = {
    # forward(A); prefetch(B); prefetch(C); backward(A): the second prefetch must not take the cache that serves A
    "prefetch_never_takes_the_cache_of_the_batch_in_flight": [
        ("forward", 0), ("prefetch", 1), ("prefetch", 2), ("backward", 0)],
    # prefetch(A); prefetch(B); forward(A); prefetch(C); backward(A): the same, with A's cache chosen by a prefetch
    "prefetch_never_takes_the_cache_of_a_prefetched_batch_in_flight": [
        ("prefetch", 0), ("prefetch", 1), ("forward", 0), ("prefetch", 2), ("backward", 0)],
    # prefetch(A); prefetch(B); forward(C); backward(C); forward(B): B's prefetch record must not outlive its cache's content
    "prefetch_record_is_voided_when_its_cache_goes_to_another_batch": [
        ("prefetch", 0), ("prefetch", 1), ("forward", 2), ("backward", 0), ("forward", 1)],
}


class IllegalSchedule(Exception):
    pass


class Model:
    """The state the contract defines, advanced one operation at a time; apply() raises IllegalSchedule."""

    def __init__(self, pool_shapes=POOL_SHAPES):
        self.shapes = tuple(pool_shapes)
        n = len(self.shapes)
        self.content = list(range(n))      # content[i]: which batch's original points tensor i holds
        self.gen = [0] * n                 # generation of tensor i: a rebuilt tensor is a new object
        self.alive = [True] * n            # False: dropped by the caller, rebuilt at the next use
        self.outstanding = []              # (i, generation) of the unconsumed prefetches, oldest first
        self.held = False                  # a forward has had no backward yet
        self.last = None                   # (i, generation) of the last forward
        self.last_shape = None
        self.steps = 0                     # forwards so far
        self.after_backward = False        # the previous forward / backward operation was a backward
        self.prefetch_since_forward = False
        self.tally = dict.fromkeys(SITUATIONS, 0)

    def _touch(self, i):
        if not self.alive[i]:
            self.alive[i] = True
            self.gen[i] += 1
        return (i, self.gen[i])

    def rewrite_allowed(self, i):
        key = (i, self.gen[i])
        return key not in self.outstanding and not (self.held and self.last == key)

    def apply(self, op):
        kind, t = op[0], self.tally
        if kind == "forward":
            key = self._touch(op[1])
            shape = self.shapes[op[1]]
            if any(o[0] == key[0] and o != key for o in self.outstanding):
                t["forward_after_prefetch_of_dropped_tensor"] += 1
            if self.held and self.prefetch_since_forward:
                t["forward_without_backward_then_prefetch"] += 1
            if self.last_shape is not None and shape != self.last_shape:
                if self.outstanding:
                    t["shape_change_with_prefetch_outstanding"] += 1
                if self.after_backward:
                    t["shape_change_right_after_backward"] += 1
            if key in self.outstanding:
                if len(self.outstanding) == 2 and self.outstanding[0] == key:
                    t["forward_matches_older_of_two_prefetches"] += 1
                self.outstanding.remove(key)
            else:
                if self.outstanding:
                    t["forward_matches_no_prefetch_while_one_outstanding"] += 1
                if len(self.outstanding) == 2:
                    self.outstanding.pop(0)
            self.held, self.last, self.last_shape = True, key, shape
            self.steps += 1
            self.after_backward = self.prefetch_since_forward = False
        elif kind == "backward":
            if not self.held:
                raise IllegalSchedule("backward without a forward that has had none")
            if not 0 <= op[1] < N_UPSTREAM:
                raise IllegalSchedule("no such upstream gradient")
            if self.prefetch_since_forward:
                t["prefetch_between_forward_and_backward"] += 1
            self.held, self.after_backward = False, True
        elif kind == "prefetch":
            key = self._touch(op[1])
            if key not in self.outstanding:
                if len(self.outstanding) == 2:
                    t["third_prefetch_while_two_outstanding"] += 1
                while len(self.outstanding) >= (1 if self.held else 2):
                    self.outstanding.pop(0)
                self.outstanding.append(key)
                if len(self.outstanding) == 2:
                    t["two_prefetches_outstanding"] += 1
            if self.held:
                self.prefetch_since_forward = True
        elif kind == "tune":
            self._touch(op[1])
            if self.steps:
                t["tune_after_first_step"] += 1
        elif kind == "prepare":
            if not 0 <= op[1] < N_SHAPES:
                raise IllegalSchedule("no such shape")
            if self.steps:
                t["prepare_after_first_step"] += 1
        elif kind == "rewrite":
            i, j = op[1], op[2]
            if self.shapes[i] != self.shapes[j]:
                raise IllegalSchedule("rewrite across shapes")
            self._touch(i)
            if not self.rewrite_allowed(i):
                raise IllegalSchedule("tensor %d rewritten while a prefetch or a backward still needs it" % i)
            if self.last == (i, self.gen[i]):
                t["rewrite_of_previous_step_tensor"] += 1
            self.content[i] = j
        elif kind == "drop":
            self.alive[op[1]] = False
        else:
            raise IllegalSchedule("unknown operation %r" % (kind,))


def replay(schedule, pool_shapes=POOL_SHAPES):
    """The tally of a schedule; raises IllegalSchedule where it breaks the contract."""
    m = Model(pool_shapes)
    for op in schedule:
        m.apply(op)
    return m.tally


_WEIGHTS = (("forward", 30), ("backward", 22), ("prefetch", 30), ("rewrite", 11), ("drop", 6), ("tune", 2), ("prepare", 2))


def generate(seed, length=36, pool_shapes=POOL_SHAPES):
    """(schedule, tally) of `length` operations, a function of the arguments alone."""
    rng = random.Random(seed)
    m = Model(pool_shapes)
    n = len(m.shapes)
    out = []
    while len(out) < length:
        kind = rng.choices([k for k, _ in _WEIGHTS], [w for _, w in _WEIGHTS])[0]
        if kind == "forward":
            # mostly a prefetched batch (either of them), else any batch; now and then twice in a row without a backward
            if m.held and rng.random() < 0.7:
                continue
            live = [o[0] for o in m.outstanding]
            op = ("forward", rng.choice(live) if live and rng.random() < 0.6 else rng.randrange(n))
        elif kind == "backward":
            if not m.held:
                continue
            op = ("backward", rng.randrange(N_UPSTREAM))
        elif kind == "prefetch":
            op = ("prefetch", rng.randrange(n))
        elif kind == "rewrite":
            # mostly the tensor of the previous step; only tensors the contract lets the caller write
            i = m.last[0] if m.last is not None and rng.random() < 0.6 else rng.randrange(n)
            if not m.alive[i] or not m.rewrite_allowed(i):
                continue
            op = ("rewrite", i, rng.choice([j for j in range(n) if m.shapes[j] == m.shapes[i]]))
        elif kind == "drop":
            # mostly a tensor whose prefetch is outstanding: the stack's reference is then the only one left
            live = [o[0] for o in m.outstanding if m.alive[o[0]] and o[1] == m.gen[o[0]]]
            i = rng.choice(live) if live and rng.random() < 0.7 else rng.randrange(n)
            if not m.alive[i] or (m.held and m.last == (i, m.gen[i])):
                continue            # (the tensor in flight stays: the runner keeps it for the backward's reference anyway)
            op = ("drop", i)
        elif kind == "tune":
            op = ("tune", rng.randrange(n))
        else:
            op = ("prepare", rng.randrange(N_SHAPES))
        m.apply(op)
        out.append(op)
    return out, dict(m.tally)


def coverage(seeds=SEEDS, length=36, pool_shapes=POOL_SHAPES):
    """Situation -> how often the schedules of `seeds` reach it."""
    total = dict.fromkeys(SITUATIONS, 0)
    for s in seeds:
        for k, v in generate(s, length, pool_shapes)[1].items():
            total[k] += v
    return total
