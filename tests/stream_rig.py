"""The stream-contract rig: does a call stay on the caller's stream, and does it return without waiting for the device?

include/conv3p.h promises "no host synchronisation ... every call is ordered on `stream`".  judge(case, stream) measures
both halves of that sentence for one call ("The stream contract"):

  ordered        everything the call enqueued ran after what the caller had enqueued before it on the current stream and
                 before what the caller enqueued behind it.  The inputs hold POISON (other valid values) in memory; the
                 real values are copied in on the stream, behind a delay kernel; the outputs are read back on the stream.
                 Work that left the stream without an event joining it back reads the poison, or writes after the
                 read-back: the outputs then differ, bit for bit, from those of a run on the idle device.
  asynchronous   the call returned while the delay kernel was still running (an event recorded on the stream just before
                 the call has not completed when the call returns): the host cannot have waited for, or read, anything
                 on the device.

The rig runs on a NON-default torch stream: those are non-blocking streams, which the legacy NULL stream does not wait
for, so work that strays to the NULL stream overtakes the delay.  On the default stream nothing could be detected.

A case is a Case(inputs, poison, run, reset):
  inputs   the device tensors the call reads;
  poison   per input another VALID tensor of the same shape and dtype (another seed of the same generator; another
           in-range tensor for labels and indices; never a NaN, never an index out of range): a kernel that runs early
           computes a wrong answer and never forms a bad address.  The rig cannot provoke a fault;
  run()    performs the call and returns the list of its output tensors;
  reset()  restores whatever the call mutates, so that two runs start equal.

The delay is per case: max(50 ms, 20 x the host time of the call on the idle device), from `_sleep` cycles calibrated
against events once per process.  A blocked host would wait out the whole remaining delay anyway; the factor only keeps a
slow enqueue from being mistaken for a wait.  A case that would need more than a second is reported as "enqueue too slow
to judge".  The delay kernel is bounded and ends by itself; nothing here waits on a condition.
"""
import collections
import time
import traceback
import warnings

import torch

Case = collections.namedtuple("Case", "inputs poison run reset")
Case.__new__.__defaults__ = (lambda: None,)

MIN_DELAY_MS = 50.0
HOST_FACTOR = 20.0
MAX_DELAY_MS = 1000.0

Verdict = collections.namedtuple("Verdict", "ordered asynchronous deterministic t_host_ms delay_ms mismatched diagnostic")

_CYCLES_PER_MS = {}


def cycles_per_ms(dev):
    """`torch.cuda._sleep` cycles per millisecond on `dev`, measured once per process with events around a sleep."""
    key = torch.device(dev).index or 0
    if key not in _CYCLES_PER_MS:
        with torch.cuda.device(dev):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(1 << 16)                   # (the kernel's code object)
            rate = None
            for cycles in (1 << 20, 1 << 24):            # the second, longer one is the measurement if the first is short
                torch.cuda.synchronize()
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                rate = cycles / max(a.elapsed_time(b), 1e-3)
                if a.elapsed_time(b) >= 5.0:
                    break
        _CYCLES_PER_MS[key] = rate
    return _CYCLES_PER_MS[key]


def _bits(t):
    """A host tensor as integers: floats are compared as int32 / int64 views, so a NaN equals itself and -0.0 is not 0.0."""
    t = t.contiguous()
    if t.dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])
    return t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check_case(case):
    assert len(case.inputs) == len(case.poison) and case.inputs, "a case needs inputs, and a poison per input"
    for i, (x, p) in enumerate(zip(case.inputs, case.poison)):
        assert x.is_cuda and p.is_cuda and x.shape == p.shape and x.dtype == p.dtype, "input %d and its poison differ" % i
        assert x.data_ptr() != p.data_ptr() or x.numel() == 0, "input %d is its own poison" % i


def _outputs(res):
    outs = list(res) if isinstance(res, (list, tuple)) else [res]
    assert outs and all(isinstance(t, torch.Tensor) for t in outs), "run() returns the list of its output tensors"
    return outs


def _idle_run(case, s):
    """reset(), run() on the idle device -> (host copies of the outputs, host wall time of run() in ms)."""
    case.reset()
    s.synchronize()
    t0 = time.perf_counter()
    outs = _outputs(case.run())
    t_host = (time.perf_counter() - t0) * 1e3
    s.synchronize()
    return [t.detach().cpu() for t in outs], t_host


def _measured_run(case, s, real, pinned, cycles, mode):
    """Step 2 of the module docstring -> (host copies of the outputs, returned_early, the sync warnings / error text)."""
    case.reset()
    for x, p in zip(case.inputs, case.poison):
        x.copy_(p)
    torch.cuda.synchronize()
    notes, early = [], None
    torch.cuda._sleep(cycles)
    for x, r in zip(case.inputs, real):
        x.copy_(r)                                       # device to device: asynchronous, on the stream
    marker = torch.cuda.Event()
    marker.record(s)
    before = torch.cuda.get_sync_debug_mode()
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode(mode)
            try:
                outs = _outputs(case.run())
            finally:
                torch.cuda.set_sync_debug_mode(before)
            early = not marker.query()
        notes = ["%s:%d: %s" % (w.filename, w.lineno, w.message) for w in caught if "synchroniz" in str(w.message)]
        for t, h in zip(outs, pinned):
            h.copy_(t.detach(), non_blocking=True)
    finally:
        s.synchronize()
    return [h.clone() for h in pinned], early, notes


def judge(case, s):
    """The verdict on one case, everything on the non-default stream `s`."""
    assert s != torch.cuda.default_stream(s.device), "the rig needs a non-default stream"
    _check_case(case)
    dev = s.device
    with torch.cuda.device(dev), torch.cuda.stream(s):
        real = [x.clone() for x in case.inputs]          # device-resident staging
        _idle_run(case, s)                               # pays every one-off cost
        expected, t_host = _idle_run(case, s)
        again, t2 = _idle_run(case, s)
        t_host = min(t_host, t2)
        deterministic = len(expected) == len(again) and all(_same(a, b) for a, b in zip(expected, again))
        delay = max(MIN_DELAY_MS, HOST_FACTOR * t_host)
        if delay > MAX_DELAY_MS:
            return Verdict(None, None, deterministic, t_host, delay, [], "enqueue too slow to judge: %.1f ms on the host" % t_host)
        cycles = int(delay * cycles_per_ms(dev))
        pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in expected]
        diagnostic = ""
        try:
            got, early, notes = _measured_run(case, s, real, pinned, cycles, "error")
        except RuntimeError as e:
            if "synchroniz" not in str(e):
                raise
            # the debug mode's traceback says where torch synchronised; the marker of a second run, under "warn", is
            # the criterion
            diagnostic = traceback.format_exc()
            torch.cuda.synchronize()
            got, early, notes = _measured_run(case, s, real, pinned, cycles, "warn")
        if notes and not diagnostic:
            diagnostic = "\n".join(notes)
        for x, r in zip(case.inputs, real):
            x.copy_(r)
        s.synchronize()
        mismatched = [i for i, (a, b) in enumerate(zip(expected, got)) if not _same(a, b)]
        if len(expected) != len(got):
            mismatched.append(-1)
    return Verdict(not mismatched, bool(early), deterministic, t_host, delay, mismatched, diagnostic)


# ------------------------------------------------------------------------------------------------ the rig sees: plants
def _plant(dev, thunk_of):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4096, generator=g).to(dev)
    p = torch.randn(4096, generator=g).to(dev)
    return Case([x], [p], thunk_of(x))


def plant_wrong_stream(dev):
    """A torch op that reads its input on the DEFAULT stream, whatever the current one is."""
    def thunk(x):
        def run():
            with torch.cuda.stream(torch.cuda.default_stream(dev)):
                return [x * 2.0]
        return run
    return _plant(dev, thunk)


def plant_item(dev):
    """A thunk that reads a device value on the host."""
    def thunk(x):
        def run():
            y = x * 2.0
            y.sum().item()
            return [y]
        return run
    return _plant(dev, thunk)


def plant_pageable_upload(dev):
    """A thunk that uploads a pageable host tensor in the middle of the call."""
    host = torch.arange(4096, dtype=torch.float32)

    def thunk(x):
        return lambda: [x * 2.0 + host.to(dev)]
    return _plant(dev, thunk)


def plant_well_behaved(dev):
    return _plant(dev, lambda x: (lambda: [x * 2.0 + 1.0]))


def find_stream(dev, tries=4):
    """A non-default stream on which the wrong-stream plant is detected, and the verdicts of every plant on it:
    (stream, tries used, {plant: Verdict}).  A side stream that shares a hardware queue with the default stream cannot
    show an op that strays there, so up to `tries` fresh streams are tried; (None, tries, last verdicts) if none sees."""
    verdicts = {}
    for n in range(1, tries + 1):
        s = torch.cuda.Stream(device=dev)
        verdicts = {"wrong_stream": judge(plant_wrong_stream(dev), s)}
        if verdicts["wrong_stream"].ordered is False:
            verdicts["item"] = judge(plant_item(dev), s)
            verdicts["pageable_upload"] = judge(plant_pageable_upload(dev), s)
            verdicts["well_behaved"] = judge(plant_well_behaved(dev), s)
            return s, n, verdicts
    return None, tries, verdicts
