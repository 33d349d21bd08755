"""The stream contract of every entry point (-m gpu): ordered on the caller's stream, no host synchronisation
(include/conv3p.h).  tests/stream_rig.py measures both facts for one call; the calls are the table of
tests/stream_contract_cases.py.

First the rig proves that it can see: planted violations written in plain torch must come out as violations.  The
contract tests depend on the same module-scoped fixture, so they fail with it instead of passing blind.  Then one test
per case: ordered for every case, asynchronous for every case outside HOST_BY_CONTRACT, and -- through recording shims
around the functions of the loaded library, for the duration of the case's run() calls -- exactly the streamed C entry
points the case claims to reach."""
import pytest
import torch

from tests import stream_contract_cases as table, stream_rig

pytestmark = pytest.mark.gpu

STREAMED = sorted(table.streamed_functions())


@pytest.fixture(scope="module")
def rig():
    """(device, the stream the cases run on, the verdicts of the plants on it); fails if no stream sees the plant."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from pointwise_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    stream, tries, plants = stream_rig.find_stream(dev)
    assert stream is not None, ("an op on the default stream was not seen from any of %d fresh side streams: they may share "
                                "a hardware queue with it; nothing below would prove anything (%r)" % (tries, plants))
    print("stream contract: torch stream try %d of 4 (handle %#x) sees the wrong-stream plant" % (tries, stream.cuda_stream))
    return dev, stream, plants


def test_the_rig_sees_a_read_on_the_default_stream(rig):
    v = rig[2]["wrong_stream"]
    assert v.deterministic and v.ordered is False, v


def test_the_rig_sees_an_item(rig):
    v = rig[2]["item"]
    assert v.asynchronous is False, v
    assert v.ordered is True, v
    assert "synchroniz" in v.diagnostic, v               # the debug mode's traceback is kept as the diagnostic


def test_the_rig_sees_a_pageable_upload(rig):
    v = rig[2]["pageable_upload"]
    assert v.asynchronous is False and v.ordered is True, v


def test_the_rig_passes_a_well_behaved_op(rig):
    v = rig[2]["well_behaved"]
    assert v.deterministic and v.ordered is True and v.asynchronous is True and not v.diagnostic, v


class Shims:
    """Recording shims around the streamed functions of the object _lib.load() returns: each notes its name while a
    case's run() is on the stack, and passes through."""

    def __init__(self):
        from pointwise_amd import _lib
        self.lib = _lib.load()
        self.seen = set()
        self.active = False
        self.originals = {}

    def __enter__(self):
        for name in STREAMED:
            fn = getattr(self.lib, name)
            self.originals[name] = fn
            setattr(self.lib, name, self._shim(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.originals.items():
            setattr(self.lib, name, fn)

    def _shim(self, name, fn):
        def call(*args):
            if self.active:
                self.seen.add(name)
            return fn(*args)
        return call

    def around(self, case):
        def run():
            self.active = True
            try:
                return case.run()
            finally:
                self.active = False
        return case._replace(run=run)


@pytest.mark.parametrize("name", table.NAMES)
def test_stream_contract(rig, name):
    dev, stream, _ = rig
    e = table.ENTRIES[table.NAMES.index(name)]
    real, poison = e.halves()
    with Shims() as shims:
        v = stream_rig.judge(shims.around(e.build(dev, real, poison)), stream)
    print("%s: t_host %.3f ms, delay %.1f ms, ordered %s, asynchronous %s" % (name, v.t_host_ms, v.delay_ms, v.ordered, v.asynchronous))
    assert v.ordered is not None, v.diagnostic
    assert v.deterministic, "two runs on the idle device differ: the case is not fit for a bitwise comparison"
    assert v.ordered, "outputs %s differ from the idle run's: work left the caller's stream" % v.mismatched
    if name not in table.HOST_BY_CONTRACT:
        assert v.asynchronous, "the call waited for the device before it returned\n" + v.diagnostic
    assert shims.seen == set(e.reaches), (sorted(shims.seen), sorted(e.reaches))
