"""The stream contract of include/conv3p_match.h's entry point: ordered on the caller's stream, no host synchronisation
(DESIGN.md section 4), on the rig of tests/stream_rig.py with the cases of tests/stream_contract_match_cases.py.  The host
half (no GPU): the streamed declaration of the header has a case, the cases reach symbols of _lib.MATCH_SYMBOLS, and the
poison matches its input.  The device half (-m gpu): the rig must see a planted violation first; then every case is
ordered, asynchronous and deterministic, and -- by recording shims around the streamed functions of all four headers --
enters exactly c3p_grid_match_segments."""
import pytest
import torch

from pointwise_amd import _lib
from tests import stream_contract_cases as main_table, stream_contract_graph_cases as graph_table
from tests import stream_contract_knn_cases as knn_table, stream_contract_match_cases as table, stream_rig


# ---------------------------------------------------------------------------------------------------------- the host half
def test_the_streamed_function_of_the_match_header_has_a_case():
    streamed = table.streamed_functions()
    assert streamed == set(_lib.MATCH_SYMBOLS) - {"c3p_grid_match_scratch_bytes"} == {"c3p_grid_match_segments"}
    others = main_table.streamed_functions() | graph_table.streamed_functions() | knn_table.streamed_functions()
    assert not streamed & others and not main_table.streamed_functions(table.HEADER)     # nothing under the conv3p_ prefix
    assert not set(_lib.MATCH_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS) | set(_lib.KNN_SYMBOLS))
    assert set().union(*(e.reaches for e in table.ENTRIES)) == streamed
    assert len(set(table.NAMES)) == len(table.NAMES)
    assert not set(table.NAMES) & (set(main_table.NAMES) | set(graph_table.NAMES) | set(knn_table.NAMES))
    for other in (main_table, graph_table, knn_table):   # the other tables are left as they are
        assert all(e not in other.ENTRIES for e in table.ENTRIES)


def test_poison_matches_its_input_in_shape_and_dtype():
    for e in table.ENTRIES:
        real, poison = e.halves()
        assert len(real) == len(poison) and real, e.name
        for i, (r, p) in enumerate(zip(real, poison)):
            assert r.shape == p.shape and r.dtype == p.dtype, (e.name, i)
            assert r.size == 0 or not (r == p).all(), (e.name, i, "the poison equals the input")


# -------------------------------------------------------------------------------------------------------- the device half
@pytest.fixture(scope="module")
def rig():
    """(device, the stream the cases run on); fails if no stream sees the wrong-stream plant."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    dev = torch.device("cuda:0")
    stream, tries, plants = stream_rig.find_stream(dev)
    assert stream is not None, ("an op on the default stream was not seen from any of %d fresh side streams (%r)" % (tries, plants))
    assert plants["item"].asynchronous is False and plants["well_behaved"].asynchronous is True, plants
    return dev, stream


class Shims:
    """Recording shims around the streamed functions of the four headers on the object _lib.load() returns."""

    def __init__(self):
        self.lib, self.seen, self.active, self.originals = _lib.load(), set(), False, {}

    def __enter__(self):
        for name in sorted(main_table.streamed_functions() | graph_table.streamed_functions() | knn_table.streamed_functions()
                           | table.streamed_functions()):
            self.originals[name] = fn = getattr(self.lib, name)
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", table.NAMES)
def test_stream_contract(rig, name):
    dev, stream = rig
    e = table.ENTRIES[table.NAMES.index(name)]
    real, poison = e.halves()
    with Shims() as shims:
        v = stream_rig.judge(shims.around(e.build(dev, real, poison)), stream)
    print("%s: t_host %.3f ms, delay %.1f ms, ordered %s, asynchronous %s" % (name, v.t_host_ms, v.delay_ms, v.ordered, v.asynchronous))
    assert v.ordered is not None, v.diagnostic
    assert v.deterministic, "two runs on the idle device differ: the case is not fit for a bitwise comparison"
    assert v.ordered, "outputs %s differ from the idle run's: work left the caller's stream" % v.mismatched
    assert v.asynchronous, "the call waited for the device before it returned\n" + v.diagnostic
    assert shims.seen == set(e.reaches) == {"c3p_grid_match_segments"}, (sorted(shims.seen), sorted(e.reaches))
