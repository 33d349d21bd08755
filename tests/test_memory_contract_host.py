"""The memory contract's rig and tables, on the host (no device): tests/memory_rig.py finds every caller-owned region of
include/conv3p.h, every such function has a case in tests/stream_contract_cases.py, the sentences KEEPS_STATE quotes are the
header's, and the arena -- alignment, guard widths, intact() -- sees the three planted violations on CPU tensors and
passes the well-behaved plant."""
import re

import pytest
import torch

from tests import memory_rig as rig, stream_contract_cases as table
from tests.test_memory_contract import NO_REGION_THIS_CALL, NOT_REACHED, ROUTE_BY_SIZE

REGIONS = rig.regions()
HEADER_TEXT = open(rig.HEADER).read()


def test_the_finder_names_every_function_with_a_region_once():
    text = re.sub(r"/\*.*?\*/", " ", HEADER_TEXT, flags=re.S)
    # independently of the finder's parameter split: every `void *X, size_t X_bytes` of the header, and the function
    # whose parameter list it closes in
    names = []
    for m in re.finditer(r"void\s*\*\s*(workspace|scratch|cache)\s*,\s*size_t\s+\1_bytes\b", text):
        names.append((re.findall(r"\b(conv3p_\w+)\s*\(", text[:m.start()])[-1], m.group(1)))
    assert len(names) == len(set(names)), "a function is declared twice"
    assert sorted(names) == sorted((f, r) for f, pairs in REGIONS.items() for r, _, _ in pairs)
    assert len(REGIONS) > 50 and REGIONS["conv3p_stack_backward_f32"] == [("scratch", 13, 14), ("cache", 15, 16)]
    for f, pairs in REGIONS.items():
        for region, p, b in pairs:
            assert b == p + 1 and region in rig.REGION_NAMES, (f, region)


def test_the_positions_agree_with_the_ctypes_signatures():
    import ctypes
    from pointwise_amd import _lib
    for f, pairs in REGIONS.items():
        argtypes = _lib.SYMBOLS[f][1]
        for region, p, b in pairs:
            assert argtypes[p] is ctypes.c_void_p and argtypes[b] is ctypes.c_size_t, (f, region)
        for p in rig.output_positions()[f]:
            assert argtypes[p] is ctypes.c_void_p, (f, p)


def test_every_function_with_a_region_has_a_case_or_a_reason():
    reached = set().union(*[e.reaches for e in table.ENTRIES])
    for f in REGIONS:
        assert (f in reached) != (f in NOT_REACHED), "%s needs a case in stream_contract_cases.ENTRIES or a reason" % f
    assert set(NOT_REACHED) <= set(REGIONS)
    assert all(isinstance(r, str) and r for r in NOT_REACHED.values())


def test_keeps_state_quotes_the_header():
    for f, per in rig.KEEPS_STATE.items():
        assert f in REGIONS, f
        for region, sentence in per.items():
            assert region in [r for r, _, _ in REGIONS[f]], (f, region)
            assert sentence in HEADER_TEXT, "quote the header verbatim: %r" % sentence
    # every `cache` is classified, and nothing else is: the other regions are per-call
    for f, pairs in REGIONS.items():
        assert {r for r, _, _ in pairs if r == "cache"} == set(rig.KEEPS_STATE.get(f, {})), f
    assert set(rig.NO_DECLARED_SIZE) <= set(REGIONS)


def test_the_other_tables_quote_the_header():
    flat = rig.flat_header()
    for f, (status, sentence) in rig.REFUSES_WITH.items():
        assert f in REGIONS and f not in rig.KEEPS_STATE and status != rig.ERR_WORKSPACE, f
        assert sentence in flat, (f, sentence)
    reaches = {e.name: e.reaches for e in table.ENTRIES}
    for (case, f), sentence in NO_REGION_THIS_CALL.items():
        assert f in reaches[case] and f in REGIONS, (case, f)
        assert sentence in flat, (case, sentence)


def test_route_by_size_cites_a_source_line():
    import os
    csrc = os.path.join(os.path.dirname(rig.HEADER), os.pardir, "pointwise_amd", "csrc")
    names = [e.name for e in table.ENTRIES]
    for case, (source, line) in ROUTE_BY_SIZE.items():
        assert case in names, case
        assert re.fullmatch(r"conv3p_abi_\w+\.hpp", source), source
        assert line.strip() in open(os.path.join(csrc, source)).read(), (case, line)


@pytest.mark.parametrize("nbytes", [1, 255, 256, 1000, (64 << 10) - 1, (64 << 10) + 1, 100000, (16 << 20) + 5])
def test_arena_layout(nbytes):
    a = rig.Arena(nbytes, "cpu")
    assert a.body.numel() == nbytes and a.low.numel() == a.high.numel() == a.guard
    assert a.base % 256 == 0 and a.body.data_ptr() % 256 == 0
    assert a.body.data_ptr() == a.base + a.guard and a.high.data_ptr() == a.body.data_ptr() + nbytes
    assert a.guard >= min(max(nbytes, 64 << 10), 16 << 20) and a.guard <= (16 << 20)
    assert a.guard >= nbytes or a.guard == (16 << 20)
    # everything lies inside the one allocation
    lo, hi = a.raw.data_ptr(), a.raw.data_ptr() + a.raw.numel()
    assert lo <= a.base and a.high.data_ptr() + a.guard <= hi
    i = torch.arange(a.guard)
    assert torch.equal(a.low, ((131 * i + 7) & 0xFF).to(torch.uint8)) and torch.equal(a.high, a.low)
    assert a.low.unique().numel() == 256                 # position-dependent: no constant fill reproduces it
    assert a.intact() is None


def test_intact_reports_first_and_last_changed_offset():
    a = rig.Arena(1000, "cpu")
    a.body.fill_(0xFF)
    assert a.intact() is None                            # the body is the call's
    a.high[0] ^= 0xFF
    assert a.intact() == (1000, 1000)
    a.high[300] ^= 1
    assert a.intact() == (1000, 1300)
    a.low[-1] ^= 0xFF
    a.low[0] ^= 0xFF
    assert a.intact() == (-a.guard, 1300)
    a.mend()
    assert a.intact() is None
    a.high[:512] = 0                                     # a memset-style overrun: a constant is not the pattern
    first, last = a.intact()
    assert first >= 1000 and last <= 1000 + 511 and last - first > 500


@pytest.fixture(scope="module")
def plants():
    return rig.judge_plants("cpu")


def test_plant_write_past(plants):
    v = plants["write_past"]
    assert rig.all_changed(v) == {(rig.PLANT_BYTES, rig.PLANT_BYTES)} and all(v.changed.values()), v.changed
    assert not rig.any_dirty(v)


def test_plant_write_before(plants):
    v = plants["write_before"]
    assert rig.all_changed(v) == {(-1, -1)} and all(v.changed.values()), v.changed
    assert not rig.any_dirty(v)


def test_plant_reads_stale(plants):
    v = plants["reads_stale"]
    assert v.dirty["0xFF"] == [0] and v.dirty["leftover"] == [0] and not rig.all_changed(v), v.dirty


def test_plant_well_behaved(plants):
    v = plants["well_behaved"]
    assert not rig.all_changed(v) and not rig.any_dirty(v), (v.changed, v.dirty)
    assert list(v.sizes.values()) == [rig.PLANT_BYTES]


def test_the_output_finder_takes_the_largest_tensor_at_an_address():
    dev = torch.device("cpu")
    whole = torch.zeros(64)
    head, tail, strided = whole[:8], whole[8:], whole[::2]
    found = {}
    rig._note_tensors(found, [head, strided, "no tensor", whole, tail, torch.zeros(0)], dev)
    assert found[whole.data_ptr()] is whole and found[tail.data_ptr()] is tail and len(found) == 2
    assert rig._as_bytes(torch.zeros((), dtype=torch.float64)).numel() == 8      # a 0-dim output has bytes too


def test_the_dirty_fills_differ():
    """0x00 is the clean fill; the dirty ones -- 0xFF and what a run on the other half's inputs left -- differ from it
    and from each other."""
    assert list(rig.FILLS.values()) == [0x00, 0xFF] and rig.SENTINEL not in rig.FILLS.values()
    case, regs = rig.plant_well_behaved("cpu")
    rig.judge(case, regs, "cpu")
    (arena,) = regs.arenas.values()
    leftover = arena.body.clone()
    zeros, ones = torch.zeros_like(leftover), torch.full_like(leftover, 0xFF)
    assert not torch.equal(leftover, zeros) and not torch.equal(leftover, ones) and not torch.equal(ones, zeros)
    # the leftover is that of a run on OTHER inputs: the poison half differs from the real one
    for e in table.ENTRIES[:3]:
        real, poison = e.halves()
        assert any((r != p).any() for r, p in zip(real, poison))
