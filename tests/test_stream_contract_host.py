"""The table of tests/stream_contract_cases.py covers what it must (no GPU): every function of include/conv3p.h with a
stream parameter, every public name of the package, and poison that matches its input.  A new C entry point or public
function without a case fails here."""
import inspect
import re

import pointwise_amd
from pointwise_amd import _lib
from tests import stream_contract_cases as table


def test_the_header_parse_finds_the_streamed_functions():
    streamed = table.streamed_functions()
    assert {"conv3p_forward_f32", "conv3p_stack_forward_f64", "conv3p_stack_prefetch_f32", "conv3p_cache_init",
            "conv3p_grid_merge_segments", "conv3p_cls_tail_step_f32"} <= streamed
    # the status and profile calls have no stream parameter; the size functions neither
    assert not streamed & {"conv3p_cache_fused_status", "conv3p_cache_forget", "conv3p_profile_read", "conv3p_workspace_bytes"}
    assert streamed <= set(_lib.SYMBOLS)
    # every declaration with a stream argument in the binding is found in the header, by its last parameter's name
    text = re.sub(r"/\*.*?\*/", " ", open(table.HEADER).read(), flags=re.S)
    assert len(streamed) == len(set(re.findall(r"\b(conv3p_\w+)\s*\([^;{}()]*void\s*\*\s*stream\s*(?:,[^;{}()]*)?\)\s*;", text)))


def test_every_streamed_function_is_reached_or_exempt():
    reached = set().union(*(e.reaches for e in table.ENTRIES))
    streamed = table.streamed_functions()
    assert not reached & set(table.NOT_STREAMED), "a function is both reached and exempt"
    assert reached | set(table.NOT_STREAMED) == streamed, (sorted(streamed - reached - set(table.NOT_STREAMED)),
                                                           sorted((reached | set(table.NOT_STREAMED)) - streamed))
    assert all(isinstance(r, str) and r for r in table.NOT_STREAMED.values())


def test_every_public_name_has_a_case_or_a_reason():
    tokens = set()
    for name in table.NAMES:
        tokens.update(re.split(r"[^A-Za-z0-9_]+", name))
    for public in pointwise_amd.__all__:
        obj = getattr(pointwise_amd, public)
        assert callable(obj) or inspect.isclass(obj), public
        assert (public in tokens) != (public in table.NO_CASE), "%s needs a case or a reason, not both or neither" % public
    assert set(table.NO_CASE) <= set(pointwise_amd.__all__)
    assert all(isinstance(r, str) and r for r in table.NO_CASE.values())


def test_the_exemptions_name_cases_and_carry_their_reason():
    assert set(table.HOST_BY_CONTRACT) <= set(table.NAMES)
    assert all(isinstance(r, str) and "\"" in r for r in table.HOST_BY_CONTRACT.values()), "quote the docstring sentence"
    assert len(table.HOST_BY_CONTRACT) <= 4 and len(table.NOT_STREAMED) <= 1


def test_case_names_are_unique_and_reaches_are_declared():
    assert len(set(table.NAMES)) == len(table.NAMES)
    for e in table.ENTRIES:
        assert e.reaches and e.reaches <= set(_lib.SYMBOLS), e.name


def test_poison_matches_its_input_in_shape_and_dtype():
    for e in table.ENTRIES:
        real, poison = e.halves()
        assert len(real) == len(poison) and real, e.name
        for i, (r, p) in enumerate(zip(real, poison)):
            assert r.shape == p.shape and r.dtype == p.dtype, (e.name, i)
            assert r.size == 0 or not (r == p).all(), (e.name, i, "the poison equals the input")
