"""The host's launch decisions, pinned (-m gpu): every case of tests/launch_census_cases.py runs with the profile on, and
the {kind name: launches} map of each of its calls -- the forward and the backward of every variant, the calls of the
sequences on one cache, the passes of the stack-level entry points -- equals the record in tests/golden/launch_census.json.
The counts are host-side launch scopes: they do not depend on the data or on the device, only on which launchers the host
glue of csrc/conv3p_abi*.hpp runs, which zero-fills it issues, when it skips a search and which companions ride along."""
import json

import pytest
import torch

from pointwise_amd import _lib
from tests import launch_census_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(cases.GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_launch_census(dev, golden, name):
    census, _ = cases.CASES[name](dev)
    assert sorted(census) == sorted(golden[name]), (name, "variants", sorted(census))
    for variant, seen in census.items():
        assert seen == golden[name][variant], (name, variant, seen, "recorded", golden[name][variant])
