"""CPU tests (not gpu) of the Python host mirror: tests/host_mirror_cases.py replayed against tests/golden/host_mirror.json,
which was recorded from the package before its argument checks, scratch handling and views were stated once
(pointwise_amd/_host.py).  Every exception class, message and check order, every view's shape, ownership and offset, and
the host-only block bounds must come out equal."""
import json

import pytest

from tests import host_mirror_cases as cases

with open(cases.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_the_table_and_the_record_name_the_same_entries():
    assert sorted(cases.TABLE) == sorted(GOLDEN)
    assert sum(cases.count(v) for v in GOLDEN.values()) == 1119          # as recorded; a shrunken record pins less


@pytest.mark.parametrize("name", sorted(cases.TABLE))
def test_entry_replays_as_recorded(name):
    got = json.loads(json.dumps(cases.TABLE[name]()))                    # tuples and lists compare alike
    want = GOLDEN[name]
    if isinstance(got, list) and isinstance(want, list):
        assert len(got) == len(want)
        for rung, (g, w) in enumerate(zip(got, want)):
            assert g == w, "rung %d of %s" % (rung, name)
    assert got == want
