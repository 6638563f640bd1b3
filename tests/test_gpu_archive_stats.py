"""GPU tier: what the device archive's calls report is pinned, not bounded.  tests/archive_stats_cases.py runs every entry point
of csc_amd.csa.DeviceArchive over one small scenario; tests/golden/archive_stats.json is what that gave when it was recorded
(tools/make_golden_archive_stats.py).  Launch counts, wave counts, piece counts, the bytes up and down the bus, the files tables,
the diffs, the update's task table and the adler32 of every archive and destination must be the record's, field for field; only
the time fields are left out."""
import json

import pytest

import archive_stats_cases as S
from test_gpu_archive_device import codec  # noqa: F401  (the fixture: the oracle's encoder and decoder)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def recorded(csa, codec):  # noqa: F811
    with open(S.GOLDEN) as f:
        return S.record(csa, codec), json.load(f)


def test_every_call_is_in_the_record(recorded):
    got, want = recorded
    assert sorted(got) == sorted(want) and len(got) == 3 + 2 * 14
    assert all(r["rc"] == 0 for r in want.values()), "the scenario holds no failing call"


def test_statistics_are_the_recorded_ones(recorded):
    got, want = recorded
    got = json.loads(json.dumps(got))               # (tuples as lists, as the record holds them)
    for key in sorted(want):
        for field in sorted(set(want[key]["stats"]) | set(got[key]["stats"])):
            assert got[key]["stats"].get(field) == want[key]["stats"].get(field), (key, field)
        assert got[key] == want[key], key
