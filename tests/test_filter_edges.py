"""CPU tier for the adversarial filter and analyzer cases (tests/filter_cases.py): the oracle gives what the REFERENCE
recorded for every case (tests/golden/filter_edges.json, tools/make_golden_filter_edges.py) and what the reference gives live
where oracle/_ref is built; forward then inverse is the identity wherever the reference accepts; the generator is
deterministic; the 82 % boundary pairs land on the dstSize they were built for, the lower accepted and the upper rejected.

Sensitivity: plain-Python restatements of Forward_E89 and of the dictionary filter's token chain reproduce the reference on
every case -- and, with ONE mistake planted, differ from it on at least one case that the test names.  A planted mistake
that no case catches means that the case list is incomplete."""
import json
import os

import pytest

import filter_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "filter_edges.json")
REF = os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def groups(orc):
    return F.all_cases(orc.lib)


@pytest.fixture(scope="module")
def orc_out(orc, groups):
    """the oracle's outputs, computed once and shared (never modified)"""
    return F.outputs_of(F.Probes(orc.lib, "orc"), groups)


def test_generator_is_deterministic(orc, groups):
    assert F.all_cases(orc.lib) == groups
    assert sum(len(g) for g in groups.values()) == len({n for g in groups.values() for n in g})


def test_golden_has_no_stale_and_no_missing_names(groups, golden):
    assert set(golden) == {n for g in groups.values() for n in g}


@pytest.mark.parametrize("group", ["e89", "delta", "dict", "analyze"])
def test_oracle_matches_the_recorded_reference(groups, orc_out, golden, group):
    for name in groups[group]:
        assert F.golden_entry(groups, name, orc_out[name]) == golden[name], name


@pytest.mark.parametrize("group", ["e89", "delta", "dict", "analyze"])
def test_oracle_matches_the_reference_live(groups, orc_out, golden, group):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/libcsc_ref.so not built")
    from csc_amd.capi import CscLib
    sub = {g: (groups[g] if g == group else {}) for g in groups}
    for name, want in F.outputs_of(F.Probes(CscLib(REF).lib, "ref"), sub).items():
        got = orc_out[name]
        if group == "analyze":
            assert got == want, name
        else:
            assert got[:-1] == want[:-1], name
            assert got[-1] == want[-1], f"{name}: {F.first_difference(got[-1], want[-1])}"
        assert F.golden_entry(groups, name, want) == golden[name], f"{name}: the golden file is stale"


def test_forward_then_inverse_is_the_identity(orc, groups, orc_out):
    p = F.Probes(orc.lib, "orc")
    for name, data in groups["e89"].items():
        assert p.run("inverse_e89", orc_out[name][1])[1] == data, name
    for name, (data, chn) in groups["delta"].items():
        assert p.run("inverse_delta", orc_out[name][1], chn)[1] == data, name
    accepted = 0
    for name, (data, _) in groups["dict"].items():
        _, ok, out = orc_out[name]
        if ok:
            accepted += 1
            assert p.run("inverse_dict", out)[1] == data, name
        else:
            assert out == data, f"{name}: a refused run is left as it was"
    assert accepted > len(groups["dict"]) // 2


def test_reject_boundary_and_copy_back_cases_are_what_they_were_built_for(groups, golden):
    pairs = 0
    for size in F.reject_sizes():
        lo, hi = golden[f"dict/reject/{size}/at"], golden[f"dict/reject/{size}/above"]
        assert lo["dst_size"] == int(size * 0.82) and hi["dst_size"] == lo["dst_size"] + 1
        assert lo["dict_ok"] == 1 and hi["dict_ok"] == 0, size
        assert len(groups["dict"][f"dict/reject/{size}/at"][0]) == size
        pairs += 1
    assert pairs >= 3
    seen = set()
    for name, (data, dst) in groups["dict"].items():
        if name.startswith("dict/copyback/"):
            assert golden[name]["dict_ok"] == 1 and golden[name]["dst_size"] == dst
            seen.add((len(data) % 16, dst % 16))
    assert seen == {(a, b) for a in (0, 1, 15) for b in (0, 1, 15)}
    assert golden["dict/size/16383"]["dict_ok"] == 0 and golden["dict/size/16384"]["dict_ok"] == 1


# ---- sensitivity ---------------------------------------------------------------------------------------------------------

def _caught(cases, golden, restated):
    """names of the cases on which a restatement's output differs from the reference's recorded one"""
    return [name for name, data in cases.items() if F.digest(restated(data)) != golden[name]["sha256"]]


def test_restated_e89_is_the_reference(groups, golden):
    assert _caught(groups["e89"], golden, F.forward_e89) == []


@pytest.mark.parametrize("mistake,kw,witness", [
    ("skip j + 5", {"skip": 5}, "e89/top/e8/10"),
    ("skip j + 3", {"skip": 3}, "e89/phase/start/0"),
    ("eligible one further", {"bound": 4}, "e89/end/100/5/e8"),
    ("eligible one short", {"bound": 6}, "e89/end/100/6/e8"),
])
def test_e89_cases_catch_a_planted_mistake(groups, golden, mistake, kw, witness):
    hits = _caught(groups["e89"], golden, lambda d: F.forward_e89(d, **kw))
    assert witness in hits, f"{mistake}: caught by {hits[:8]}"


def _dict_caught(orc, groups, golden, **kw):
    w = F.words(orc.lib)
    hits = []
    for name, (data, _) in groups["dict"].items():
        ok, out, _ = F.forward_dict(data, w, **kw)
        if ok != golden[name]["dict_ok"] or F.digest(out) != golden[name]["sha256"]:
            hits.append(name)
    return hits


def test_restated_dict_chain_is_the_reference(orc, groups, golden):
    assert _dict_caught(orc, groups, golden) == []


def test_dict_cases_catch_a_chain_not_carried_across_a_step(orc, groups, golden):
    hits = _dict_caught(orc, groups, golden, carry=False)
    for witness in ("dict/straddle/0/0/4/62", "dict/straddle/2/3/2/60", "dict/backtoback/1"):
        assert witness in hits, hits[:8]


def test_dict_cases_catch_ge_for_gt_at_the_82_percent_test(orc, groups, golden):
    hits = _dict_caught(orc, groups, golden, reject=lambda dst, size: dst >= size * 0.82)
    assert hits and all(h.startswith("dict/reject/") and h.endswith("/at") for h in hits), hits
    assert "dict/reject/16400/at" in hits
