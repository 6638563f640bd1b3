"""CPU tier for the chunk-walk and duplicate-check cases (tests/walk_cases.py): the oracle writes the stream the REFERENCE
recorded for every case (tests/golden/walk_edges.json, tools/make_golden_walk_edges.py) and the one the reference writes live
where oracle/_ref is built, and decodes it as the reference does; the oracle's trace (orc_trace_*) shows every claim of every
case and fills every cell of walk_cases.COVERAGE; two plain-Python restatements -- the walk from the per-block figures, the
TestFind verdict from the per-candidate figures -- equal the oracle on every case and, with ONE mistake planted, differ from
it on a case that the test names.  A planted mistake that no case catches means that the case list is incomplete."""
import json
import os

import pytest

import soak_gen
import walk_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "walk_edges.json")
REF = os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so")
FAMILY_NAMES = ("types", "skip", "bpb95", "runs", "dup")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(orc):
    return W.all_cases(orc.lib)


@pytest.fixture(scope="module")
def traced(orc, zalloc, cases):
    """name -> (rc, stream, Trace) of the oracle, computed once and shared (never modified)"""
    return {c.name: W.traced_encode(orc, zalloc, c) for c in cases}


def _family(cases, fam):
    return [c for c in cases if c.name.split("/")[0] == fam]


def test_generator_is_deterministic_and_small(orc, cases):
    again = W.all_cases(orc.lib)
    assert [(c.name, c.data, c.spec) for c in again] == [(c.name, c.data, c.spec) for c in cases]
    assert {c.name.split("/")[0] for c in cases} == set(FAMILY_NAMES)
    for c in cases:
        assert len(c.data) <= 300_000, c.name
        assert 32 << 10 <= soak_gen.props_of(orc, c.spec).dict_size <= (1 << 20) + 10240, c.name


def test_golden_has_no_stale_and_no_missing_names(cases, golden):
    assert set(golden) == {c.name for c in cases}


def test_the_trace_changes_nothing(orc, zalloc, cases, traced):
    for c in cases[::7]:
        rc, s, _, _ = soak_gen.check_one(orc, zalloc, c.spec, c.data)
        assert (rc, s) == traced[c.name][:2], c.name


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_oracle_matches_the_recorded_reference(orc, zalloc, cases, traced, golden, fam):
    for c in _family(cases, fam):
        rc, s, _ = traced[c.name]
        assert rc == 0, c.name
        assert W.golden_entry(s, orc.decode(s, alloc=zalloc)) == golden[c.name], c.name


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_oracle_matches_the_reference_live(orc, zalloc, cases, traced, golden, fam):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/libcsc_ref.so not built")
    from csc_amd.capi import CscLib
    ref = CscLib(REF)
    for c in _family(cases, fam):
        rc, s, rcd, back = soak_gen.check_one(ref, zalloc, c.spec, c.data)
        assert (rc, s) == traced[c.name][:2], c.name
        assert orc.decode(s, alloc=zalloc) == (rcd, back), c.name
        assert W.golden_entry(s, (rcd, back)) == golden[c.name], f"{c.name}: the golden file is stale"


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_every_case_shows_the_branch_it_claims(cases, traced, fam):
    for c in _family(cases, fam):
        assert c.claims, c.name
        assert W.failed_claims(c, traced[c.name][2]) == [], c.name


def test_coverage_table_is_complete_cell_by_cell(cases, traced):
    """a cell counts when a case that names it has all its claims in the trace (the test above), plus, for the cells that are
    plain trace facts, the fact itself"""
    shown = {}
    for c in cases:
        if not W.failed_claims(c, traced[c.name][2]):
            for cell in c.cells:
                shown.setdefault(cell, []).append(c.name)
    empty = [cell for cell in W.COVERAGE if not shown.get(cell)]
    assert not empty, empty
    assert set(shown) <= set(W.COVERAGE), sorted(set(shown) - set(W.COVERAGE))
    verdicts = {b[W.B_AN] for _, _, tr in traced.values() for b in tr.blocks}
    assert verdicts >= set(W.TYPE_NAMES), sorted(set(W.TYPE_NAMES) - verdicts)
    pairs = set()
    for _, _, tr in traced.values():
        pairs |= {(a[W.B_AN], b[W.B_AN]) for a, b in zip(tr.blocks, tr.blocks[1:]) if a[W.B_CHUNK] == b[W.B_CHUNK]}
    main = [W.TYPE_OF[n] for n in W.MAIN_TYPES]
    assert pairs >= {(a, b) for a in main for b in main}
    tables = {(c[W.C_TABLE], c[W.C_HIT]) for _, _, tr in traced.values() for c in tr.cands}
    assert tables == {(0, 0), (0, 1), (1, 0), (1, 1)}, tables


def test_both_sides_of_the_095_line_are_taken(traced):
    got = {}
    for side in ("under", "on", "over"):
        b = traced[f"bpb95/{side}"][2].blocks[1]
        got[side] = (b[W.B_DLT_USED] - b[W.B_BPB] * 0.95, b[W.B_BPB95])
    assert -1 < got["under"][0] < 0 and got["under"][1] == W.DT_DLT
    assert got["on"][0] == 0.0 and got["on"][1] == W.DT_NORMAL
    assert 0 < got["over"][0] < 1 and got["over"][1] == W.DT_NORMAL


def test_form_cases_keep_their_verdicts_in_every_props_row(orc, zalloc, cases):
    """tests/test_gpu_walk.py runs FORM_CASES under variant 0 of every row of the dispatch table: the hits stay hits and the
    near misses stay misses there (the hash geometry changes, the planted keys do not collide)"""
    from test_gpu_forms import FORMS
    by_name = {c.name: c for c in cases}
    assert set(W.FORM_CASES) <= set(by_name)
    verdicts = set()
    for row, form in FORMS.items():
        for name in W.FORM_CASES:
            c = W.in_form(by_name[name], form["variants"][0])
            assert soak_gen.spec_row(c.spec) == row
            tr = W.traced_encode(orc, zalloc, c)[2]
            for ch, blk, dup in W.dup_claims(c):
                got = [b[W.B_DUP] for b in tr.blocks if b[:2] == (ch, blk)]
                assert got == [dup], (row, name, blk, got)
                verdicts.add(dup)
            assert W.dup_claims(c), name
    assert verdicts == {0, 1}


# ---- restatements driven by the trace, and their planted mistakes ----------------------------------------------------------

def _switches(orc, c):
    p = soak_gen.props_of(orc, c.spec)
    return (p.DLTFilter, p.TXTFilter, p.EXEFilter), p.raw_blocksize


def _walk_caught(orc, cases, traced, mistake=None):
    hits = []
    for c in cases:
        tr = traced[c.name][2]
        sw, raw = _switches(orc, c)
        if W.walk(tr.blocks, raw, sw, mistake) != [tuple(r) for r in tr.runs]:
            hits.append(c.name)
    return hits


def _find_caught(cases, traced, mistake=None):
    hits = []
    for c in cases:
        tr = traced[c.name][2]
        for b in tr.blocks:
            if b[W.B_DUP] == 2:
                continue
            cands = [x for x in tr.cands if x[:2] == b[:2]]
            if W.test_find_verdict(cands, mistake) != bool(b[W.B_DUP]):
                hits.append(c.name)
                break
    return hits


def test_restated_walk_is_the_oracle(orc, cases, traced):
    assert _walk_caught(orc, cases, traced) == []


def test_restated_test_find_is_the_oracle(cases, traced):
    assert _find_caught(cases, traced) == []
    assert sum(len(tr.cands) for _, _, tr in traced.values()) > 10_000


@pytest.mark.parametrize("mistake,witness", [
    ("bpb_cleared_on_skip", "skip/dlt2/tail511"),
    ("gt_at_095", "bpb95/on"),
    ("merge_across_chunks", "runs/exactly_raw_plus_one/bad"),
    ("ge_at_raw_blocksize", "runs/exactly_raw_plus_one/normal"),
    ("fast_merged", "types/fast_next_to_normal"),
])
def test_walk_cases_catch_a_planted_mistake(orc, cases, traced, mistake, witness):
    hits = _walk_caught(orc, cases, traced, mistake)
    assert witness in hits, f"{mistake}: caught by {hits[:8]}"


def test_switches_after_the_delta_rule_is_no_mistake(orc, cases, traced):
    """the filter switches and the 0.95 rule both only ever turn a delta type into DT_NORMAL, and neither looks at what the
    other left: in either order the block ends as DT_NORMAL exactly when one of them says so.  The swapped order is the same
    function of the block -- no stream can tell -- so there is no case to name; what is held is that the cases with
    DLTFilter off and a delta block in them agree under both orders."""
    assert _walk_caught(orc, cases, traced, "switches_after_delta_rule") == []
    assert any(b[W.B_AN] >= W.DT_DLT and b[W.B_AN] != W.DT_SKIP and b[W.B_SWITCH] == W.DT_NORMAL
               for n in ("types/switch_off/D", "types/switch_off/DT", "types/switch_off/DE") for b in traced[n][2].blocks)


@pytest.mark.parametrize("mistake,witness", [
    ("ge_18", "dup/equal18"),
    ("climit_without_window", "dup/window_end/18"),
    ("dist_gt_vld", "dup/dist/vld"),
    ("wpos_gt_dist", "dup/wpos_eq_dist"),
])
def test_dup_cases_catch_a_planted_mistake(cases, traced, mistake, witness):
    hits = _find_caught(cases, traced, mistake)
    assert witness in hits, f"{mistake}: caught by {hits[:8]}"
