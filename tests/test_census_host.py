"""CPU tier: the encoder census (tests/census_cases.py).  The frozen cases of tests/golden/census_cases.json must still reach the
events they were picked for when the oracle encodes them again, the oracle's stream must be the reference build's, every (event,
row) cell where the event's branch exists must have a case or stand in OPEN under its cap, and the block-size family must reach
the coder's seam and flush events in every row.  tests/test_gpu_census.py runs the same cases through every kernel form."""
import pytest

import census_cases as cc
import soak_gen

ALL = cc.load()["cases"]


@pytest.fixture(scope="module")
def counted(orc, zalloc):
    """every frozen case through the oracle once, census attached: name -> (rc, stream, counts)"""
    return {c["name"]: cc.census(orc, zalloc, c["spec"]) for c in ALL}


def test_names_match_the_oracle(orc):
    assert cc.oracle_names(orc) == cc.EVENTS
    assert set(cc.DEAD) <= set(cc.EVENTS) and all(ev in cc.EVENTS and row in cc.APPLIES[ev] for ev, row in cc.OPEN)


def test_rows_are_the_forms_tests():
    import test_gpu_forms as F
    assert list(F.FORMS) == cc.ROWS and all(soak_gen.spec_row(F._spec(row, k, 32768, [])) == row for row in cc.ROWS for k in range(3))


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_case_reaches_its_events(counted, case):
    rc, _, got = counted[case["name"]]
    assert rc == 0
    assert soak_gen.spec_row(case["spec"]) == case["row"]
    assert len(soak_gen.build_input(case["spec"])) == case["size"] <= cc.MAX_CASE
    assert case["events"], "a case that claims nothing"
    short = {ev: (got[ev], n) for ev, n in case["events"].items() if got[ev] < n}
    assert not short, f"(counted, recorded): {short}"
    chk, za, _ = soak_gen.checker()
    _, s, rcd, back = soak_gen.check_one(chk, za, case["spec"], soak_gen.build_input(case["spec"]))
    assert s == counted[case["name"]][1] and (rcd == 0 and back == soak_gen.build_input(case["spec"])) == case["decodes"]
    if case["spec"]["props"].get("csc_blocksize", 65536) < cc.load()["floor"]["floor"]:
        assert not case["decodes"]


def test_oracle_stream_is_the_reference_builds(ref, zalloc, counted):
    for c in ALL:
        rc, s = ref.encode(soak_gen.build_input(c["spec"]), props=soak_gen.props_of(ref, c["spec"]), alloc=zalloc)
        assert rc == 0 and s == counted[c["name"]][1], c["name"]


def test_every_cell_has_a_case_or_is_open():
    have = {(ev, c["row"]) for c in ALL for ev in c["events"]}
    cells = {(ev, row) for ev in cc.EVENTS for row in cc.APPLIES[ev]}
    assert have <= cells, have - cells
    dead = {(ev, row) for ev in cc.DEAD for row in cc.APPLIES[ev]}
    assert not have & dead, "an event argued dead has a case: the argument in oracle/orc_encoder.c is wrong"
    missing = cells - have - dead - set(cc.OPEN)
    assert not missing, sorted(missing)
    assert not set(cc.OPEN) & have, "OPEN names a cell that has a case"
    for row in cc.ROWS:
        assert sum(c["size"] for c in cc.cases_of(row)) <= cc.MAX_ROW


def test_open_stays_under_its_cap():
    open_rows = {}
    for ev, row in cc.OPEN:
        assert ev not in cc.DEAD and cc.OPEN[(ev, row)]
        open_rows.setdefault(ev, set()).add(row)
    assert not [ev for ev in open_rows if ev in cc.CODER], "no coder event may be open in any row"
    everywhere = [ev for ev, rows in open_rows.items() if rows == set(cc.APPLIES[ev]) and len(rows) > 1]
    assert len(everywhere) <= 2, everywhere
    assert not [ev for ev, rows in open_rows.items() if ev not in everywhere and len(rows) > 1]


def test_dead_events_stay_dead(counted):
    for name, (_, _, got) in counted.items():
        assert not [ev for ev in cc.DEAD if got[ev]], name


@pytest.mark.parametrize("row", cc.ROWS)
def test_block_size_family(orc, zalloc, row):
    """from the census: over csc_blocksize 16 / 17 / 255 / 4096 the family reaches every event of FAMILY_MUST_HIT in this row; the
    recorded counts and the recorded verdict of the checker's decoder still hold; below the floor the decoder refuses the stream"""
    rec = cc.load()["family"][row]
    floor = cc.load()["floor"]["floor"]
    chk, za, _ = soak_gen.checker()
    total = {ev: 0 for ev in cc.FAMILY_MUST_HIT}
    for (name, spec), (member, _, decodes) in zip(cc.family_members(row), cc.family_specs(row)):
        assert soak_gen.spec_row(spec) == row
        data = soak_gen.build_input(spec)
        rc, s, got = cc.census(orc, zalloc, spec, data)
        assert rc == 0 and {ev: got[ev] for ev in cc.CODER if got[ev]} == rec[name]["events"], member
        rc2, s2, rcd, back = soak_gen.check_one(chk, za, spec, data)
        assert rc2 == 0 and s2 == s, member
        assert (rcd == 0 and back == data) == decodes, member
        if spec["props"]["csc_blocksize"] < floor:
            assert not decodes
        else:
            assert decodes or (rcd == -1 and got["flush_bc_empty"]) or rcd == -96, member      # the two hazards above the floor
        if spec["props"]["csc_blocksize"] in cc.FAMILY_BSIZES:
            for ev in total:
                total[ev] += got[ev]
    assert all(total.values()), total


def test_floor_record():
    f = cc.load()["floor"]
    assert f["floor"] == 6 and min(f["tried"]) == 1 and {b for b, _ in cc.FAMILY_BELOW_FLOOR} == {1, 3}
    assert all(b >= f["floor"] for b in f["empty_bc_block"] + f["decode_error"])
