"""GPU tier (-m gpu): the chunk walk of the encoder kernels (seg_next, dev_is_duplicate, k_analyze's verdicts) on the cases of
tests/walk_cases.py, each of which the CPU tier (tests/test_walk_edges.py) has shown to reach the branch it names.

  single stream   every case through CSCEnc_Encode in the form its own props select: stream == the reference's recorded one
                  (tests/golden/walk_edges.json), and decoded on the device == the reference decoder's recorded (rc, digest)
  batch           all cases of one kernel flavour in one CSCMI_EncodeDeviceChunkBatch call a chunk round (the `multi`
                  kernels, every stream with its own raw_blocksize): every stream == golden, one launch a round
  every form      the duplicate check's hit and near-miss cases (walk_cases.FORM_CASES) under variant 0 of each row of
                  test_gpu_forms.FORMS, as single streams and in 8-stream batches, against the checker (oracle/_ref when it is
                  there, the oracle otherwise)

No test plants a fault on the device, slows a wavefront or patches a kernel."""
import json
import os

import pytest

import soak_gen
import walk_cases as W
from test_gpu_forms import FORMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = ("types", "skip", "bpb95", "runs", "dup")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "walk_edges.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(orc):
    return W.all_cases(orc.lib)


@pytest.fixture(scope="module")
def chk():
    return soak_gen.checker()[:2]


def _stream_line(s):
    return {"stream_size": len(s), "stream_sha256": W.digest(s)}


def _want(golden, name):
    g = golden[name]
    return {"stream_size": g["stream_size"], "stream_sha256": g["stream_sha256"]}


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_single(prod, cases, golden, fam):
    n = 0
    for c in cases:
        if c.name.split("/")[0] != fam:
            continue
        rc, s = prod.encode(c.data, props=soak_gen.props_of(prod, c.spec))
        assert rc == 0, c.name
        assert _stream_line(s) == _want(golden, c.name), f"{c.name}: HIP stream differs from the reference's ({c.claims})"
        rcd, back = prod.decode(s)
        assert (rcd, W.digest(back)) == (golden[c.name]["dec_rc"], golden[c.name]["dec_sha256"]), f"{c.name}: device decoder differs from the reference's"
        n += 1
    assert n


def _rows(cases):
    rows = {}
    for c in cases:
        rows.setdefault(soak_gen.spec_row(c.spec), []).append(c)
    return rows


def _chunks(prod, c):
    raw = soak_gen.props_of(prod, c.spec).raw_blocksize
    return raw, -(-len(c.data) // raw)


@pytest.mark.parametrize("row", ["level12", "level3", "adv_generic"])
def test_batch(prod, cases, golden, row):
    """every case of the flavour in one call a chunk round; the stream with the most chunks leads, so that its handle counts
    every round's launch"""
    group = sorted(_rows(cases)[row], key=lambda c: -_chunks(prod, c)[1])
    props = [soak_gen.props_of(prod, c.spec) for c in group]
    stats = []
    got, rounds = soak_gen.encode_batch(prod, props, [c.data for c in group], chunk=[p.raw_blocksize for p in props], stats=stats)
    assert rounds == _chunks(prod, group[0])[1]
    bad = [c.name for c, s in zip(group, got) if _stream_line(s) != _want(golden, c.name)]
    assert not bad, f"{len(bad)} of {len(group)} batch streams differ from the reference's: {bad[:6]}"
    assert stats[0].encode_launches == rounds, (stats[0].encode_launches, rounds)
    dec = soak_gen.decode_batch(prod, got)
    bad = [c.name for c, (rc, back) in zip(group, dec) if (rc, W.digest(back)) != (golden[c.name]["dec_rc"], golden[c.name]["dec_sha256"])]
    assert not bad, bad[:6]


def test_batch_rows_are_all_the_rows_the_cases_select(cases):
    assert set(_rows(cases)) == {"level12", "level3", "adv_generic"}


@pytest.mark.parametrize("row", list(FORMS), ids=[f"{r}-{f['single']}+{f['multi']}" for r, f in FORMS.items()])
def test_duplicate_check_in_every_form(prod, chk, cases, row):
    by_name = {c.name: c for c in cases}
    group = [W.in_form(by_name[n], FORMS[row]["variants"][0]) for n in W.FORM_CASES]
    want = []
    for c in group:
        assert soak_gen.spec_row(c.spec) == row
        rc2, s2, rcd2, back2 = soak_gen.check_one(*chk, c.spec, c.data)
        assert rc2 == 0
        want.append((s2, rcd2, back2))
        rc, s = prod.encode(c.data, props=soak_gen.props_of(prod, c.spec))
        assert rc == 0 and s == s2, f"{row} {c.name}: HIP stream differs from the checker's ({len(s)} vs {len(s2)} bytes; {c.claims})"
        assert prod.decode(s) == (rcd2, back2), f"{row} {c.name}: device decoder differs from the checker's"
    for part in (range(0, 8), range(len(group) - 8, len(group))):          # two 8-stream calls hold every case
        sub = [group[i] for i in part]
        got, rounds = soak_gen.encode_batch(prod, [soak_gen.props_of(prod, c.spec) for c in sub], [c.data for c in sub])
        assert rounds == 1
        bad = [c.name for c, s, i in zip(sub, got, part) if s != want[i][0]]
        assert not bad, f"{row}: batch streams differ from the checker's: {bad}"
