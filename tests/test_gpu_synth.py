"""GPU tier for the stream synthesizer: the device decoder on valid streams no encoder writes, and on streams the
reference refuses at a defined point (tests/synth_gen.py draws them and predicts the answer; tests/test_synth_gen.py pins
generator, oracle and reference to each other on the CPU).

Every stream is decoded alone (whole and ragged Reads) and through CSCMI_DecodeBatch with all families and the refused
streams mixed in one call; the answer must be the checker's (the reference where oracle/_ref is built, else the oracle),
the prediction and the reference's recorded line in tests/golden/synth.json.  Refused streams are parity of a defined answer:
each is decoded once per path.

The test-only build in which every packet takes the checkpointed path (DEC_DBG_CAREFUL) is not part of this file: tests/stage
carries no decoder variant today and building one means a second device compile of the decoder in build().

long_chain (one packet with more than kDecUndoCap = 32 768 long-length bits, only reachable with raw_blocksize > 32 768 x 143
bytes in the header): the reference decodes it, the device journals one entry a bit and refuses the packet.  Parity is
knowingly not reached there; the test asserts the documented answer (include/csc_mi355x.h): DECODE_ERROR with
every earlier run delivered and no byte of that run.  Measured on an MI355X: rc -96 after the first run's 100 bytes."""
import json
import os

import pytest

import soak_gen
import synth_gen as G
from csc_amd.capi import DECODE_ERROR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_SEEDS = [(f, s) for f in G.FAMILIES for s in G.FAMILIES[f] if f not in ("long_chain", "long_rle")]
_memo = {}


def _golden():
    if "golden" not in _memo:
        with open(os.path.join(ROOT, "tests", "golden", "synth.json")) as f:
            _memo["golden"] = {g["id"]: g for g in json.load(f)}
    return _memo["golden"]


def _want(orc, family, seed):
    """[(case, stream, (rc, bytes))]: the checker's answer, checked against the prediction and the golden line"""
    if (family, seed) not in _memo:
        chk, za, _ = soak_gen.checker()
        rows = []
        for case in G.cases(orc.lib, family, seed):
            st = G.stream(orc.lib, case)
            want = chk.decode(st, alloc=za)
            assert want == (case["rc"], case["out"]), f"checker differs from the prediction; {G.describe(case)}"
            line = _golden()[G.case_id(case)]
            assert dict(G.golden_line(case, st, *want), short=line["short"]) == line, f"golden line differs; {G.describe(case)}"
            rows.append((case, st, want))
        _memo[family, seed] = rows
    return _memo[family, seed]


def _same(got, want, case, how):
    assert got[0] == want[0] and got[1] == want[1], \
        f"{how}: rc {got[0]} len {len(got[1])}, reference rc {want[0]} len {len(want[1])}, first difference at " \
        f"{next((i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b), min(len(got[1]), len(want[1])))}; {G.describe(case)}"


@pytest.mark.parametrize("family,seed", FAMILY_SEEDS)
def test_device_decoder_on_synthesized_streams(prod, orc, family, seed):
    chk, za, _ = soak_gen.checker()
    for case, st, want in _want(orc, family, seed):
        _same(prod.decode(st), want, case, "alone")
        if case["rc"] == 0:                                       # (a refused stream is decoded once per path)
            mr = 65537 if case["meta"].get("big") else [257, 1000, 65537][case["meta"]["index"] % 3]
            got = prod.decode(st, max_read=mr)
            _same(got, chk.decode(st, alloc=za, max_read=mr), case, f"max_read {mr}")
            assert G.digest(*got) == _golden()[G.case_id(case)]["short"][str(mr)], f"max_read {mr}: not the reference's recorded answer; {G.describe(case)}"


@pytest.mark.parametrize("group", [256, 7, 1])
def test_device_decoder_batch_on_synthesized_streams(prod, orc, group):
    rows = [r for f, s in FAMILY_SEEDS for r in _want(orc, f, s)]
    if group != 256:                                              # the long copies once; the coverage table's cases at every size
        rows = [r for r in rows if not r[0]["meta"].get("big")]
    if group == 1:
        rows = rows[::4]
    rows = rows[1::2] + rows[0::2]                                # families and refused streams mixed within a call
    got = soak_gen.decode_batch(prod, [st for _, st, _ in rows], group=group)
    for (case, _, want), g in zip(rows, got):
        _same(g, want, case, f"CSCMI_DecodeBatch, {group} a call")


def test_long_rle(prod, orc):
    """The same limit at the DEFAULT geometry: an RLE run of the delta path coded as about 5 000 000 and clipped by its block of a
    few hundred bytes.  The reference decodes it (rc 0); the device counts the long-length bits of the run length like a copy's and
    refuses.  Asserted: the documented answer, DECODE_ERROR with the earlier run delivered and no byte of the block."""
    (case, st, want), = _want(orc, "long_rle", G.FAMILIES["long_rle"][0])
    got = prod.decode(st)
    print(f"long_rle: rc {got[0]} after {len(got[1])} bytes (reference: rc {want[0]}, {len(want[1])} bytes)")
    assert got[0] == DECODE_ERROR and got[1] == want[1][:100], \
        f"rc {got[0]} len {len(got[1])}: not the documented refusal; {G.describe(case)}"


def test_long_chain(prod, orc):
    (case, st, want), = _want(orc, "long_chain", G.FAMILIES["long_chain"][0])
    got = prod.decode(st)
    first_run = 100                                               # the run delivered before the long packet's
    print(f"long_chain: rc {got[0]} after {len(got[1])} bytes (reference: rc {want[0]}, {len(want[1])} bytes)")
    assert got[0] == DECODE_ERROR and got[1] == want[1][:first_run], \
        f"rc {got[0]} len {len(got[1])}: not the documented refusal; {G.describe(case)}"
