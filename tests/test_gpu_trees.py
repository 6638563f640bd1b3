"""GPU tier (-m gpu): what the level-3 spine hands to the tree wavefront (d6_trees, role 9) -- the literals' trees in p_lit, coded up to sixteen records a
pass in two halves of eight, and the match and rep packets' length and distance trees -- byte for byte against the
oracle (and the reference build oracle/_ref when it is there), every stream decoded again by the device decoder and compared with its
input.  Each case runs as one stream (k_encode_runs_dp4) and as three different streams in one CSCMI_EncodeDeviceChunkBatch
(k_encode_runs_multi_dp4): the case's input, the input rotated by a third and its first 60 000 bytes.

What the inputs make the parser do was counted on the CPU with tests/model/trees_model.c (tests/test_trees_model.py holds the counts
against these conditions on every run; a "way out" is a window's packets plus its exit packet, the figures are the case's own input):

  (a) short blocks      a 200-byte block repeated with single-byte edits 4..10 bytes apart, then pieces of 4..9 bytes copied from the last
                        1 000 bytes, 120 000 bytes: 28 ways out with more than eight match / rep records (most: 332); inside runs of eight
                        records 3 349 repeat an earlier record's length, 1 122 its distance slot under the same length class, 242 its extra
                        bits and low nibble
  (b) distance classes  pieces from 2 MiB back, 40..3 000 back, 4..32 back and 1..3 back side by side (2 199 152 bytes: a distance with more
                        than 20 extra bits is longer than 2 MiB, so this input alone exceeds 256 KB): match records with 0 / 1 / 2 direct
                        entries 3 206 / 3 417 / 602; 453 runs of eight consecutive records of one way out hold extra bits 0, 1..4, 5..20 and
                        > 20 together
  (c) ring wraps        text, then a 1 500-byte block with edits, 120 000 bytes: 24 415 literal and 9 886 match records (the rings hold 128
                        and 64); 65 and 66 ways out cross a ring's end with their records; 84 exit literals' records sit on slot 0 or 127
  (d) literal runs      pieces of 3..8 bytes copied from the last 300 bytes, 100 000 bytes: 253 ways out with more than sixteen literals
                        (most: 1 203), 14 225 records that repeat the (context, symbol) of a record in the other half of their group of
                        sixteen, 18 720 of one in their own group of eight
  (e) small dictionary  text | entropy8 | delta | text | entropy8, 240 000 bytes, dictionary 64 KiB: 18 431 positions leave without a window
                        (649 runs of eight or more), between 4 882 windows; 1 091 exit literals share their context row with a literal of
                        their window, 26 come behind a window of more than 64 nodes
  (f) long stream       256 KiB of text: 840 805 queue entries (the spine asks for room about every 2 000: some 400 times), 71 refreshes of
                        GetMatchLenPrice's table, 17 of them within the first eight nodes of a window whose predecessor left match records;
                        291 exit literals behind windows of more than 64 nodes
"""
import os

import pytest

import soak_gen
import trees_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = trees_cases.CASES


@pytest.fixture(scope="module")
def want(orc, zalloc):
    """the oracle's stream for every input of every case, computed once; and the reference build's, where there is one"""
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so")
    ref = None
    if os.path.exists(ref_path):
        from csc_amd.capi import CscLib
        ref = CscLib(ref_path)
    out = {}
    for name, (_, dict_size) in CASES.items():
        rows = []
        for data in trees_cases.streams_of(name):
            rc, s = orc.encode(data, 3, dict_size, alloc=zalloc)
            assert rc == 0
            if ref is not None:
                assert ref.encode(data, 3, dict_size, alloc=zalloc) == (0, s), f"{name}: oracle and reference build disagree"
            rows.append((data, s))
        out[name] = rows
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_single_stream(prod, want, name):
    data, s = want[name][0]
    rc, got = prod.encode(data, 3, CASES[name][1])
    assert rc == 0
    assert got == s, f"{name}: HIP stream differs from the oracle's ({len(got)} vs {len(s)} bytes)"
    assert prod.decode(got) == (0, data)


@pytest.mark.parametrize("name", list(CASES))
def test_batch_of_three(prod, want, name):
    rows = want[name]
    props = [prod.props_init(min(CASES[name][1], len(d)), 3) for d, _ in rows]      # (the dictionary clamped to the input, as CscLib.encode does for the oracle)
    got, rounds = soak_gen.encode_batch(prod, props, [d for d, _ in rows])
    assert rounds == (2 if max(len(d) for d, _ in rows) > 2 << 20 else 1)
    for i, (data, s) in enumerate(rows):
        assert got[i] == s, f"{name}: stream {i} of the batch differs from the oracle's ({len(got[i])} vs {len(s)} bytes)"
    dec = soak_gen.decode_batch(prod, got)
    assert dec == [(0, d) for d, _ in rows]
