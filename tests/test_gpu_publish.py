"""GPU tier (-m gpu): the level-3 spine asking for room in the coder's queue (d6_room, csc_amd/csrc/csc_kernels_dp4.inc) while the tree
wavefront still has records to code -- the spine publishes what is complete instead of waiting for the trees -- byte for byte against the
oracle (and the reference build oracle/_ref when it is there), every stream decoded again and compared with its input.  Each input runs as
one stream (k_encode_runs_dp4) and as three different streams in one CSCMI_EncodeDeviceChunkBatch (k_encode_runs_multi_dp4): the input, the
input rotated by a third and its first 60 000 bytes.  The queue holds 4 096 entries and fills about every 1.3 KB of input, so each of
these inputs (at most 128 KiB) asks for room fifty times and more.

  (i)   text            96 KiB of text: the plain case, literal and match records outstanding together
  (ii)  literal runs    pieces of 3..8 bytes copied from the last 300 bytes: ways out with more than 120 literals (the literal ring fills),
                        the packet-at-a-time path, the oldest record far behind the head (the join that is left)
  (iii) short matches   a 200-byte block repeated with single-byte edits 4..10 bytes apart: the match ring near full when room is asked for
  (iv)  long matches    a 4 KiB block repeated with edits 300..900 bytes apart: lengths from 145 on are coded in line, behind a join, between
                        deferred records
  (v)   small window    entropy8 under a 64 KiB dictionary: literals without a window, d6_room(16) -- where the block analysis leaves the
                        bytes to the LZ parser at all: on this input alone it does not (the development counters show no window and no
                        request for room), hence
  (vi)  mixed           text | entropy8 | text under the same dictionary, the shape of tests/test_gpu_trees.py's case (e)

Which branch of the slow path a call takes depends on timing and cannot be asserted here; profiles/publish_lanes.md holds the development
build's counters for these inputs (calls, joins, records outstanding)."""
import os

import pytest

import cases
import soak_gen
import trees_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (input, dictionary)
CASES = {
    "i_text": (lambda: cases.build([["text", 71, 0, 96 << 10]]), 1 << 20),
    "ii_literal_runs": (lambda: trees_cases.shuffled(72, 300, 96 << 10, 3, 6), 256 << 10),
    "iii_short_matches": (lambda: trees_cases.mutated(73, 200, 96 << 10, 4, 10), 256 << 10),
    "iv_long_matches": (lambda: trees_cases.mutated(74, 4096, 128 << 10, 300, 900), 256 << 10),
    "v_small_window": (lambda: cases.build([["entropy8", 75, 0, 96 << 10]]), 64 << 10),
    "vi_mixed_small_window": (lambda: cases.build([["text", 76, 0, 40000], ["entropy8", 77, 0, 40000], ["text", 76, 40000, 40000]]), 64 << 10),
}


def streams_of(name):
    data = CASES[name][0]()
    assert len(data) <= 128 << 10
    return [data, data[len(data) // 3:] + data[:len(data) // 3], data[:60000]]


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
        for data in streams_of(name):
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
    assert rounds == 1
    for i, (data, s) in enumerate(rows):
        assert got[i] == s, f"{name}: stream {i} of the batch differs from the oracle's ({len(got[i])} vs {len(s)} bytes)"
    dec = soak_gen.decode_batch(prod, got)
    assert dec == [(0, d) for d, _ in rows]
