"""GPU tier (-m gpu): the level-3 way out -- a window's packets coded 64 at a time in lanes (d6_chunk_lanes), the packet-at-a-time
loop it falls back to, the window-less literals and the exit packets around them -- byte for byte against the oracle (and the
reference build oracle/_ref when it is there), every stream decoded again by the device decoder and compared with its input.
Each case runs as one stream (k_encode_runs_dp4) and as three different streams in one CSCMI_EncodeDeviceChunkBatch
(k_encode_runs_multi_dp4): the case's input, the input rotated by a third and its first 60 000 bytes.

What the inputs make the level-3 parser do was measured on the CPU, with tests/model/m3_model.c counting per window (the way
out's packets between two exits; "nodes" = the window's length in positions, the kernel takes 64 nodes a chunk):

  (a) text       200 000 bytes of text, dictionary 1 MiB: 6 228 windows, the common shapes; 165 of them longer than 64 nodes
                 (longest 209), at most 67 literals in one
  (b) sparse     text | delta | entropy8 | text, 106 254 bytes, dictionary 64 KiB (smaller than the input): 13 341 positions
                 leave through DP_SEEN_EXIT (no window: the literal after match-rich windows), 2 918 windows, 59 longer than 64
                 nodes, five with more than 120 literals (most: 1 381 of 1 396 nodes)
  (c) mutations  a 4 000-byte block of text repeated with a byte replaced, dropped or inserted every 5..40 bytes, 200 000 bytes,
                 dictionary 256 KiB: in windows 51 rep0len1 packets and 1 277 / 1 113 / 707 / 540 rep matches of index 0 / 1 / 2 / 3
  (d) chunks     200 000 bytes of exe, dictionary 1 MiB: 14 windows longer than 64 nodes (longest 97): a second chunk that
                 starts from the state and context the first one left
  (e) literals   text | entropy8 | text | delta, 230 000 bytes, dictionary 64 KiB: five windows with more than 120 literals (most:
                 2 042 literals in a window of 2 045 nodes, 32 chunks): more literals than the literal ring takes (120) unless
                 the tree wavefront keeps up -- when it does not, the chunk goes one packet at a time
"""
import os

import pytest

import cases
import soak_gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mutated(seed, block, total, lo, hi):
    """a block of text over and over, every copy with its own single-byte edits lo..hi bytes apart: 70 % a byte replaced, 15 % a
    byte dropped, 15 % a byte inserted (a generator of its own: the same bytes under every Python)"""
    state = [seed * 2654435761 % (1 << 32) or 1]

    def rnd(n):
        state[0] = (state[0] * 1664525 + 1013904223) % (1 << 32)
        return (state[0] >> 8) % n

    base = cases.build([["text", seed, 0, block]])
    out = bytearray()
    while len(out) < total:
        i = 0
        while i < len(base):
            n = lo + rnd(hi - lo + 1)
            out += base[i:i + n]
            i += n
            r = rnd(100)
            if r < 70 and i < len(base):
                out.append((base[i] + 1 + rnd(255)) & 0xFF)
                i += 1
            elif r < 85:
                i += 1
            else:
                out.append(rnd(256))
    return bytes(out[:total])


# name -> (input, dictionary)
CASES = {
    "a_text": (lambda: cases.build([["text", 31, 0, 200000]]), 1 << 20),
    "b_sparse": (lambda: cases.build([["text", 41, 0, 30000], ["delta", 3317694466, 65229574, 26254], ["entropy8", 33, 0, 30000],
                                      ["text", 41, 30000, 20000]]), 64 << 10),
    "c_mutations": (lambda: mutated(35, 4000, 200000, 5, 40), 256 << 10),
    "d_chunks": (lambda: cases.build([["exe", 36, 0, 200000]]), 1 << 20),
    "e_literals": (lambda: cases.build([["text", 34, 0, 60000], ["entropy8", 33, 0, 70000], ["text", 34, 60000, 30000],
                                        ["delta", 32, 0, 70000]]), 64 << 10),
}


def streams_of(name):
    data = CASES[name][0]()
    assert len(data) <= 256 << 10
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
