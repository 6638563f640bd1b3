"""Inputs of tests/test_gpu_trees.py and the CPU-side counter (tests/model/trees_model.c) that says what they make the level-3 parser
hand to the tree wavefront.  tests/test_trees_model.py holds the counts against the conditions each case is there for."""
import ctypes as C
import os
import subprocess

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SO = os.path.join(ROOT, "tests", "model", "libtreesmodel.so")

# TrCounts of tests/model/trees_model.c, in its order
FIELDS = ("windows exit_limit exit_lit exit_match exit_match_long no_window exit_lit_end0 lit_records match_records queue_entries most_lit most_match "
          "wo_match_gt8 wo_lit_gt8 wo_lit_gt16 wo_gt64_nodes same_len_cells same_slot_cells same_low_cells runs8_all_classes dir0 dir1 dir2 "
          "lring_wraps_inside mring_wraps_inside pair_repeats_across_halves pair_repeats_in_eight exit_lit_same_row exit_lit_same_pair "
          "exit_lit_on_ring_edge exit_lit_after_gt64 no_window_runs_ge8 refreshes refreshes_early_after_records").split()


def rng(seed):
    """a generator of its own: the same bytes under every Python"""
    state = [seed * 2654435761 % (1 << 32) or 1]

    def rnd(n):
        state[0] = (state[0] * 1664525 + 1013904223) % (1 << 32)
        return (state[0] >> 8) % n
    return rnd


def mutated(seed, block, total, lo, hi, kind="text"):
    """a block over and over, every copy with its own single-byte edits lo..hi bytes apart: 70 % a byte replaced, 15 % a byte dropped,
    15 % a byte inserted (the shape of tests/test_gpu_wayout.py's generator)"""
    rnd = rng(seed)
    base = cases.build([[kind, seed, 0, block]])
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


def spliced(seed, total, far_gap):
    """Distance classes side by side.  A 2 000-byte source block, `far_gap` bytes of a period-251 filler (cheap to parse), then pieces of
    four to eleven bytes taken in turn from the far source block, from 40..3 000 bytes back, from 4..32 bytes back and from 1..3 bytes
    back, a fresh byte behind every eighth piece: neighbouring match packets with more than 20, 5..20, 1..4 and no extra distance bits.
    More than 20 extra bits is a distance beyond 2 MiB, so this input alone is longer than that."""
    rnd = rng(seed)
    src = cases.build([["text", seed, 0, 2000]])
    out = bytearray(src)
    filler = bytes((i * 7 + 3) & 0xFF for i in range(251))
    while len(out) < len(src) + far_gap:
        out += filler
    del out[len(src) + far_gap:]
    k = 0
    while len(out) < total:
        n = 4 + rnd(8)
        which = k & 3
        if which == 0:
            at = rnd(len(src) - n)
        elif which == 1:
            at = len(out) - 40 - rnd(2960)
        elif which == 2:
            at = len(out) - 4 - rnd(29)
        else:
            at = len(out) - 1 - rnd(3)
        for j in range(n):
            out.append(out[at + j])
        k += 1
        if k % 8 == 0:
            out.append(rnd(256))
    return bytes(out[:total])


def shuffled(seed, block, total, nmin, nspan):
    """a block of text, then pieces of nmin .. nmin + nspan - 1 bytes copied from anywhere in the last `block` bytes, nothing between them:
    match after match of a few lengths in one or two distance slots, and -- where a piece is cheaper as literals -- long stretches of
    literals inside a window whose (context, symbol) pairs come back"""
    rnd = rng(seed)
    out = bytearray(cases.build([["text", seed, 0, block]]))
    while len(out) < total:
        n = nmin + rnd(nspan)
        at = len(out) - block + rnd(block - n)
        for j in range(n):
            out.append(out[at + j])
    return bytes(out[:total])


FAR = (2 << 20) + 40000
# name -> (input, dictionary)
CASES = {
    "a_short_blocks": (lambda: mutated(51, 200, 60000, 4, 10) + shuffled(51, 1000, 60000, 4, 6), 256 << 10),
    "b_distance_classes": (lambda: spliced(52, FAR + 2000 + 60000, FAR), 4 << 20),
    "c_ring_wraps": (lambda: cases.build([["text", 53, 0, 60000]]) + mutated(53, 1500, 60000, 4, 20), 256 << 10),
    "d_literal_runs": (lambda: shuffled(54, 300, 100000, 3, 6), 256 << 10),
    "e_small_dictionary": (lambda: cases.build([["text", 56, 0, 50000], ["entropy8", 57, 0, 60000], ["delta", 58, 0, 50000], ["text", 56, 50000, 40000],
                                                ["entropy8", 59, 0, 40000]]), 64 << 10),
    "f_long_stream": (lambda: cases.build([["text", 60, 0, 256 << 10]]), 1 << 20),
}


def streams_of(name):
    """the case's input, the input rotated by a third and its first 60 000 bytes"""
    data = CASES[name][0]()
    return [data, data[len(data) // 3:] + data[:len(data) // 3], data[:60000]]


def build_model():
    src = [os.path.join(ROOT, "tests", "model", "trees_model.c"), os.path.join(ROOT, "oracle", "orc_decoder.c"), os.path.join(ROOT, "oracle", "zalloc.c")]
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wl,-Bsymbolic", "-o", MODEL_SO] + src + ["-lm"], check=True)
    return MODEL_SO


def counts(mod, data, dict_size, alloc):
    """-> (the model's stream, its counters by name) for one level-3 encode of `data`"""
    mod.lib.trees_model_reset()
    rc, s = mod.encode(data, 3, dict_size, alloc=alloc)
    assert rc == 0
    buf = (C.c_uint64 * 64)()
    n = mod.lib.trees_model_counts(buf, 64)
    assert n == len(FIELDS), (n, len(FIELDS))
    return s, dict(zip(FIELDS, list(buf)[:n]))
