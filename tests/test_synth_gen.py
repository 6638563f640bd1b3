"""CPU tier for the stream synthesizer: the seeded script generator (tests/synth_gen.py) is deterministic, its coverage
table is complete for the fixed seeds, and every synthesized stream decodes to exactly the predicted (rc, bytes) through the
oracle's decoder, through the reference when oracle/_ref is built, and matches the reference's recorded answer
(tests/golden/synth.json, written by tools/make_golden_synth.py from oracle/_ref) in both cases.

Ragged Read sizes: the reference's block reader takes a short Read for the end of the stream (MemIO::ReadBlock), so with
max_read below a stream's largest block the defined answer is a read failure after the runs decoded so far, not the
prediction; the reference's answer at 257, 1000 and 65 537 is recorded in the golden line and both decoders must give it, with
or without oracle/_ref.  Where max_read is above every block (65 537 at the default geometry) it must be the prediction too."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import filter_cases as F
import synth_gen as G
from csc_amd.capi import CscLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "synth.json")
REF = os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so")
FAMILY_SEEDS = [(f, s) for f in G.FAMILIES for s in G.FAMILIES[f]]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {g["id"]: g for g in json.load(f)}


def _cases(orc, family, seed, _memo={}):
    if (family, seed) not in _memo:
        _memo[family, seed] = G.cases(orc.lib, family, seed)
    return _memo[family, seed]


def test_generator_is_deterministic(orc):
    for family, seed in FAMILY_SEEDS:
        a, b = G.cases(orc.lib, family, seed), G.cases(orc.lib, family, seed)
        assert [c["meta"] for c in a] == [c["meta"] for c in b]
        for x, y in zip(a, b):
            assert np.array_equal(x["script"], y["script"]) and x["out"] == y["out"] and x["cover"] == y["cover"], G.describe(x)


def complete():
    """What the fixed seeds must cover, cell by cell."""
    want = set()
    for state in range(64):
        for kind in range(4):                                   # literal, match, one-byte rep, rep match: out of every state
            want.add(("state", state, kind))                    # (the end-of-run marker is counted apart, as ("end_run", state))
            want.add(("rep", state, kind))                      # rep index 0..3 out of every state
    for ctx in range(7):                                        # length context: coded length 0, 1, 2, 3, 4, 5, >= 6
        top = 7 if ctx == 0 else 15 if ctx <= 2 else 21         # slots the context can code (3 / 4 / 5 bits); 21: a 2 MiB window
        for slot in range(top + 1):
            want.add(("dist", ctx, slot, "lo"))                 # dist_table_[slot] + 0
            if slot >= 3:                                       # (slots 0..2 hold one distance)
                want.add(("dist", ctx, slot, "lo1"))            # + 1
                if not (ctx == 0 and slot == 7):                # length 2 at coded distance 64 is the end-of-run marker
                    want.add(("dist", ctx, slot, "hi"))         # dist_table_[slot + 1] - 1
    lengths = [str(n) for n in list(range(2, 18)) + list(range(142, 147)) + list(range(285, 289)) + list(range(8191, 8195))] + ["65536"]
    for kind in ("match", "rep"):
        for n in lengths + ["1MiB", "to_end"]:
            want.add(("len", kind, n))
        for n in lengths:
            for d in (1, 2, 3, 63, 64, 65):
                if kind == "rep" or d <= G.max_dist(int(n)):
                    want.add(("overlap", kind, n, d))
            for rel in (-1, 0, 1):                              # distance = length - 1, length, length + 1
                d = int(n) + rel
                if d >= 1 and d not in (1, 2, 3, 63, 64, 65) and (kind == "rep" or d <= G.max_dist(int(n))):
                    want.add(("overlap", kind, n, rel))
    for d in (1, 2, 3, 63, 64, 65):
        want.add(("overlap", "match", "1MiB", d))
    for kind in ("match", "rep"):                               # a long copy from written bytes at distance >= length
        want |= {("far_source", kind, "65536"), ("far_source", kind, "1MiB")}
    for ctx in range(3, 7):                                     # slot 22's first two distances still fit the 2 MiB + 4 KiB window
        want |= {("dist", ctx, 22, "lo"), ("dist", ctx, 22, "lo1")}
    for e in ("wrap", "wrap_inside_run", "source_never_written", "src_ends_at_wnd", "dst_ends_at_wnd", "packet_ends_at_limit",
              "run_of_exactly_raw_blocksize", "zero_byte_run", "rep_distance_zero", "rep1_first_packet", "rep1_at_curpos_eq_rep0",
              "rep1_at_curpos_eq_rep0_after_wrap", "largest_distance", "largest_distance_after_wrap", "rle_run_at_1", "rle_run_clipped",
              "long_chain", "rle_run_above_undo_cap"):
        want.add(("edge", e))
    for name in ("limit_match", "limit_rep", "limit_lit", "limit_rep1"):
        want.add(("edge", "packet_ends_at_limit", name))
    for typ in (G.DT_BAD, G.DT_ENTROPY, G.DT_DLT):
        want.add(("edge", "size_field_eq_max", typ))
    for chn in (1, 2, 3, 4, 8):
        want.add(("edge", "delta_inverse", chn))
    for typ in (G.DT_NORMAL, G.DT_ENGTXT, G.DT_EXE, G.DT_BAD, G.DT_ENTROPY, 0x10, 0x11, 0x12, 0x13, 0x14):
        want.add(("block", typ))
    want |= {("restart", 0), ("restart", 1), ("edge", "rc_block_full"), ("edge", "bc_block_full")}
    for name in G.REFUSED:
        want.add(("refused", name))
    for g in G.GEOMETRY:
        want.add(("geometry",) + g)
    # family `filters`, DT_ENGTXT runs: one cell for each thing its list promises
    for n in G.TXT_SIZES:
        want.add(("flt", "txt_size", n))
    for follow in ("hi", "lo"):                                 # the byte behind the run: >= 0x82, < 0x82
        for length in G.RUN254:
            for start in G.RUN254_STARTS:
                want.add(("flt", "run254", length, start, follow))
        want.add(("flt", "whole_step_of_254", follow))          # the carry's lead == 64 branch
    for where in ("serial", "tail"):                            # run of <= 66 bytes / the serial tail behind vector steps
        want |= {("flt", "last_254", where), ("flt", "last_but_one_254_hi", where)}
    for name in G.TAIL_BOUNDARY:
        want.add(("flt", "tail_boundary", name))
    for b in (0x82, 0xFB, 0xFC, 0xFD, 0xFF):
        want.add(("flt", "byte", b))
    want.add(("flt", "pair_254_254"))
    for wl in (2, 3, 4):
        for room in (1, 2, 3):
            want.add(("flt", "clip", wl, room))
    for r in range(4):
        want.add(("flt", "all_four_letter", r))
    for f in ("n", "0", "1MiB"):
        want.add(("flt", "size_field", f))
    for name in F.e89_cases():                                  # DT_EXE runs: the forward E89 case list as the filtered side
        want.add(("flt", "exe", name))
    return want


CASES = {"walk": 12, "lengths": 64, "distances": 4, "edges": 22, "blocks": 12, "geometry": 6, "refused": 36, "long_chain": 1, "long_rle": 1,
         "filters": 12}


def test_coverage_table_is_complete(orc):
    cs = [c for f, s in FAMILY_SEEDS for c in _cases(orc, f, s)]
    count = {f: sum(c["meta"]["family"] == f for c in cs) for f in G.FAMILIES}
    assert count == CASES, "the families' fixed seeds and case counts changed"
    for name in G.REFUSED:                                      # every refused check once a seed
        hits = [c for c in cs if ("refused", name) in c["cover"]]
        assert len(hits) == 2, name
    cov = G.coverage(cs)
    for c in cs:                                                # two cells are properties of the coded stream
        if c["meta"]["family"] == "blocks":
            for is_rc, _, full in G.blocks_of(G.stream(orc.lib, c)):
                if full:
                    cov.add(("edge", "rc_block_full" if is_rc else "bc_block_full"))
    missing = sorted(complete() - cov, key=str)
    assert not missing, f"{len(missing)} cells uncovered by the fixed seeds: {missing[:40]}"


def _check(lib, za, st, case, who, biggest, line):
    got = lib.decode(st, alloc=za)
    assert got[0] == case["rc"] and got[1] == case["out"], \
        f"{who}: rc {got[0]} len {len(got[1])}, predicted rc {case['rc']} len {len(case['out'])}; {G.describe(case)}"
    for mr in G.short_reads(case):
        got = lib.decode(st, alloc=za, max_read=mr)
        assert G.digest(*got) == line["short"][str(mr)], \
            f"{who} max_read {mr}: rc {got[0]} len {len(got[1])}, the reference recorded {line['short'][str(mr)]}; {G.describe(case)}"
        if mr >= biggest:                                       # no block is cut short: the prediction itself
            assert got[0] == case["rc"] and got[1] == case["out"], f"{who} max_read {mr} differs from the prediction; {G.describe(case)}"


@pytest.mark.parametrize("family,seed", FAMILY_SEEDS)
def test_streams_decode_as_predicted(orc, zalloc, golden, family, seed):
    ref = CscLib(REF) if os.path.exists(REF) else None
    for case in _cases(orc, family, seed):
        st = G.stream(orc.lib, case)
        biggest = max(n for _, n, _ in G.blocks_of(st))
        line = golden.get(G.case_id(case))
        assert line is not None, f"no golden line (run tools/make_golden_synth.py); {G.describe(case)}"
        mine = dict(G.golden_line(case, st, case["rc"], case["out"]), short=line["short"])
        assert mine == line, f"the reference's recorded answer {line} differs from {mine}; {G.describe(case)}"
        _check(orc, zalloc, st, case, "oracle", biggest, line)
        if ref is not None:
            _check(ref, zalloc, st, case, "reference", biggest, line)


def test_golden_has_no_stale_lines(orc, golden):
    ids = {G.case_id(c) for f, s in FAMILY_SEEDS for c in _cases(orc, f, s)}
    assert set(golden) == ids


# ---- family `filters`: the prediction's own footing, and what its runs are sensitive to -----------------------------------

@pytest.fixture(scope="module")
def txt_runs(orc):
    words = F.words(orc.lib)
    return words, [(name, src, out) for name, runs in G.txt_runs(words).items() for src, out, _ in runs]


def test_filter_runs_stay_inside_their_buffers_and_invert_as_restated(orc, txt_runs):
    """the condition of the header's kept-out list: Inverse_Dict reads no source index at or behind a run's size; and the
    restated inverses are the oracle's (and the reference's, where oracle/_ref is built) on every run of the family"""
    words, runs = txt_runs
    probes = [F.Probes(orc.lib, "orc")] + ([F.Probes(CscLib(REF).lib, "ref")] if os.path.exists(REF) else [])
    assert len(runs) > 80
    for name, src, out in runs:
        got, hi = G.inverse_dict(src, words)
        assert got == out and hi < len(src), (name, len(src), hi)
        assert G.inverse_dict_steps(src, words) == out, (name, len(src))
        for p in probes:
            assert p.run("inverse_dict", src)[1] == out, (name, len(src))
    for name, runs_ in G.exe_runs().items():
        for coded, plain, _ in runs_:
            for p in probes:
                assert p.run("inverse_e89", coded)[1] == plain, name
                assert p.run("forward_e89", plain)[1] == coded, name


@pytest.mark.parametrize("mistake,witness", [
    ("parity_not_carried", "txt_254_lo"),
    ("run_of_64_even", "txt_254_hi"),
    ("guard_dropped", "txt_tail"),
    ("not_clipped", "txt_clip"),
    ("max_symbol_fd", "txt_symbols"),
])
def test_filter_runs_catch_a_planted_mistake(txt_runs, mistake, witness):
    """Inverse_Dict restated the way a 64-lane step computes it, with one mistake planted: a run of the named case differs"""
    words, runs = txt_runs
    hits = {name for name, src, out in runs if G.inverse_dict_steps(src, words, mistake) != out}
    assert witness in hits, f"{mistake}: caught by {sorted(hits)}"
