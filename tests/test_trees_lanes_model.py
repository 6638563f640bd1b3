"""CPU tier: tests/model/trees_lanes_model.c -- the lane arrangement the tree wavefront gives the match and rep packets' length and
distance trees (d6_trees, csc_amd/csrc/csc_kernels_dp4.inc: up to four records a pass, a record in 16 or 32 lanes, decisions on one cell
chained in record order through the lane d6_rec_lane computes) against the records coded one after the other in the order of
Model::EncodeMatch.  The model compares P[] and every queue entry and its position, direct-bit entries included, stops at the first
difference, and refuses a scatter in which two lanes store to one cell; this test builds it, runs it on seeded random record lists and
the constructed ones, and checks from its counters that each situation the arrangement has to get right was walked."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "model", "trees_lanes_model.c")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trees_lanes") / "trees_lanes_model")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    return exe


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "TREES_LANES_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def num(text, pattern):
    m = re.search(pattern, text)
    assert m, (pattern, text)
    return [int(g) for g in m.groups()]


def test_lanes_equal_serial(model):
    out = run(model)
    lists, records, p1, p2, p3, p4, wide, cross = num(out, r"lists (\d+) records (\d+) passes of 1 (\d+) of 2 (\d+) of 3 (\d+) of 4 (\d+) wide (\d+) crossing the ring's end (\d+)")
    assert lists >= 4000 and records > 100000
    assert min(p1, p2, p3, p4) > 1000, (p1, p2, p3, p4)                   # passes of 1, 2, 3 and 4 records
    assert wide > 1000                                                    # a record of more than 14 decisions: 32 lanes a record
    assert cross > 100                                                    # a pass that crosses ring slot 63 -> 0
    r0, r1, r2, r3, rounds, left = num(out, r"on their cell 0 (\d+) 1 (\d+) 2 (\d+) 3 (\d+) chain rounds (\d+) stores left to a later record (\d+)")
    assert min(r0, r1, r2, r3) > 10000 and rounds > 10000 and left > 10000
    four, full, three, between = num(out, r"four of a kind (\d+) chained at every level (\d+) shared distance tree at three offsets (\d+) rep between matches (\d+)")
    assert four >= 32 and full == four                                    # same length, slot and low nibble: every decision of the fourth record third in its chain
    assert three >= 36                                                    # lengths 6-7, 8-15 and >= 16 side by side: one distance tree from lanes 4, 5 and 9
    assert between > 100                                                  # rep records between match records
    e0, e1, e2, e3, d0, d1, d2, c0, c1, c2 = num(out, r"extra bits none (\d+) 1\.\.4 (\d+) 5\.\.20 (\d+) above 20 (\d+) direct entries (\d+) (\d+) (\d+) length classes (\d+) (\d+) (\d+)")
    assert min(e0, e1, e2, e3) > 1000 and min(d0, d1, d2) > 1000          # direct-bit entries: none, one, two
    assert min(c0, c1, c2) > 1000                                         # d6_len_slots 4 / 5 / 9
    first, last, mid = num(out, r"nine-slot record first (\d+) last (\d+) in the middle (\d+) of a pass")
    assert min(first, last, mid) > 100, (first, last, mid)


@pytest.mark.parametrize("seed", [1, 77, 123456789])
def test_other_seeds(model, seed):
    run(model, str(seed), "1500")
