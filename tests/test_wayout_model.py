"""CPU tier: tests/model/wayout_model.c -- the lane arrangement the level-3 kernels give the way out's flag coding
(d6_chunk_lanes, csc_amd/csrc/csc_kernels_dp4.inc: 64 packets of a window at a time, packet r in lane r, same-cell decisions
chained in packet order) against the packets coded one after the other (d6_literal / d6_rep0len1 / d6_rep_match / d6_match).
The model compares P[], every queue entry and its position, the tree records and their order, and the state / context /
queue head / statistics behind the list, and stops at the first difference; this test builds it, runs it on seeded random
lists and the adversarial ones (all literals, literal / rep0len1, the four rep indices, every length class, every distance
class, lists of 63 / 64 / 65 / 128 packets) and checks from its counters that the paths the arrangement rests on were walked."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "model", "wayout_model.c")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wayout") / "wayout_model")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    return exe


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "WAYOUT_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def num(text, pattern):
    m = re.search(pattern, text)
    assert m, (pattern, text)
    return [int(g) for g in m.groups()]


def test_lanes_equal_serial(model):
    out = run(model)
    lists, packets, chunks, carried = num(out, r"lists (\d+) packets (\d+) chunks (\d+) chunks entered with a carried state (\d+)")
    assert lists >= 4000 and packets > 100000 and chunks > lists
    assert carried > 100                                                  # a second chunk that starts from the state the first one left
    longest, ge8, mixed, steps = num(out, r"chains longest (\d+) of length >= 8 (\d+) with both bits (\d+) chain steps (\d+)")
    assert longest == 64                                                  # all literals: one state, one cell, a whole chunk in one chain
    assert ge8 > 100 and mixed > 1000 and steps > 10000
    kinds = num(out, r"kinds literal (\d+) match (\d+) rep0len1 (\d+) rep (\d+) rep indices (\d+) (\d+) (\d+) (\d+)")
    assert min(kinds) > 1000, kinds
    classes = num(out, r"length classes (\d+) (\d+) (\d+) direct pieces (\d+) (\d+) (\d+)")
    assert min(classes) > 100, classes                                    # d6_len_slots 4 / 5 / 9; direct bits in 0, 1 and 2 pieces
    extra = {int(x) for x in re.search(r"extra bits((?: \d+)+)", out).group(1).split()}
    assert {0, 1, 3, 4, 5, 6, 19, 20, 21, 22} <= extra, extra             # both sides of 0, 4, 5, 20 and 21


@pytest.mark.parametrize("seed", [1, 77, 123456789])
def test_other_seeds(model, seed):
    run(model, str(seed), "1500")
