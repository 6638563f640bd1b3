"""CPU tier: tests/model/publish_model.c -- what d6_room (csc_amd/csrc/csc_kernels_dp4.inc) publishes to the coder wavefront when the spine
needs queue room: everything in front of the oldest record the tree wavefront has not counted done, and a join only where that cannot
give the room.  Spine, tree wavefront and coder are three state machines under seeded random schedules; the tree wavefront fills kept
slots at arbitrary steps and stores its count at a later one.  The model itself stops at the first violation (the coder consuming an
unfilled slot, an unfilled slot in front of a published point, `pub` moving backwards, more than kCoderQ - 64 entries outstanding, a
fallback that disagrees with the 32-bit positions, a stall); this test builds it, runs it and checks from its counters that every
situation of the slow path was reached."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "model", "publish_model.c")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("publish") / "publish_model")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    return exe


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "PUBLISH_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def num(text, pattern):
    m = re.search(pattern, text)
    assert m, (pattern, text)
    return [int(g) for g in m.groups()]


def test_publish_point(model):
    out = run(model)
    runs, entries, batches, most, joins, ring_waits = num(out, r"runs (\d+) entries (\d+) coder batches (\d+) most outstanding (\d+) joins (\d+) waits for a ring (\d+)")
    assert runs == 600 and entries > 10_000_000 and batches > 100000
    assert most == 4096 - 64                                              # the queue was filled to its limit, never beyond (the model stops beyond)
    assert joins > 1000 and ring_waits > 1000
    slow, lit_only, match_only, both, none, fallbacks, partial = num(out, r"slow path (\d+) outstanding literal only (\d+) match only (\d+) both (\d+) none (\d+) fallbacks (\d+) partial publishes (\d+)")
    assert slow == lit_only + match_only + both + none
    assert min(lit_only, match_only, both, none) > 500, (lit_only, match_only, both, none)
    assert fallbacks > 100                                                # the oldest uncoded record too far back for the room asked
    assert partial > 10000                                                # published short of the head
    wraps, stale, clamped, mean = num(out, r"wrapped in 16 bits (\d+) counts moved on before the publish (\d+) clamped (\d+) mean distance (\d+)")
    assert wraps > 100                                                    # the record's 16-bit queue position above the head's low 16 bits
    assert stale > 1000                                                   # a count stale by the time it is used: conservative only
    assert clamped == 0                                                   # (the clamp is a guard: the point itself never moves backwards)
    assert 0 < mean < 4096 - 64


@pytest.mark.parametrize("seed", [1, 77, 123456789])
def test_other_seeds(model, seed):
    run(model, str(seed), "200")
