#!/usr/bin/env python3
"""Records what the REFERENCE makes of every chunk-walk and duplicate-check case (tests/walk_cases.py) into
tests/golden/walk_edges.json.  Needs oracle/_ref; the zero-filling allocator as in tools/make_golden.py.  Per case: stream
size and SHA-256, the reference decoder's (rc, digest) for that stream, the whole stream in hex where it is <= 1 200 bytes.

No case had to be left out for memory the reference never wrote: what TestFind hashes past the end of a chunk belongs to
one of the last five offsets of a block, where the compare's limit is below 19 and cannot hit, and the slack behind the window
is zero under this allocator.  The loop asserts the first for every candidate the oracle's trace records.

  python tools/make_golden_walk_edges.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import soak_gen  # noqa: E402
import walk_cases as W  # noqa: E402
from csc_amd.capi import CscLib  # noqa: E402

orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
ref = CscLib(os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so"))
orc.lib.orc_zero_alloc.restype = C.c_void_p
za = orc.lib.orc_zero_alloc()
gold = {}
for case in W.all_cases(orc.lib):
    rc, s, rcd, back = soak_gen.check_one(ref, za, case.spec, case.data)
    assert rc == 0, (case.name, rc)
    _, _, tr = W.traced_encode(orc, za, case)
    for c in tr.cands:                                      # a compare that could reach bytes behind the block has no room to hit
        assert c[W.C_I] + c[W.C_LIMIT] == next(b[W.B_SIZE] for b in tr.blocks if b[:2] == c[:2]), (case.name, c)
        assert not (c[W.C_LIMIT] <= 18 and c[W.C_HIT]), (case.name, c)
    gold[case.name] = W.golden_entry(s, (rcd, back))
with open(os.path.join(ROOT, "tests", "golden", "walk_edges.json"), "w") as f:
    json.dump(gold, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(gold), "cases")
