#!/usr/bin/env python3
"""Records what the device archive's calls report for the scenario of tests/archive_stats_cases.py into
tests/golden/archive_stats.json (tests/test_gpu_archive_stats.py holds the library to it).  Needs a GPU and the built library.
Run it on the commit whose counters are to be kept, BEFORE the change that must not move them.  The scenario runs twice: a field
that differs between the two runs is named and the record is not written.

  python tools/make_golden_archive_stats.py [output path]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import archive_stats_cases as S  # noqa: E402
from csc_amd import csa  # noqa: E402
from csc_amd.capi import CscLib  # noqa: E402

orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
orc.lib.orc_zero_alloc.restype = C.c_void_p
zalloc = orc.lib.orc_zero_alloc()


def enc(data, dict_size, level):
    rc, s = orc.encode(data, props=orc.props_init(dict_size, level), alloc=zalloc)
    assert rc == 0
    return s


def dec(stream):
    rc, raw = orc.decode(stream, alloc=zalloc)
    assert rc == 0
    return raw


csa.lib()
runs = []
for _ in range(2):
    t0 = time.time()
    secs = {}
    runs.append(json.loads(json.dumps(S.record(csa, (enc, dec), secs))))
    print(f"{len(runs[-1])} calls in {time.time() - t0:.2f} s, {sum(s for s, _ in secs.values()):.2f} s of them inside the library")
moved = [(k, f) for k in runs[0] for f in runs[0][k]["stats"] if runs[0][k]["stats"][f] != runs[1][k]["stats"].get(f)]
moved += [(k, f) for k in runs[0] for f in ("rc", "diffs", "adler32") if runs[0][k].get(f) != runs[1][k].get(f)]
if moved or runs[0] != runs[1]:
    sys.exit(f"not reproducible between two runs: {moved}")
bad = [k for k, r in runs[0].items() if r["rc"] != 0]
if bad:
    sys.exit(f"calls that failed: {bad}")
with open(sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN, "w") as f:
    json.dump(runs[0], f, indent=0, sort_keys=True)
    f.write("\n")
