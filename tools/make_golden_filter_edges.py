#!/usr/bin/env python3
"""Records what the REFERENCE makes of every adversarial filter and analyzer case (tests/filter_cases.py) into
tests/golden/filter_edges.json, through the probes of oracle/ref_probe.cpp.  Needs oracle/_ref.  Digests and small integers
only: a sha-256 per output, Foward_Dict's return value, the analyzer's rows, and for the counted cases the dstSize the
generator intended.

  python tools/make_golden_filter_edges.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import filter_cases as F  # noqa: E402
from csc_amd.capi import CscLib  # noqa: E402

orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
ref = CscLib(os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so"))
gold = F.golden_of(F.Probes(ref.lib, "ref"), F.all_cases(orc.lib))
for name, ent in gold.items():
    if name.startswith("dict/reject/"):                     # the lower of each pair is accepted, the upper rejected
        assert ent["dict_ok"] == (1 if name.endswith("/at") else 0), (name, ent)
    if name.startswith("dict/copyback/"):
        assert ent["dict_ok"] == 1, (name, ent)
with open(os.path.join(ROOT, "tests", "golden", "filter_edges.json"), "w") as f:
    json.dump(gold, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(gold), "cases")
