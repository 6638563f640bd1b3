#!/usr/bin/env python3
"""Records what the REFERENCE's Foward_Dict makes of every case of tests/dict_wide_cases.py into tests/golden/dict_wide.json,
through the probe of oracle/ref_probe.cpp (as tools/make_golden_filter_edges.py does).  Needs oracle/_ref.  Per case: the
sha-256 of the buffer afterwards and the return value.

  python tools/make_golden_dict_wide.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dict_wide_cases as W  # noqa: E402
import filter_cases as F  # noqa: E402
from csc_amd.capi import CscLib  # noqa: E402

orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
ref = CscLib(os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so"))
probes = F.Probes(ref.lib, "ref")
gold = {}
for name, data in W.cases(F.words(orc.lib)).items():
    ok, out = probes.run("forward_dict", data)
    gold[name] = {"dict_ok": int(ok), "sha256": F.digest(out)}
    if name.startswith("reject/"):                          # the lower of the pair is accepted, the upper rejected and untouched
        assert ok == (1 if name.endswith("/at") else 0), (name, ok)
        assert ok or out == data, name
    elif not name.startswith("text/"):
        assert ok == 1, (name, ok)
with open(os.path.join(ROOT, "tests", "golden", "dict_wide.json"), "w") as f:
    json.dump(gold, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(gold), "cases")
