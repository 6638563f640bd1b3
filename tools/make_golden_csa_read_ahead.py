#!/usr/bin/env python3
"""Record what the REFERENCE ARCHIVER (oracle/_ref/csarc_ref, built by oracle/Makefile) writes for the multi-chunk tree of
tests/csa_cases.py (READ_AHEAD_FILES, READ_AHEAD_ARGV): size and SHA-256 of the archive -> tests/golden/csa_read_ahead.json.

  python tools/make_golden_csa_read_ahead.py
"""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases, csa_cases

REF = os.path.join(ROOT, "oracle", "_ref", "csarc_ref")
with tempfile.TemporaryDirectory() as td:
    content = csa_cases.make_read_ahead_tree(td)
    subprocess.run([REF] + csa_cases.READ_AHEAD_ARGV, cwd=td, check=True, capture_output=True)
    arc = open(os.path.join(td, "ref0.csa"), "rb").read()
out = {"what": "csarc_ref " + " ".join(csa_cases.READ_AHEAD_ARGV) + " over tests/csa_cases.py READ_AHEAD_FILES (tools/make_golden_csa_read_ahead.py)",
       "raw_bytes": sum(len(v) for v in content.values()), "archive_size": len(arc), "archive_sha256": cases.digest(arc)}
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "csa_read_ahead.json"), "w"), indent=1)
print(out)
