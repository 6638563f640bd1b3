#!/usr/bin/env python3
"""Record what the REFERENCE's command-line tool on the REFERENCE's libcsc (oracle/_ref/csc_ref, built by oracle/Makefile with the
zero-filling heap of oracle/zero_heap.cpp) writes and prints for the cases of tests/dropin_cases.py -> tests/golden/dropin_cli.json:
per case the argv, the input spec, size and SHA-256 of the stream, the whole stderr of `c` (the "Estimated memory usage" line and
every Progress record), and the whole stderr and the output digest of `d` on that stream.  Data only.

  python tools/make_golden_dropin.py
"""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases, dropin_cases as dc

REF = os.path.join(ROOT, "oracle", "_ref", "csc_ref")


def record(case):
    """run `csc_ref c` then `csc_ref d` for the case in a fresh directory -> the golden entry (and the stream, for the tests)"""
    spec = dc.CLI_CASES[case][0]
    data = cases.build(spec)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, dc.IN_NAME), "wb") as f:
            f.write(data)
        c = subprocess.run([REF] + dc.encode_argv(case), cwd=td, capture_output=True, check=True)
        stream = open(os.path.join(td, dc.OUT_NAME), "rb").read()
        d = subprocess.run([REF] + dc.decode_argv(), cwd=td, capture_output=True, check=True)
        back = open(os.path.join(td, dc.BACK_NAME), "rb").read()
    ent = {"argv": dc.encode_argv(case), "spec": spec, "input_size": len(data), "stream_size": len(stream), "stream_sha256": cases.digest(stream),
           "encode_stderr": c.stderr.decode("latin-1"), "decode_argv": dc.decode_argv(), "decode_stderr": d.stderr.decode("latin-1"),
           "decoded_size": len(back), "decoded_sha256": cases.digest(back)}
    return ent, stream


if __name__ == "__main__":
    out = {}
    for case in dc.CLI_CASES:
        out[case], stream = record(case)
        assert record(case) == (out[case], stream), case          # the checker is deterministic
        print(case, out[case]["input_size"], "->", out[case]["stream_size"], repr(out[case]["encode_stderr"][-40:]), flush=True)
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "dropin_cli.json"), "w"), indent=1)
