"""Records the REFERENCE decoder's answer for every synthesized stream (tests/synth_gen.py) into tests/golden/synth.json:
one line a case -- sha-256 of the stream, return code, length and sha-256 of the bytes delivered.  Needs oracle/_ref.
The tests compare with these lines wherever oracle/_ref is absent, so the oracle never only agrees with itself."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import synth_gen as G  # noqa: E402
from csc_amd.capi import CscLib  # noqa: E402

orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
orc.lib.orc_zero_alloc.restype = C.c_void_p
za = orc.lib.orc_zero_alloc()
ref = CscLib(os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so"))
lines = []
for case in G.all_cases(orc.lib):
    st = G.stream(orc.lib, case)
    rc, out = ref.decode(st, alloc=za)
    line = G.golden_line(case, st, rc, out)
    # MemIO::ReadBlock takes a short Read for the end of the stream: below a block's size the answer is a read failure
    # after the runs decoded so far, which only the reference defines -- recorded, not predicted
    line["short"] = {str(mr): G.digest(*ref.decode(st, alloc=za, max_read=mr)) for mr in G.short_reads(case)}
    lines.append(line)
with open(os.path.join(ROOT, "tests", "golden", "synth.json"), "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(g, sort_keys=True) for g in lines) + "\n]\n")
print(len(lines), "lines")
