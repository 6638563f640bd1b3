#!/usr/bin/env python3
"""Evidence run (python tools/gpu_soak.py [seconds] [seed]): random single-stream cases from tests/soak_gen.py (single_case: corpus
kind or splice, offset, size 0 .. 3 MiB weighted to powers of two +- 64, level 1..5 or custom props from every dispatch row, dictionaries
smaller than the input, filters off, ragged Read sizes) through the HIP library, every stream compared byte for byte with the reference
build's (oracle/_ref/libcsc_ref.so, or the oracle where that is absent) and decoded back on the GPU -- the decoded bytes compared with the
reference DECODER's output for the same stream.  tests/test_gpu_soak.py runs the same generator on fixed seeds and case counts.
Prints one line per case and a summary; exit code 1 on the first difference (the case's spec is in its line: the run is reproducible by seed)."""
import hashlib, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa
import csc_amd
import soak_gen

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20261004
rng = random.Random(seed)
prod = csc_amd.load()
chk, za, is_ref = soak_gen.checker()
print(f"checker: {'reference build (oracle/_ref)' if is_ref else 'oracle'}; seed {seed}; budget {budget:.0f} s", flush=True)

t_start = time.time()
n_cases = n_bytes = n_ref_rt = 0
by_row = {}
while time.time() - t_start < budget:
    spec = soak_gen.single_case(rng)
    data = soak_gen.build_input(spec)
    rc, s = prod.encode(data, props=soak_gen.props_of(prod, spec), max_read=spec["max_read"])
    rc2, want, rcr, ref_back = soak_gen.check_one(chk, za, spec, data)
    # the decoder's parity is with the REFERENCE decoder on the same stream (which, rarely, does not give the input back -- tests/golden/ref_roundtrip_hazard.json --:
    # such cases are counted, and the device decoder must reproduce them byte for byte)
    rcd, back = prod.decode(s, max_read=spec["dec_max_read"]) if rc == 0 else (rc, b"")
    ok = (rc, s) == (rc2, want) and (rcd, back) == (rcr, ref_back)
    note = ""
    if ok and back != data:
        n_ref_rt += 1
        note = " [reference round trip != input, reproduced]"
    n_cases += 1; n_bytes += len(data)
    by_row[spec["row"]] = by_row.get(spec["row"], 0) + 1
    print(f"{soak_gen.describe(seed, n_cases - 1, spec)} -> {len(s)} B sha {hashlib.sha256(s).hexdigest()[:10]} "
          f"{'OK' if ok else 'DIFFERS rc=%d/%d dec=%d' % (rc, rc2, rcd)}{note}", flush=True)
    if not ok:
        print("FAILED", flush=True)
        sys.exit(1)
print(f"ALL OK: {n_cases} cases ({n_ref_rt} of them streams the reference's own decoder does not turn back into the input: reproduced byte for byte), {n_bytes} input bytes, by row {dict(sorted(by_row.items()))}, {time.time() - t_start:.0f} s; library sha256[:16] {hashlib.sha256(open(os.path.join(ROOT, 'csc_amd', 'libcsc_mi355x.so'), 'rb').read()).hexdigest()[:16]}")
