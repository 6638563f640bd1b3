#!/usr/bin/env python3
"""Record what the REFERENCE does in the cases of tests/test_oracle_vs_ref.py, so that those tests hold the oracle to it without a
reference build: every stream of the (case, level) grid with what the reference's decoder makes of it, the stale flush byte under a
zeroing and a 0xAA-filling allocator, the write / read error codes, and what the reference's decoder returns for
25 one-bit corruptions and three truncations of a level-3 stream (the same seeded mutations the test makes).
Generated with oracle/_ref (the reference's own sources, built by oracle/Makefile) and oracle/liborc.so (the allocators);
writes tests/golden/oracle_vs_ref.json."""
import ctypes as C, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases
from csc_amd.capi import BytesReader, BytesWriter, CscLib

NAMES = ["text_300k", "exe_300k", "mix_types", "dup_blocks", "window_wrap_32k", "short_reads_511"]
LEVELS = [1, 2, 3, 4, 5]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def decoded(res):
    rc, out = res
    return {"rc": rc, "bytes": len(out), "sha256": sha(out)}


def main():
    ref = CscLib(os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so"))
    o = C.CDLL(os.path.join(ROOT, "oracle", "liborc.so"))
    o.orc_zero_alloc.restype = C.c_void_p
    o.orc_aa_alloc.restype = C.c_void_p
    za, aa = o.orc_zero_alloc(), o.orc_aa_alloc()
    g = {"what": "the reference (oracle/_ref, zeroing allocator unless named) in the cases of tests/test_oracle_vs_ref.py; tools/make_golden_vs_ref.py",
         "streams": {}}
    for name in NAMES:
        spec, dict_size, clamp, max_read = cases.STREAM_CASES[name]
        data = cases.build(spec)
        for level in LEVELS:
            rc, s = ref.encode(data, level, dict_size, alloc=za, clamp_dict=clamp, max_read=max_read)
            g["streams"][f"{name}/m{level}"] = {"input_sha256": sha(data), "rc": rc, "stream_bytes": len(s), "stream_sha256": sha(s),
                                                "decoded": decoded(ref.decode(s, alloc=za))}
    data = cases.build([["text", 3, 0, 30000]])
    z_ref, a_ref = ref.encode(data, 3, 1 << 20, alloc=za)[1], ref.encode(data, 3, 1 << 20, alloc=aa)[1]
    assert len(z_ref) == len(a_ref)
    g["stale_flush"] = {"input_sha256": sha(data), "zero_alloc_sha256": sha(z_ref), "aa_alloc_sha256": sha(a_ref), "stream_bytes": len(a_ref),
                        "differs_at": [i for i in range(len(z_ref)) if z_ref[i] != a_ref[i]]}
    data = cases.build([["text", 3, 0, 300000]])
    g["error_codes"] = {"write_fail_after_5000": ref.encode(data, 2, 1 << 20, alloc=za, writer=BytesWriter(fail_after=5000))[0],
                        "read_fail_at_200000": ref.encode(data, 2, 1 << 20, alloc=za, reader=BytesReader(data, max_read=100000, fail_at=200000))[0]}
    data = cases.build(cases.STREAM_CASES["mix_types"][0])
    s = ref.encode(data, 3, 1 << 20, alloc=za)[1]
    g["corrupted"] = {"stream_sha256": sha(s), "decoded": [decoded(ref.decode(b, alloc=za)) for b in cases.corruptions(s)]}
    json.dump(g, open(os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.json"), "w"), indent=1)
    print("wrote tests/golden/oracle_vs_ref.json:", len(g["streams"]), "streams,", len(g["corrupted"]["decoded"]), "corrupted decodes")


if __name__ == "__main__":
    main()
