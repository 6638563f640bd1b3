"""CPU tier of the drop-in rows: the reference's own two callers of the C boundary -- the archiver (archiver/*.cpp) and the command-line
tool (libcsc/csc.cpp) -- linked against libcsc_mi355x.so by oracle/Makefile (oracle/_ref/csarc_on_product, csc_on_product), and the record of
what the tool prints and writes on the REFERENCE's libcsc (oracle/_ref/csc_ref -> tests/golden/dropin_cli.json, tools/make_golden_dropin.py).

Here: the link itself (what each binary needs and imports), the record against the tool run live, and the record against both checkers
through capi -- streams, the "Estimated memory usage" line and every (in, out) pair of ICompressProgress, encode and decode.  No
`on_product` binary is run: without a GPU CSCEnc_Create returns NULL and the reference's callers dereference it.  The GPU tier
(tests/test_gpu_dropin.py) runs them."""
import json
import os
import subprocess
import sys

import pytest

import cases
import dropin_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
HAVE_REF = os.path.exists(os.path.join(REFDIR, "libcsc_ref.so"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built (needs the reference tree)")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "dropin_cli.json")))

ELEVEN = {"CSCEncProps_Init", "CSCEnc_WriteProperties", "CSCEnc_EstMemUsage", "CSCEnc_Create", "CSCEnc_Destroy", "CSCEnc_Encode",
          "CSCEnc_Encode_Flush", "CSCDec_ReadProperties", "CSCDec_Create", "CSCDec_Destroy", "CSCDec_Decode"}
IMPORTS = {"csarc_on_product": ELEVEN - {"CSCEnc_EstMemUsage"}, "csc_on_product": ELEVEN}


def _nm(path, which):
    out = subprocess.run(["nm", "-D", which, path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}


# ---------------------------------------------------------------------------------------------
# the link
# ---------------------------------------------------------------------------------------------
@needs_ref
def test_build_leaves_the_three_binaries():
    for name in ("csarc_on_product", "csc_on_product", "csc_ref"):
        path = os.path.join(REFDIR, name)
        assert os.path.isfile(path) and os.access(path, os.X_OK), name


@needs_ref
@pytest.mark.parametrize("name", sorted(IMPORTS))
def test_on_product_binary_needs_the_product_library(name):
    out = subprocess.run(["readelf", "-d", os.path.join(REFDIR, name)], capture_output=True, text=True, check=True).stdout
    needed = [l.split("[")[1].split("]")[0] for l in out.splitlines() if "(NEEDED)" in l]
    assert "libcsc_mi355x.so" in needed and not [n for n in needed if "orc" in n or "csc_ref" in n], needed
    # found relative to the binary, so the pair still works when the tree is copied elsewhere
    path = [l.split("[")[1].split("]")[0] for l in out.splitlines() if "(RUNPATH)" in l or "(RPATH)" in l]
    assert path == ["$ORIGIN/../../csc_amd"], path


@needs_ref
@pytest.mark.parametrize("name", sorted(IMPORTS))
def test_on_product_binary_imports_the_c_boundary_and_nothing_else(name):
    """every CSC* symbol undefined, none defined (no libcsc object went into the link); of all the product library exports the
    binary takes the reference's 10 (archiver) or 11 (command-line tool) entry points and no extension"""
    path = os.path.join(REFDIR, name)
    undefined, defined = _nm(path, "--undefined-only"), _nm(path, "--defined-only")
    assert {s for s in undefined if s.startswith("CSC")} == IMPORTS[name]
    assert not {s for s in defined if s.startswith(("CSC", "CSA"))}
    exported = _nm(os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so"), "--defined-only")
    assert ELEVEN <= exported and undefined & exported == IMPORTS[name]


# ---------------------------------------------------------------------------------------------
# the record against the tool itself
# ---------------------------------------------------------------------------------------------
def test_golden_holds_the_cases():
    assert list(GOLD) == list(dc.CLI_CASES)
    for case, g in GOLD.items():
        assert g["argv"] == dc.encode_argv(case) and g["spec"] == dc.CLI_CASES[case][0] and g["decode_argv"] == dc.decode_argv()
        data = cases.build(g["spec"])
        assert (len(data), cases.digest(data)) == (g["input_size"], g["decoded_sha256"]) and g["decoded_size"] == len(data)
    # what the issue's author saw on the reference: a second chunk of 5 bytes, `1 -> 11`, 27 bytes and no record for nothing, `7 -> 0` back
    assert [p[0] for p in dc.parse_stderr(GOLD["text_2m5_m1_d1m"]["encode_stderr"])[1]] == [2 << 20, (2 << 20) + 5]
    assert dc.parse_stderr(GOLD["one_byte"]["encode_stderr"])[1] == [(1, 11)]
    assert GOLD["empty"]["stream_size"] == 27 and dc.parse_stderr(GOLD["empty"]["encode_stderr"])[1] == []
    assert dc.parse_stderr(GOLD["empty"]["decode_stderr"]) == (None, [(7, 0)])


@needs_ref
@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_golden_equals_the_reference_tool_live(case):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_dropin
    ent, _ = make_golden_dropin.record(case)
    assert ent == GOLD[case]


# ---------------------------------------------------------------------------------------------
# the record against the checkers through capi: what tests/test_gpu_dropin.py holds the product's callers to is what the
# oracle and the reference library do behind the same boundary
# ---------------------------------------------------------------------------------------------
def drained_payload(stream, props):
    """payload bytes of the whole coder blocks in `stream` (header included): MemIO::WriteBlock's framing, csc_memio.cpp:83-108"""
    pos, total = 10, 0
    while pos < len(stream):
        fb = stream[pos]
        pos += 1
        if fb & 0x40:
            size = props.csc_blocksize
        else:
            size = int.from_bytes(stream[pos:pos + 3], "big")
            pos += 3
        pos += size
        total += size
    assert pos == len(stream)
    return total


def through_capi(lib, case, alloc):
    """the case through `lib` in the caller order of csc.cpp:137-163 -> what the tool would have printed and written"""
    from csc_amd.capi import BytesWriter
    data = cases.build(dc.CLI_CASES[case][0])
    props = dc.props_of(lib, case, len(data))
    w = BytesWriter()
    enc, drained = [], []

    def on_encode(a, b):
        enc.append((a, b))
        drained.append(drained_payload(bytes(w.out), props))          # what had reached Write when Progress was called

    rc, stream = lib.encode(data, props=props, alloc=alloc, writer=w, progress=on_encode)
    assert rc == 0
    dec = []
    rcd, back = lib.decode(stream, alloc=alloc, progress=lambda a, b: dec.append((a, b)))
    assert rcd == 0 and back == data
    return {"mem_mb": lib.est_mem_usage(props) // 1048576, "stream": stream, "encode_pairs": enc, "drained_at_progress": drained, "decode_pairs": dec}


@pytest.fixture(scope="module")
def orc_runs(orc, zalloc):
    return {case: through_capi(orc, case, zalloc) for case in dc.CLI_CASES}


@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_recorded_stream_is_the_oracles(orc_runs, case):
    s = orc_runs[case]["stream"]
    assert (len(s), cases.digest(s)) == (GOLD[case]["stream_size"], GOLD[case]["stream_sha256"])


@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_recorded_progress_and_memory_line_are_the_oracles(orc_runs, case):
    mem, pairs = dc.parse_stderr(GOLD[case]["encode_stderr"])
    r = orc_runs[case]
    assert (mem, pairs) == (r["mem_mb"], r["encode_pairs"])
    assert dc.parse_stderr(GOLD[case]["decode_stderr"]) == (None, r["decode_pairs"])


@needs_ref
@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_recorded_progress_and_memory_line_are_the_reference_librarys(ref, zalloc, case):
    r = through_capi(ref, case, zalloc)
    assert (len(r["stream"]), cases.digest(r["stream"])) == (GOLD[case]["stream_size"], GOLD[case]["stream_sha256"])
    assert dc.parse_stderr(GOLD[case]["encode_stderr"]) == (r["mem_mb"], r["encode_pairs"])
    assert dc.parse_stderr(GOLD[case]["decode_stderr"]) == (None, r["decode_pairs"])


@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_memory_line_and_header_of_the_product(prod, orc, case):
    """CSCEncProps_Init, CSCEnc_EstMemUsage and CSCEnc_WriteProperties are host arithmetic: the product's line and header need no GPU"""
    n = GOLD[case]["input_size"]
    p, q = dc.props_of(prod, case, n), dc.props_of(orc, case, n)
    assert p.as_dict() == q.as_dict() and prod.write_properties(p) == orc.write_properties(q)
    assert prod.est_mem_usage(p) // 1048576 == dc.parse_stderr(GOLD[case]["encode_stderr"])[0]


@pytest.mark.parametrize("case", list(dc.CLI_CASES))
def test_out_size_is_the_payload_drained_when_progress_is_called(orc_runs, case):
    """The product's CSCEnc_Encode reports the payload of the coder blocks it has handed to Write (csc_host.cpp: write_arena adds
    every block's size, drain_arena runs before Progress); the reference reports outsize_ + rc_size_ + bc_size_
    (csc_encoder_main.cpp:174-177).  The two are the same number at every Progress call, because CSCEncoder::Compress ends each
    chunk with Coder::Flush (csc_encoder_main.cpp:141-145): both pending counts are zero and every byte counted has been written.
    Held here on the checker's Write sequence -- which the GPU tier holds the product's to -- against the recorded pairs."""
    pairs = dc.parse_stderr(GOLD[case]["encode_stderr"])[1]
    assert orc_runs[case]["drained_at_progress"] == [b for _, b in pairs]
