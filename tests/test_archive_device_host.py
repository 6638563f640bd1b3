"""CPU tier for the device-resident archive read (CSAMI_DeviceOpen / Plan / Read / Close, include/csa_mi355x.h): the declarations,
the exports, the refusal without a device, the host-only planner (CSAMI_PlanDeviceLayout) against a plan written here in plain
Python over oracle/orc_csa.py, crafted indices, and the kernels' shared text (csc_amd/csrc/csa_dev_read.h: the piece split, the
copy between ranges of any alignment, the adler32 sums and their fold) compiled for the host with the sanitizers and run as a
program of its own (tests/model/csa_dev_model.cpp)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

import csa_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

FIVE = ["CSAMI_DeviceOpen", "CSAMI_DevicePlan", "CSAMI_DeviceRead", "CSAMI_DeviceClose", "CSAMI_PlanDeviceLayout"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevArchive *a = 0; CSADevFile f; CSADevReadStats s; uint32_t n = 0, nt = 0; uint64_t b = 0, r = 0;\n"
                   "  const uint8_t raw[8] = {0}; double ms[3];\n"
                   "  f.name = 0; f.esize = f.edate = f.eattr = 0; f.offset = f.size = 0; f.nfrags = f.failed_frags = 0;\n"
                   "  s.tasks = s.frags = s.waves = s.launches = s.decode_launches = s.readback_bytes = s.raw_bytes = 0;\n"
                   "  s.verify_failures = s.reserved = 0; s.kernel_ms = s.seconds_total = 0;\n"
                   "  if (CSAMI_DeviceOpen(0, 0, &a)) return 1;\n"
                   "  CSAMI_DevicePlan(a, 0, 0, &f, 1, &n, &b); CSAMI_DeviceRead(a, 0, 0, 0, 0, 0, &f, 1, &s); CSAMI_DeviceKernelMs(a, ms);\n"
                   "  CSAMI_DeviceClose(a);\n"
                   "  return CSAMI_PlanDeviceLayout(raw, 8, 24, 0, 0, &f, 1, &n, &b, &r, 1, &nt); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_five_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in FIVE if s not in have] == []


def test_ctypes_mirrors_have_the_c_layout(tmp_path, csa):
    F, S = csa.CSADevFile, csa.CSADevReadStats
    ff = [n for n, _ in F._fields_]
    sf = [n for n, _ in S._fields_]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){ printf("%zu %zu", sizeof(CSADevFile), sizeof(CSADevReadStats));\n'
                   + "".join(f'  printf(" %zu", offsetof(CSADevFile, {n}));\n' for n in ff)
                   + "".join(f'  printf(" %zu", offsetof(CSADevReadStats, {n}));\n' for n in sf) + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(F), C.sizeof(S)] + [getattr(F, n).offset for n in ff] + [getattr(S, n).offset for n in sf]


def test_no_gpu_means_no_device_archive(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    buf = (C.c_uint8 * 64)()
    h = C.c_void_p(0x1234)
    assert csa.lib().CSAMI_DeviceOpen(buf, 64, C.byref(h)) == csa.CSCMI_DEVICE_ERROR, "there is no CPU fallback"
    assert h.value == 0x1234, "*out is left alone"


# ---- 2. the planner against a plain-Python plan -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def archives(orc, zalloc, tmp_path_factory):
    """{case: (archive size, raw index bytes, parsed index, parsed block table)} for every CPU case, from the oracle container"""
    from csc_amd.capi import BytesWriter

    def enc(data, dict_size, level):
        w = BytesWriter()
        rc, s = orc.encode(data, props=orc.props_init(dict_size, level), alloc=zalloc, writer=w)
        assert rc == 0
        return s, [10] + w.sizes

    def dec(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw

    out = {}
    cwd = os.getcwd()
    try:
        for case in csa_cases.CPU_CASES:
            d = tmp_path_factory.mktemp(case)
            csa_cases.make_tree(str(d), case)
            os.chdir(d)
            spec = csa_cases.CSA_CASES[case]
            arc = orc_csa.create(csa_cases.ARCNAME, spec["args"], encode=enc, **spec["opts"])
            info = orc_csa.parse(arc, dec)
            out[case] = (len(arc), info["index_raw"], info["index"], info["abindex"])
    finally:
        os.chdir(cwd)
    return out


def python_plan(index, names):
    """the layout rules of include/csa_mi355x.h restated: -> ([file dicts], dst_bytes, [task raw sizes in decode order])"""
    raw = {}
    for e in index.values():
        for f in e["frags"]:
            raw[f["bid"]] = max(raw.get(f["bid"], 0), f["posblock"] + f["size"])
    files, off, totals = [], 0, {}
    for name in sorted(index, key=lambda s: s.encode("latin-1")):
        if not orc_csa.isselected(list(names), name):
            continue
        e = index[name]
        size = max([f["posfile"] + f["size"] for f in e["frags"]], default=0)
        files.append({"name": name, "esize": e["esize"], "edate": e["edate"], "eattr": e["eattr"], "offset": off, "size": size,
                      "nfrags": len(e["frags"]), "failed_frags": 0})
        off += (size + 15) // 16 * 16
        for f in e["frags"]:
            if f["size"]:
                totals[f["bid"]] = totals.get(f["bid"], 0) + f["size"]
    order = sorted(totals, key=lambda b: (-totals[b], b))
    return files, off, [raw[b] for b in order]


SELECTIONS = {"mixed_tree": [[], ["*.txt"], ["d/sub"], ["d/empty"], ["d/a.txt", "d/noext"], ["nothing"]],
              "many_files": [[], ["m/same*"], ["m/f0?.*"], ["m/tiny07.cfg"]],
              "chunk_edges_m5": [[], ["c/p2.raw"], ["c/p3.raw", "c/p0.raw"]],
              "single_split3": [[], ["big.bin"], ["*.txt"]]}


@pytest.mark.parametrize("case", csa_cases.CPU_CASES)
def test_planner_equals_the_plain_python_plan(csa, archives, case):
    arc_size, raw_index, index, _ = archives[case]
    for names in SELECTIONS.get(case, [[]]):
        rc, files, total, tasks = csa.plan_device_layout(raw_index, arc_size, names)
        want = python_plan(index, names)
        assert rc == 0 and (files, total, tasks) == want, (case, names)
        assert all(f["offset"] % 16 == 0 for f in files) and total % 16 == 0
    if case == "mixed_tree":
        got = {tuple(n): [f["name"] for f in csa.plan_device_layout(raw_index, arc_size, n)[1]] for n in ([], ["*.txt"], ["d/sub"], ["d/empty"])}
        assert got[("*.txt",)] == ["d/a.txt", "d/b.txt"] and got[("d/sub",)] == ["d/sub/", "d/sub/c.exe", "d/sub/e.dat"]
        assert got[("d/empty",)] == ["d/empty"] and len(got[()]) == 8
    if case == "single_shadowed_by_empty":       # csarc.cpp:516-530: a file the reference stored nothing of: listed, size 0, no task
        rc, files, total, tasks = csa.plan_device_layout(raw_index, arc_size, [])
        assert [(f["name"], f["esize"], f["size"], f["nfrags"]) for f in files if f["name"] == "q/a.bin"] == [("q/a.bin", 100000, 0, 0)]
        assert total == 0 and tasks == []


# ---- 3. crafted indices -----------------------------------------------------------------------------------------------

def _index(entries, blocks):
    """entries: [(name, [(bid, posblock, size, posfile)] or a raw fragment-count byte)]; blocks: {bid: [(off, size)]}"""
    index = {n: {"edate": 20231114221320, "esize": 1, "eattr": 0, "frags": [{"bid": b, "checksum": 0, "posblock": pb, "size": sz, "posfile": pf}
                                                                          for b, pb, sz, pf in fr]} for n, fr in entries}
    return orc_csa.pack_index(index, blocks, "out.csa")


M64 = 1 << 64
CRAFTED = {
    "a fragment size near 2^64": _index([("a", [(0, 0, M64 - 8, 0)])], {0: [(24, 100)]}),
    "file sizes whose rounded sum passes 2^64": _index([("a", [(0, 0, 1 << 63, 0)]), ("b", [(0, 0, 1 << 63, 0)])], {0: [(24, 100)]}),
    "posblock + size wraps": _index([("a", [(0, M64 - 16, 32, 0)])], {0: [(24, 100)]}),
    "posfile + size wraps": _index([("a", [(0, 0, 32, M64 - 16)])], {0: [(24, 100)]}),
    "an archive block past arc_size": _index([("a", [(0, 0, 32, 0)])], {0: [(24, 100), (4000, 97)]}),
    "an archive block whose end wraps": _index([("a", [(0, 0, 32, 0)])], {0: [(M64 - 4, 8)]}),
}


@pytest.mark.parametrize("what", list(CRAFTED))
def test_crafted_index_is_refused(csa, what):
    assert csa.plan_device_layout(CRAFTED[what], 4096, [])[0] == -1
    # (selected alone, either file of the wrapping sum fits: the layout is the selection's)
    assert csa.plan_device_layout(CRAFTED[what], 4096, ["a"])[0] == (0 if "rounded sum" in what else -1)


def test_crafted_fragment_counts(csa):
    """the count is one signed byte (csa_indexpack.cpp:105): 128 reads as -128 and the index does not parse; 127 does.  A count
    of 0 is what the reference itself writes for directories, empty files and the file of single_shadowed_by_empty, so it is
    not an error: the entry is listed with size 0 and asks for no task."""
    good = _index([("a", [(0, 32 * k, 32, 32 * k) for k in range(127)])], {0: [(24, 100)]})
    rc, files, total, tasks = csa.plan_device_layout(good, 4096, [])
    assert rc == 0 and files[0]["nfrags"] == 127 and files[0]["size"] == 127 * 32 == total and tasks == [127 * 32]
    count_at = 4 + 4 + 1 + 24
    assert good[count_at] == 127
    bad = bytearray(good[:count_at] + b"\x80" + good[count_at + 1:] + bytes(32))       # 128 fragments, and the bytes for them
    assert csa.plan_device_layout(bytes(bad), 4096, [])[0] == -1
    none = bytearray(_index([("a", [])], {}))
    assert none[count_at] == 0
    struct.pack_into("<q", none, 4 + 4 + 1 + 8, 12345)                                  # esize says 12345 bytes, the index holds none
    rc, files, total, tasks = csa.plan_device_layout(bytes(none), 4096, [])
    assert rc == 0 and [(f["name"], f["esize"], f["size"], f["nfrags"]) for f in files] == [("a", 12345, 0, 0)] and total == 0 and tasks == []
    for cut in (0, 3, 4, 7, count_at, len(good) - 70):                                  # and a truncated buffer never parses
        assert csa.plan_device_layout(good[:cut], 4096, [])[0] == -1


# ---- 4. the kernels' text on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devread") / "csa_dev_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


def test_copy_sum_split_and_fold_under_the_sanitizers(model):
    """16 x 16 alignments x 17 lengths, with and without the store, and 7 fragment sizes x 16 posblock residues"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == f"ok {2 * 16 * 16 * 17 + 7 * 16 * 2}"


def test_wave_planner_under_the_sanitizers(model):
    """wave_count and hbm_budget (csc_amd/csrc/csa_waves.h), which size the waves of CSA_Test / CSA_Extract, CSAMI_DeviceRead and
    CSAMI_DeviceWrite: width 1, a first task over the budget, the exact fit and one byte more, fewer tasks than the width, a need of
    UINT64_MAX, sums that wrap, and a walk over eight tasks"""
    out = model("waves")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == "ok waves 12"


@pytest.mark.parametrize("plant,where,how", [
    (1, "copy store=1 sa=0 da=0 n=1", "FAIL"),            # tail bytes dropped: the one byte of a 1-byte range is a tail byte
    (2, "copy store=1 sa=0 da=0 n=1", "FAIL"),            # weight len - i off by one: B of one byte is that byte
    (3, "frag size=32769 res=0 store=1", "FAIL"),         # the fold uses the last piece's length for all: the first fragment of three pieces
    (4, "copy store=1 sa=0 da=1 n=16", "IN"),             # head taken from src, not dst: the first 16-byte store to an unaligned dst (UBSan)
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, where, how):
    out = model(plant)
    assert out.returncode != 0
    if how == "FAIL":
        assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
    else:
        named = [l for l in out.stderr.splitlines() if l.startswith("IN ")]
        assert named[-1] == f"IN {where}" and "misaligned address" in out.stderr and "csa_dev_read.h" in out.stderr
