"""CPU tier for the fragment digests of the device archive (include/csa_mi355x.h: CSAMI_DeviceWriteFragCount, CSAMI_DeviceDigestSlices,
CSAMI_DeviceUpdateDigests, CSAMI_DeviceReadDigests): the declarations, the exports, the ctypes mirrors, the refusal without a device,
fragment_digest against the specification's vectors, the fragment count against the oracle-built archives, and the text
k_digest_leaves / k_digest_roots run (csc_amd/csrc/csa_dev_digest.h) compiled for the host with the sanitizers and run as a program
of its own (tests/model/csa_dev_digest_model.cpp), its digests compared with hashlib's."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import pytest

import csa_cases
import csa_write_cases
from test_archive_device_host import archives  # noqa: F401  (the fixture: every CPU case as the oracle container writes it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["CSAMI_DeviceWriteFragCount", "CSAMI_DeviceDigestSlices", "CSAMI_DeviceUpdateDigests", "CSAMI_DeviceReadDigests",
       "CSAMI_DeviceDigestKernelMs"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevFile f; CSADevWriteStats s; CSADevGatherStats g; CSADevUpdateStats u; CSADevUpdateTask t[2]; CSAOptions o;\n"
                   "  CSADevDigest d[2]; CSADevDigestStats ds; CSADevReadStats rs; uint64_t nf = 0; double ms[2];\n"
                   "  const void *p[1] = {0}; unsigned char arc[64];\n"
                   "  f.name = 0; CSA_OptionsInit(&o); d[0].b[31] = 0;\n"
                   "  ds.frags = ds.leaves = ds.digested_bytes = ds.launches = ds.mismatches = 0; ds.first_mismatch = UINT64_MAX; ds.kernel_ms = 0;\n"
                   "  CSAMI_DeviceDigestKernelMs(ms);\n"
                   '  if (CSAMI_DeviceWriteFragCount(&f, 1, "a.csa", &o, &nf)) return 1;\n'
                   '  if (CSAMI_DeviceDigestSlices(p, 0, 0, &f, 1, "a.csa", &o, d, 2, &ds)) return 2;\n'
                   "  if (CSAMI_DeviceReadDigests(0, &o, d, 2, d, &rs, &ds)) return 3;\n"
                   '  return CSAMI_DeviceUpdateDigests(0, d, 2, p, 0, 0, &f, 1, "a.csa", arc, sizeof(arc),\n'
                   "                                   CSAMI_UPDATE_TRUST_DIGESTS | CSAMI_UPDATE_TRUST_SUMS, &o, &s, &g, &u, t, 2, d, 2, &ds); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in NEW if s not in have or s not in csa.SYMBOLS] == []


def test_ctypes_mirrors_have_the_c_layout(tmp_path, csa):
    pairs = [("CSADevDigest", csa.CSADevDigest, 32), ("CSADevDigestStats", csa.CSADevDigestStats, 56)]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   + "".join(f'  printf(" %zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in T._fields_)
                             for name, T, _ in pairs) + '  printf(" %u", CSAMI_UPDATE_TRUST_DIGESTS);\n  return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, T, size in pairs:
        assert C.sizeof(T) == size
        want += [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]
    assert got == want + [csa.CSAMI_UPDATE_TRUST_DIGESTS]
    assert len(csa.CSADevDigestStats().as_dict()) == len(csa.CSADevDigestStats._fields_)
    assert not set(csa.CSADevDigestStats().as_dict()) & (set(csa.CSADevWriteStats().as_dict()) | set(csa.CSADevReadStats().as_dict())
                                                        | set(csa.CSADevUpdateStats().as_dict()) | set(csa.CSADevGatherStats().as_dict()))


def test_no_gpu_means_no_digests(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    name = C.create_string_buffer(b"a")
    f = csa.CSADevFile()
    f.name, f.esize, f.offset, f.size, f.nfrags = C.cast(name, C.c_void_p), 4, 77, 78, 79
    before = bytes(f)
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    at = C.addressof(buf)
    ptrs = (C.c_void_p * 1)(at + 1024)
    st, gs, us, tasks = csa.CSADevWriteStats(), csa.CSADevGatherStats(), csa.CSADevUpdateStats(), (csa.CSADevUpdateTask * 2)()
    ds, rs = csa.CSADevDigestStats(), csa.CSADevReadStats()
    every = (st, gs, us, tasks, ds, rs)
    for t in every:
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    o = csa.options()
    # (the handles are not looked at either: the refusal comes first)
    assert L.CSAMI_DeviceDigestSlices(ptrs, None, None, C.byref(f), 1, b"a.csa", C.byref(o), at + 3072, 1, C.byref(ds)) == csa.CSCMI_DEVICE_ERROR
    assert L.CSAMI_DeviceUpdateDigests(C.c_void_p(0x1234), at + 3200, 1, ptrs, None, None, C.byref(f), 1, b"a.csa", at + 2048, 1024,
                                       csa.CSAMI_UPDATE_TRUST_DIGESTS, C.byref(o), C.byref(st), C.byref(gs), C.byref(us), tasks, 2,
                                       at + 3072, 1, C.byref(ds)) == csa.CSCMI_DEVICE_ERROR
    assert L.CSAMI_DeviceReadDigests(C.c_void_p(0x1234), C.byref(o), at + 3072, 1, at + 3200, C.byref(rs), C.byref(ds)) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096
    for t in every:
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. the host reference and the fragment count ---------------------------------------------------------------------------

VECTORS = [(b"", "ad25eb732f7403ecdc8c73f81df7597e975d355ad9d485b0e72768d97245385e"),
           (b"abc", "942afdd6c58b3e9576b18aa0eae931decc2dc61bbcd2ec0bfee786f472fbb9b5"),
           (bytes(range(256)) * 129, "33e75affb83c11081bc8af8bf99d5e47528eeabcbfe57d7da63e31991b31cf6d")]


def test_fragment_digest_gives_the_specification_vectors(csa):
    assert [csa.fragment_digest(data).hex() for data, _ in VECTORS] == [want for _, want in VECTORS]
    # one leaf is NOT plain BLAKE2s: the tree parameters enter the parameter block
    assert csa.fragment_digest(b"abc") != hashlib.blake2s(b"abc").digest()
    assert csa.fragment_digest(bytearray(b"abc")) == csa.fragment_digest(memoryview(b"abc"))


def _edate(csa):
    return int(csa.lib().CSA_DecimalTime(csa_cases.MTIME))


@pytest.mark.parametrize("case", csa_cases.CPU_CASES)
def test_frag_count_equals_the_oracle_archives(csa, archives, case):  # noqa: F811
    files, _, _ = csa_write_cases.table(case, _edate(csa), with_bytes=False)
    opts = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k in ("level", "dict_size", "split_count")}
    index = archives[case][2]
    assert csa.device_write_frag_count(files, **opts) == (0, sum(len(e["frags"]) for e in index.values()))
    assert csa.device_write_frag_count(files[::-1], **opts)[1] == sum(len(e["frags"]) for e in index.values())


def test_frag_count_refuses_what_the_write_plan_refuses(csa):
    row = {"name": "a", "esize": 10, "edate": 1, "eattr": csa_write_cases.FILE_ATTR}
    assert csa.device_write_frag_count([row, dict(row)])[0] == -1, "a name twice"
    assert csa.device_write_frag_count([dict(row, esize=-1)])[0] == -1
    assert csa.device_write_frag_count([]) == (0, 0)
    assert csa.device_write_frag_count([dict(row, esize=200 << 20)], split_count=128)[0] == csa.CSA_TOO_MANY_FRAGMENTS


# ---- 3. the kernels' text on the CPU ----------------------------------------------------------------------------------------

SIZES = [0, 1, 55, 63, 64, 65, 127, 128, 16383, 16384, 16385, 32768, 49153]
ALIGNS = [0, 1, 7, 8, 15]
ROWS = 2 * 5 * 2


def _fragment(n):
    return bytes((((i * 2654435761 + n) & 0xFFFFFFFF) >> 13) & 0xFF for i in range(n))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devdigest") / "csa_dev_digest_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_digest_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


@pytest.fixture(scope="module")
def expected(csa):
    return {n: csa.fragment_digest(_fragment(n)).hex() for n in SIZES}


def _first_wrong(stdout, expected):
    """the cases the model printed, and the first whose digest is not hashlib's (None: every one is)"""
    cases, wrong = [], None
    for line in stdout.splitlines():
        m = re.fullmatch(r"((?:rows )?size=(\d+) .*) ([0-9a-f]{64})", line)
        if not m:
            continue
        cases.append(m.group(1))
        if wrong is None and m.group(3) != expected[int(m.group(2))]:
            wrong = m.group(1)
    return cases, wrong


def test_the_digest_text_under_the_sanitizers(model, expected):
    """13 sizes x 5 source alignments out of sources exactly as large as their fragments, and fragments that are the runs of a
    periodic slice (run 5, 16, 17 = stride, 4099, 20000) out of buffers exactly as large as their hulls: every digest is hashlib's;
    the root's tables byte by byte at odd addresses"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    cases, wrong = _first_wrong(out.stdout, expected)
    assert wrong is None
    assert cases[:len(SIZES) * len(ALIGNS)] == [f"size={n} al={a}" for n in SIZES for a in ALIGNS]
    assert len(cases) == len(SIZES) * len(ALIGNS) + ROWS
    assert out.stdout.splitlines()[-2:] == ["root ok", f"ok {len(cases)}"]


@pytest.mark.parametrize("plant,where", [
    # an extra empty block after a multiple of 64: the first leaf whose length is one
    (1, "size=64 al=0"),
    # the last-node flag on every leaf: the first fragment of more than one leaf
    (2, "size=16385 al=0"),
    # the node offset not set: the same fragment, whose second leaf has offset 1
    (3, "size=16385 al=0"),
])
def test_planted_mistakes_give_another_digest_at_named_cases(model, expected, plant, where):
    out = model(plant)
    assert out.returncode == 0, out.stderr[-4000:]
    assert _first_wrong(out.stdout, expected)[1] == where


def test_a_load_window_past_the_leaf_is_the_sanitizers_to_report(model):
    """the 17-word window of a whole block off the 4-byte line not checked against the leaf's end: the first leaf whose last block is
    whole and off the line is 128 bytes at alignment 1"""
    out = model(4)
    assert out.returncode != 0
    named = [l for l in out.stderr.splitlines() if l.startswith("AT ")]
    assert named[-1] == "AT size=128 al=1" and "heap-buffer-overflow" in out.stderr and "csa_dev_digest.h" in out.stderr
