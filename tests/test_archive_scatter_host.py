"""CPU tier for the device archive over the caller's buffers (include/csa_mi355x.h: CSAMI_CheckBuffers, CSAMI_DeviceWriteFrom,
CSAMI_DeviceReadInto, CSAMI_DeviceCompare): the declarations, the exports, the ctypes mirrors, the refusal without a device, the
address checks on made-up addresses, and the text k_frag_compare / k_frag_fold_diff run (csc_amd/csrc/csa_dev_read.h: compare_sum,
compare_piece, fold_first) compiled for the host with the sanitizers and run as a program of its own
(tests/model/csa_dev_compare_model.cpp)."""
import ctypes as C
import os
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["CSAMI_CheckBuffers", "CSAMI_DeviceWriteFrom", "CSAMI_DeviceReadInto", "CSAMI_DeviceCompare"]
M64 = 1 << 64


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevArchive *a = 0; CSADevFile f; CSADevReadStats s; CSADevStopStats ss; CSADevWriteStats ws; CSADevDiff d;\n"
                   "  void *p[1] = {0}; const void *q[1] = {0}; uint64_t n[1] = {0}; uint32_t bad = 0; char arc[64] = {0};\n"
                   "  f.name = \"a\"; f.esize = f.edate = f.eattr = 0; f.offset = f.size = 0; f.nfrags = f.failed_frags = 0;\n"
                   "  d.first_diff = 0; d.status = CSA_DIFF_BYTES | CSA_DIFF_SIZE | CSA_DIFF_SKIPPED | CSA_DIFF_SHORT; d.failed_frags = 0;\n"
                   "  if (CSAMI_CheckBuffers(q, n, 1, arc, 64, 1, &bad)) return 1;\n"
                   "  CSAMI_DeviceWriteFrom(q, &f, 1, \"x.csa\", arc, 64, 0, &ws);\n"
                   "  CSAMI_DeviceReadInto(a, 0, 0, p, n, 1, CSAMI_DEV_STOP_EARLY, 0, &f, &s, &ss);\n"
                   "  return CSAMI_DeviceCompare(a, 0, 0, q, n, 1, 0, 0, &f, &d, &s, &ss); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_four_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in FOUR if s not in have] == []
    assert [s for s in FOUR if s not in csa.SYMBOLS] == []


def test_ctypes_mirror_has_the_c_layout(tmp_path, csa):
    D = csa.CSADevDiff
    df = [n for n, _ in D._fields_]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){ printf("%zu", sizeof(CSADevDiff));\n'
                   + "".join(f'  printf(" %zu", offsetof(CSADevDiff, {n}));\n' for n in df)
                   + '  printf(" %u %u %u %u %u", CSAMI_DEV_STOP_EARLY, CSA_DIFF_BYTES, CSA_DIFF_SIZE, CSA_DIFF_SKIPPED, CSA_DIFF_SHORT);\n'
                   + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(D)] + [getattr(D, n).offset for n in df] + [
        csa.CSAMI_DEV_STOP_EARLY, csa.CSA_DIFF_BYTES, csa.CSA_DIFF_SIZE, csa.CSA_DIFF_SKIPPED, csa.CSA_DIFF_SHORT]
    assert C.sizeof(D) == 16, "16 bytes a fragment is also what k_frag_fold_diff leaves to read back"


def test_no_gpu_means_none_of_the_three(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    name = C.create_string_buffer(b"a")
    f = csa.CSADevFile()
    f.name, f.esize, f.offset, f.size, f.nfrags = C.cast(name, C.c_void_p), 8, 77, 78, 79
    before = bytes(f)
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    ptrs = (C.c_void_p * 1)(C.addressof(buf) + 1024)
    sizes = (C.c_uint64 * 1)(8)

    def marked(T):
        t = T()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        return t
    ws, rs, ss = marked(csa.CSADevWriteStats), marked(csa.CSADevReadStats), marked(csa.CSADevStopStats)
    d = marked(csa.CSADevDiff)
    o = csa.options()
    assert L.CSAMI_DeviceWriteFrom(ptrs, C.byref(f), 1, b"x.csa", buf, 1024, C.byref(o), C.byref(ws)) == csa.CSCMI_DEVICE_ERROR
    # (no handle can exist without a device: the refusal has to come before the handle is looked at)
    assert L.CSAMI_DeviceReadInto(None, None, 0, ptrs, sizes, 1, 0, C.byref(o), C.byref(f), C.byref(rs), C.byref(ss)) == csa.CSCMI_DEVICE_ERROR
    assert L.CSAMI_DeviceCompare(None, None, 0, ptrs, sizes, 1, 1, C.byref(o), C.byref(f), C.byref(d), C.byref(rs), C.byref(ss)) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096
    for t in (ws, rs, ss, d):
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. the address checks ------------------------------------------------------------------------------------------------

def test_adjacent_ranges_pass_and_one_byte_of_overlap_does_not(csa):
    assert csa.check_buffers([0x1000, 0x1100, 0x1200], [0x100, 0x100, 0x100], disjoint=True) == (0, None)
    assert csa.check_buffers([0x1000, 0x1300, 0x10FF, 0x2000], [0x100, 0x100, 0x100, 1], disjoint=True) == (-1, 0)
    assert csa.check_buffers([0x5000, 0x1300, 0x1000, 0x10FF], [0x100, 0x100, 0x100, 0x100], disjoint=True) == (-1, 2)
    # a long range in front hides nothing: [0x1000, 0x9000) holds both others, which do not touch each other
    assert csa.check_buffers([0x2000, 0x3000, 0x1000], [0x10, 0x10, 0x8000], disjoint=True) == (-1, 0)
    assert csa.check_buffers([0x3000, 0x1000, 0x2000, 0x1800], [0x10, 0x8000, 0x10, 0x10], disjoint=True) == (-1, 0)
    # the same range twice
    assert csa.check_buffers([0x1000, 0x4000, 0x4000], [0x10, 0x10, 0x10], disjoint=True) == (-1, 1)


def test_a_range_of_size_zero_overlaps_nothing(csa):
    # inside another range, NULL, at another's first byte, inside the excluded range
    assert csa.check_buffers([0x1000, 0x1080, 0, 0x1000, 0x2004], [0x100, 0, 0, 0, 0], excl=(0x2000, 0x10), disjoint=True) == (0, None)
    assert csa.check_buffers([], [], disjoint=True) == (0, None)


def test_null_with_bytes_is_refused(csa):
    assert csa.check_buffers([0x1000, 0, 0x2000], [0x10, 1, 0x10]) == (-1, 1)
    assert csa.check_buffers([0, 0, 0x2000], [0, 1, 0x10], disjoint=True) == (-1, 1)


def test_the_end_of_the_address_space(csa):
    assert csa.check_buffers([M64 - 0x100], [0x100], disjoint=True) == (0, None)
    assert csa.check_buffers([0x1000, M64 - 0x100], [0x10, 0x101], disjoint=True) == (-1, 1)
    assert csa.check_buffers([1], [M64 - 1]) == (0, None)
    assert csa.check_buffers([2], [M64 - 1]) == (-1, 0)


def test_overlap_with_the_excluded_range(csa):
    excl = (0x4000, 0x100)
    assert csa.check_buffers([0x3F00], [0x100], excl=excl) == (0, None)                  # ends where it begins
    assert csa.check_buffers([0x4100], [0x100], excl=excl) == (0, None)                  # begins where it ends
    assert csa.check_buffers([0x1000, 0x3F00], [0x10, 0x101], excl=excl) == (-1, 1)      # its first byte
    assert csa.check_buffers([0x1000, 0x2000, 0x40FF], [0x10, 0x10, 1], excl=excl) == (-1, 2)   # its last byte
    assert csa.check_buffers([0x3000], [0x2000], excl=excl) == (-1, 0)                   # containing it
    assert csa.check_buffers([0x4010], [0x10], excl=excl) == (-1, 0)                     # inside it
    assert csa.check_buffers([0x4010], [0x10], excl=(0x4000, 0)) == (0, None)            # an empty one excludes nothing


def test_aliasing_is_allowed_unless_disjoint(csa):
    ptrs, sizes = [0x1000, 0x1000, 0x1080], [0x100, 0x100, 0x100]
    assert csa.check_buffers(ptrs, sizes, disjoint=False) == (0, None)
    assert csa.check_buffers(ptrs, sizes, disjoint=True) == (-1, 0)
    assert csa.check_buffers(ptrs, sizes, excl=(0x10FF, 1), disjoint=False) == (-1, 0)


def test_a_hundred_thousand_ranges_are_sorted_not_paired(csa):
    n = 100000
    ptrs = (C.c_void_p * n)(*[0x10000 + 64 * (n - 1 - i) for i in range(n)])            # reverse address order
    sizes = (C.c_uint64 * n)(*([64] * n))
    bad = C.c_uint32(0)
    t0 = time.perf_counter()
    rc = csa.lib().CSAMI_CheckBuffers(ptrs, sizes, n, None, 0, 1, C.byref(bad))
    dt = time.perf_counter() - t0
    assert rc == 0 and dt < 0.5, dt                     # (all pairs: 5e9 comparisons)
    sizes[0] = 65                                        # the highest range grows by one byte: nothing behind it
    assert csa.lib().CSAMI_CheckBuffers(ptrs, sizes, n, None, 0, 1, C.byref(bad)) == 0
    sizes[n - 1] = 65                                    # the lowest one: into its neighbour
    assert csa.lib().CSAMI_CheckBuffers(ptrs, sizes, n, None, 0, 1, C.byref(bad)) == -1 and bad.value == n - 2


# ---- 3. the kernels' text on the CPU ------------------------------------------------------------------------------------

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384]


def _compare_cases():
    """the cases tests/model/csa_dev_compare_model.cpp runs, counted by its rules"""
    count = 0
    for xa in range(16):
        for n in LENS:
            head = min((16 - xa) & 15, n)
            units = (n - head) >> 4
            at = [0, head - 1, head, head + 15, head + 16, head + 16 * (units - 1) if units else -1, n - 1, n // 3 if n >= 2 else -1]
            count += 16 * (1 + sum(0 <= k < n for k in at))
    parts = [(100, 0), (100, 37), (100, 100), (4097, 4096), (16384, 1), (16384, 16383), (16384, 8200)]
    count += 4 * sum(1 + (cmp > 0) + (cmp < ln) for ln, cmp in parts)
    return count + 6 * 6


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devcmp") / "csa_dev_compare_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_compare_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


def test_compare_sum_piece_and_fold_under_the_sanitizers(model):
    """16 x 16 alignments x 14 lengths x up to 9 difference cases; pieces compared in part; fragments of three pieces"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == f"ok {_compare_cases()}"


@pytest.mark.parametrize("plant,where,how", [
    (5, "cmp xa=1 ya=0 n=1 diff=0", "FAIL"),              # head bytes not compared: the first range that has one
    (6, "cmp xa=1 ya=0 n=31 diff=head", "FAIL"),          # a unit's index taken without the head: the first unit behind a head
    (7, "cmp xa=0 ya=1 n=16 diff=none", "AT"),            # y's 32-byte window not checked: the first unit of an unaligned y that ends with it (ASan)
    (8, "fold res=0 diff=16384", "FAIL"),                 # the piece index dropped from a fragment's first difference: the first one in piece 1
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, where, how):
    out = model(plant)
    assert out.returncode != 0
    if how == "FAIL":
        assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
    else:
        named = [l for l in out.stderr.splitlines() if l.startswith("AT ")]
        assert named[-1] == f"AT {where}" and "heap-buffer-overflow" in out.stderr and "csa_dev_read.h" in out.stderr
