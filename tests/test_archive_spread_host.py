"""CPU tier for reading into and comparing against strided slices of the caller's buffers (include/csa_mi355x.h:
CSAMI_DeviceReadIntoSlices, CSAMI_DeviceCompareSlices, CSAMI_CheckSlices): the declarations, the exports, the ctypes mirror, the refusal
without a device, CSAMI_CheckSlices against a brute-force set of selected addresses, and the text k_frag_spread and
k_frag_compare_rows run (csc_amd/csrc/csa_dev_read.h: spread_sum, compare_rows) compiled for the host with the sanitizers and run as a
program of its own (tests/model/csa_dev_spread_model.cpp)."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["CSAMI_CheckSlices", "CSAMI_DeviceReadIntoSlices", "CSAMI_DeviceCompareSlices"]
M64 = 1 << 64


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declarations, exports, layout, refusal ------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevFile f; CSADevReadStats s; CSADevStopStats t; CSADevSpreadStats x; CSADevSlice c; CSADevDiff d; CSAOptions o;\n"
                   "  void *p[1] = {0}; const void *q[1] = {0}; uint64_t n[1] = {0}; uint32_t bad = 0; int r;\n"
                   "  c.offset = 0; c.run = 1; c.stride = 2; c.count = 3; f.name = 0; CSA_OptionsInit(&o);\n"
                   "  x.selected_bytes = x.hull_bytes = x.periodic_pieces = x.plain_pieces = 0;\n"
                   "  r = CSAMI_CheckSlices(q, n, &c, 1, 0, 0, 1, &bad);\n"
                   "  r += CSAMI_DeviceReadIntoSlices(0, 0, 0, p, n, &c, 1, CSAMI_DEV_STOP_EARLY, &o, &f, &s, &t, &x);\n"
                   "  r += CSAMI_DeviceCompareSlices(0, 0, 0, q, n, &c, 1, 0, &o, &f, &d, &s, &t, &x);\n"
                   "  return r + (int)x.hull_bytes + (int)bad; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    for name in NEW:
        assert name in have and name in csa.SYMBOLS, name


def test_ctypes_mirror_has_the_c_layout(tmp_path, csa):
    name, T = "CSADevSpreadStats", csa.CSADevSpreadStats
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   + f'  printf(" %zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in T._fields_)
                   + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_] and C.sizeof(T) == 32


def test_no_gpu_means_no_sliced_read_and_no_sliced_compare(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    ptrs = (C.c_void_p * 1)(C.addressof(buf) + 1024)
    sizes = (C.c_uint64 * 1)(8)
    sl = (csa.CSADevSlice * 1)()
    sl[0].offset, sl[0].run, sl[0].stride, sl[0].count = 1, 2, 3, 2
    sliced = bytes(sl)
    o = csa.options()
    for compare in (False, True):
        f, d = csa.CSADevFile(), csa.CSADevDiff()
        st, ss, sp = csa.CSADevReadStats(), csa.CSADevStopStats(), csa.CSADevSpreadStats()
        for t in (f, d, st, ss, sp):
            C.memset(C.byref(t), 0x5A, C.sizeof(t))
        head = (C.c_void_p(C.addressof(buf)), None, 0, ptrs, sizes, sl, 1, 0, C.byref(o), C.byref(f))      # (the handle is not looked at)
        if compare:
            rc = L.CSAMI_DeviceCompareSlices(*head, C.byref(d), C.byref(st), C.byref(ss), C.byref(sp))
        else:
            rc = L.CSAMI_DeviceReadIntoSlices(*head, C.byref(st), C.byref(ss), C.byref(sp))
        assert rc == csa.CSCMI_DEVICE_ERROR
        assert bytes(buf) == b"\xa5" * 4096 and bytes(sl) == sliced
        for t in (f, d, st, ss, sp):
            assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. CSAMI_CheckSlices -------------------------------------------------------------------------------------------------

BASE = 1 << 32                                                         # (host only: the addresses are never touched)
ROOM = 1 << 20


def _selected(ptr, s):
    off, run, stride, count = s
    return {ptr + off + k * (stride if count > 1 else run) + r for k in range(count) for r in range(run)}


def _hull(ptr, s):
    off, run, stride, count = s
    return (ptr + off, ptr + off + (count - 1) * (stride if count > 1 else run) + run) if count else (0, 0)


def test_check_slices_never_accepts_selections_that_meet(csa):
    rng = random.Random(20250)
    accepted = accepted_interleaved = refused = 0
    for case in range(600):
        kind = case % 4
        stride = rng.randint(2, 120)

        def one():
            count = rng.choice([1, 1, 2, 3, 7, 30])
            st = stride if kind < 3 else rng.randint(2, 120)           # three in four: one stride for both
            run = rng.randint(1, st if kind else max(1, st // 2))
            count = min(count, (4096 - run) // st + 1)
            return (rng.randint(0, 300), run, st, count)
        a, b = one(), one()
        assert all(h[1] - h[0] <= 4096 for h in (_hull(BASE, a), _hull(BASE, b)))
        rc, bad = csa.check_slices([BASE, BASE], [ROOM, ROOM], [a, b], disjoint=True)
        meet = bool(_selected(BASE, a) & _selected(BASE, b))
        (la, ha), (lb, hb) = _hull(BASE, a), _hull(BASE, b)
        apart = ha <= lb or hb <= la
        if rc == 0:
            assert not meet, (a, b)
            accepted += 1
            accepted_interleaved += not apart
        else:
            assert bad == 0 and not apart, (a, b)                       # hulls that do not overlap are never refused
            refused += 1
        assert csa.check_slices([BASE, BASE], [ROOM, ROOM], [a, b], disjoint=False) == (0, None)
    assert accepted_interleaved >= 20 and refused >= 100 and accepted >= 100, (accepted, accepted_interleaved, refused)


def test_check_slices_constructed_pairs(csa):
    def check(slices, ptrs=None, sizes=None, excl=(0, 0), disjoint=True):
        n = len(slices)
        return csa.check_slices(ptrs or [BASE] * n, sizes or [ROOM] * n, slices, excl=excl, disjoint=disjoint)
    bounds = [0, 1, 16, 33, 160, 400, 417, 999, 1000]
    blocks = [(c0, c1 - c0, 1000, 200) for c0, c1 in zip(bounds, bounds[1:])]
    assert check(blocks) == (0, None), "eight column blocks of one matrix"
    assert check(blocks[::-1]) == (0, None)
    assert check([(0, 17, 1000, 200), (500, 3, 1000, 200), (16, 17, 1000, 200)]) == (-1, 0), "two blocks sharing one column"
    assert check([(500, 3, 1000, 200), (16, 17, 1000, 200), (0, 17, 1000, 200)]) == (-1, 1), "... both are refused"
    assert check([(0, 400, 1000, 200), (400, 600, 600, 1)]) == (0, None), "a byte range inside one gap"
    assert check([(400, 600, 600, 1), (0, 400, 1000, 200)]) == (0, None)
    assert check([(0, 400, 1000, 200), (3400, 600, 0, 1)]) == (0, None), "... of a later row; count == 1 ignores its stride"
    assert check([(0, 400, 1000, 200), (400, 601, 601, 1)]) == (-1, 0), "one byte longer than the gap"
    assert check([(0, 400, 1000, 200), (399, 601, 601, 1)]) == (-1, 0)
    assert check([(0, 10, 100, 5), (50, 10, 101, 5)]) == (-1, 0), "unequal strides with overlapping hulls"
    assert check([(0, 10, 100, 5), (410, 10, 101, 5)]) == (0, None), "... with hulls that only touch"
    assert check([(0, 100, 100, 1), (99, 10, 10, 1)]) == (-1, 0), "two byte ranges that overlap"
    assert check([(0, 100, 100, 1), (100, 10, 10, 1)]) == (0, None), "... that touch"
    assert check([(0, 100, 100, 1), (99, 10, 10, 1)], disjoint=False) == (0, None)
    # the range none may overlap
    s = (7, 400, 1000, 3)                                              # hull [BASE + 7, BASE + 2407)
    assert check([s], excl=(BASE + 2407, 100)) == (0, None), "a hull touching excl"
    assert check([s], excl=(BASE, 7)) == (0, None)
    assert check([s], excl=(BASE + 500, 1)) == (-1, 0), "a hull whose gap byte lies in excl"
    assert check([(0, 1, 1, 1), s], excl=(BASE + 2406, 1), disjoint=False) == (-1, 1)
    # what the slice itself is refused for, in a buffer of sizes[i] bytes
    assert check([s], sizes=[2407]) == (0, None) and check([s], sizes=[2406]) == (-1, 0)
    assert check([(1, 0, 5, 3)]) == (-1, 0), "run == 0 with count > 0"
    assert check([(1, 1000, 999, 6)]) == (-1, 0), "stride < run with count > 1"
    assert check([(1, 1, 1 << 62, 5)], sizes=[M64 - 1]) == (-1, 0), "(count - 1) * stride wraps"
    assert check([(M64 - 8, 1, 8, 2)], sizes=[M64 - 1]) == (-1, 0), "offset + hull wraps"
    assert check([(8, 1, 8, 2)], ptrs=[M64 - 16], sizes=[32]) == (-1, 0), "the hull's address wraps"
    assert check([(0, 8, 8, 1)], ptrs=[M64 - 8], sizes=[8]) == (0, None), "a hull that ends at 2^64 does not"
    assert check([(0, 0, 0, 0), s], ptrs=[0, BASE]) == (0, None), "count == 0 selects nothing and may be NULL"
    assert check([s, (0, 4, 4, 1)], ptrs=[BASE, 0]) == (-1, 1), "a NULL buffer with count > 0"
    assert csa.lib().CSAMI_CheckSlices(None, None, None, 0, None, 0, 1, None) == 0
    bad = C.c_uint32(77)
    assert csa.lib().CSAMI_CheckSlices(None, None, None, 2, None, 0, 1, C.byref(bad)) == -1 and bad.value == 0


# ---- 3. the kernels' text on the CPU --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devspread") / "csa_dev_spread_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_spread_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=900)
    return run


def test_spread_sum_and_compare_rows_under_the_sanitizers(model):
    """11 runs x 4 gaps x 7 lengths x the phases that put a run border into the head, a unit and the tail x 16 source alignments x
    up to 16 hull alignments, sources exactly as large as the piece and buffers exactly as large as the hull; differences planted at
    every position class and in bytes that are not the entry's; fragments of three pieces end to end"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    word, count = out.stdout.split()
    assert word == "ok" and int(count) > 200000


@pytest.mark.parametrize("plant,how,where", [
    # the run border one byte late: the first piece with a unit and a gap -- its second byte goes to a gap byte
    (13, "FAIL", "spread sa=0 da=0 n=16 run=1 gap=1 r0=0"),
    # phase dropped from a thread's first unit: the first piece with a unit that does not begin at a run's start
    (14, "FAIL", "spread sa=0 da=0 n=16 run=3 gap=0 r0=2"),
    # a unit across a run border stored whole: the first piece with a unit and a gap
    (15, "FAIL", "spread sa=0 da=0 n=16 run=1 gap=1 r0=0"),
    # the row not advanced on the carry: a thread's SECOND unit (more than 256 units: 16383 bytes), under the first run that does
    # not divide the workgroup's step of 4096 positions
    (16, "FAIL", "spread sa=0 da=0 n=16383 run=3 gap=0 r0=2"),
    # the load window checked against the front of the hull only: the first unit that lies inside one run, is misaligned and ends
    # with the hull; the sanitizer sees the load
    (17, "AT", "rows sa=15 da=1 n=17 run=16 gap=0 r0=15"),
    # the head bytes summed and not compared: the first piece with a head whose differences are planted
    (18, "FAIL", "diff byte 0 sa=1 da=4 n=15 run=1 gap=0 r0=0"),
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, how, where):
    out = model(plant)
    assert out.returncode != 0
    if how == "FAIL":
        assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
    else:
        named = [l for l in out.stderr.splitlines() if l.startswith("AT ")]
        assert named[-1] == f"AT {where}" and "heap-buffer-overflow" in out.stderr and "csa_dev_read.h" in out.stderr
