"""CPU tier for byte ranges and strided slices of entries (include/csa_mi355x.h: CSAMI_DeviceReadSlices, CSAMI_PlanDeviceSlices): the
declarations, the exports, the ctypes mirrors, the refusal without a device, the host planner over crafted indices against a
brute-force set of selected offsets written here in plain Python, and the text the planner and k_frag_slices run
(csc_amd/csrc/csa_dev_read.h: slice_check, slice_next, slice_reduce, slice_sum) compiled for the host with the sanitizers and run
as a program of its own (tests/model/csa_dev_slice_model.cpp)."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

TWO = ["CSAMI_DeviceReadSlices", "CSAMI_PlanDeviceSlices"]
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
                   "int main(void){ CSADevArchive *a = 0; CSADevFile f; CSADevReadStats s; CSADevStopStats ss; CSADevSliceStats sl; CSADevSlice c;\n"
                   "  void *p[1] = {0}; uint64_t n[1] = {0}, b = 0, st = 0, r = 0; uint32_t nt = 0, nf = 0; const uint8_t raw[8] = {0};\n"
                   "  c.offset = 0; c.run = 1; c.stride = 2; c.count = 3;\n"
                   "  sl.selected_bytes = sl.touched_bytes = sl.periodic_pieces = sl.plain_pieces = 0; f.name = 0;\n"
                   "  CSAMI_DeviceReadSlices(a, 0, 0, &c, p, n, 1, CSAMI_DEV_STOP_EARLY, 0, &f, &s, &ss, &sl);\n"
                   "  return CSAMI_PlanDeviceSlices(raw, 8, 24, 0, 0, &c, 1, &b, &st, &r, 1, &nt, &nf); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_two_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in TWO if s not in have] == []
    assert [s for s in TWO if s not in csa.SYMBOLS] == []


def test_ctypes_mirrors_have_the_c_layout(tmp_path, csa):
    types = [("CSADevSlice", csa.CSADevSlice), ("CSADevSliceStats", csa.CSADevSliceStats)]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   + "".join(f'  printf(" %zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in T._fields_)
                             for name, T in types) + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, T in types:
        want += [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]
    assert got == want and C.sizeof(csa.CSADevSlice) == 32


def test_no_gpu_means_no_sliced_read(csa):
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
    caps = (C.c_uint64 * 1)(8)
    sl = (csa.CSADevSlice * 1)()
    sl[0].offset, sl[0].run, sl[0].stride, sl[0].count = 1, 2, 3, 2
    sliced = bytes(sl)

    def marked(T):
        t = T()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        return t
    rs, ss, st = marked(csa.CSADevReadStats), marked(csa.CSADevStopStats), marked(csa.CSADevSliceStats)
    o = csa.options()
    # (no handle can exist without a device: the refusal has to come before the handle is looked at)
    assert L.CSAMI_DeviceReadSlices(None, None, 0, sl, ptrs, caps, 1, 1, C.byref(o), C.byref(f), C.byref(rs), C.byref(ss),
                                    C.byref(st)) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096 and bytes(sl) == sliced
    for t in (rs, ss, st):
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


def test_rows_slice():
    from csc_amd import csa
    assert csa.rows_slice(1000, 0, 200) == (0, 200000, 200000, 1)
    assert csa.rows_slice(1000, 19, 21) == (19000, 2000, 2000, 1), "a full-width block is one byte range"
    assert csa.rows_slice(1000, 199, 200, 3, 20) == (199003, 17, 17, 1), "and so is a block of one row"
    assert csa.rows_slice(1000, 19, 21, 496, 512) == (19496, 16, 1000, 2)
    assert csa.rows_slice(1000, 0, 200, 999) == (999, 1, 1000, 200)
    for bad in ((1000, 3, 3), (1000, 0, 1, 5, 5), (1000, 0, 1, 0, 1001)):
        with pytest.raises(ValueError):
            csa.rows_slice(*bad)


# ---- 2. the planner over crafted indices ------------------------------------------------------------------------------------

def _index(entries, blocks):
    """entries: [(name, [(bid, posblock, size, posfile)])]; blocks: {bid: [(off, size)]}"""
    index = {n: {"edate": 20231114221320, "esize": 1, "eattr": 0, "frags": [{"bid": b, "checksum": 0, "posblock": pb, "size": sz, "posfile": pf}
                                                                          for b, pb, sz, pf in fr]} for n, fr in entries}
    return orc_csa.pack_index(index, blocks, "out.csa")


def _blocks(entries):
    return {b: [(24 + 16 * b, 16)] for b in sorted({f[0] for _, fr in entries for f in fr})}


def _selected(s):
    """the definition, byte by byte: the set of selected offsets"""
    if len(s) == 2:
        s = (s[0], s[1], s[1], 1)
    off, run, stride, count = s
    return {off + k * stride + j for k in range(count) for j in range(run)}


def python_plan(entries, slices):
    """touched fragments, and the tasks [(bid, stop, raw)] in decode order, from sets of selected offsets"""
    raw, tasks, touched = {}, {}, 0
    for _, fr in entries:
        for b, pb, sz, pf in fr:
            raw[b] = max(raw.get(b, 0), pb + sz)
    for name, fr in sorted(entries):
        sel = _selected(slices[name]) if name in slices else set()
        for b, pb, sz, pf in fr:
            if sz and sel & set(range(pf, pf + sz)):
                touched += 1
                t = tasks.setdefault(b, {"total": 0, "stop": 0})
                t["total"] += sz
                t["stop"] = max(t["stop"], pb + sz)
    order = sorted(tasks, key=lambda b: (-tasks[b]["total"], b))
    return touched, [(b, tasks[b]["stop"], raw[b]) for b in order]


def _plan(csa, entries, slices, names=()):
    rc, tasks, touched = csa.plan_device_slices(_index(entries, _blocks(entries)), 4096, slices, names)
    return rc, touched, [(t["bid"], t["stop"], t["raw"]) for t in tasks]


def _random_entry(rng, posblock, ntasks):
    """an entry of up to 128 bytes in fragments of 1..40 bytes, dealt to tasks at random; now and then a hole, an empty fragment,
    fragments out of file order"""
    frags, pf = [], 0
    while pf < 128 and len(frags) < 12:
        sz = rng.randint(1, 40)
        if pf + sz > 128:
            break
        if rng.random() < 0.15:
            pf += rng.randint(1, 9)                                # a hole
            if pf + sz > 128:
                break
        b = rng.randrange(ntasks)
        frags.append((b, posblock[b], sz, pf))
        posblock[b] += sz
        pf += sz
        if rng.random() < 0.1:
            frags.append((b, posblock[b], 0, pf))                  # an empty fragment: never touched
    if rng.random() < 0.3:
        rng.shuffle(frags)
    return frags


def _random_slice(rng, size):
    while True:
        run, count = rng.randint(1, 40), rng.randint(1, 6)
        stride = run + rng.choice([0, 0, 1, 2, 7, 30, 45])
        span = (count - 1) * stride + run
        if span <= size:
            return (rng.randint(0, size - span), run, stride, count)


def test_planner_equals_the_brute_force_plan(csa):
    rng = random.Random(20240229)
    seen_untouched_task = 0
    for trial in range(150):
        ntasks = rng.randint(1, 4)
        posblock = [0] * ntasks
        entries = [(n, _random_entry(rng, posblock, ntasks)) for n in ("a", "b", "c")]
        entries = [(n, fr) for n, fr in entries if fr]
        slices = {}
        for n, fr in entries:
            size = max(pf + sz for _, _, sz, pf in fr)
            if n != "c" or trial % 3 == 0:                         # c mostly without a key: count == 0
                s = _random_slice(rng, size)
                slices[n] = s if trial % 5 else s[:2]              # every fifth trial: byte ranges, given as (offset, length)
        want_touched, want_tasks = python_plan(entries, slices)
        rc, touched, tasks = _plan(csa, entries, slices)
        assert (rc, touched, tasks) == (0, want_touched, want_tasks), (trial, entries, slices)
        seen_untouched_task += len({b for _, fr in entries for b, _, sz, _ in fr if sz}) > len(tasks)
    assert seen_untouched_task >= 20, "the trials must hold tasks that no slice touches"


# task 0 holds a's bytes [0, 10), [10, 20) and [30, 40) back to back, task 1 its bytes [20, 30) behind 5 bytes of b's
BORDER = [("a", [(0, 0, 10, 0), (0, 10, 10, 10), (1, 5, 10, 20), (0, 20, 10, 30)]), ("b", [(1, 0, 5, 0)])]


@pytest.mark.parametrize("what,slices,touched,tasks", [
    ("the last byte is the byte in front of a fragment", {"a": (0, 10)}, 1, [(0, 10, 30)]),
    ("the first byte is a fragment's last", {"a": (9, 5)}, 2, [(0, 20, 30)]),
    ("the first byte is a fragment's last, alone", {"a": (9, 1)}, 1, [(0, 10, 30)]),
    ("a stride steps over whole fragments; a later one of the task raises its stop", {"a": (2, 3, 30, 2)}, 2, [(0, 30, 30)]),
    ("the same first row alone: the untouched fragments behind it do not", {"a": (2, 3)}, 1, [(0, 10, 30)]),
    ("a stride steps over a task", {"a": (12, 2, 20, 2)}, 2, [(0, 30, 30)]),
    ("the hull of that slice as a range", {"a": (12, 22)}, 3, [(0, 30, 30), (1, 15, 15)]),
    ("count == 0", {"a": (3, 0, 0, 0)}, 0, []),
    ("no key at all", {}, 0, []),
    ("stride == run", {"a": (5, 5, 5, 5)}, 3, [(0, 20, 30), (1, 15, 15)]),
    ("two entries, one task stopped by the other's fragment", {"a": (25, 1), "b": (4, 1)}, 2, [(1, 15, 15)]),
    ("the second entry alone: the task stops behind it", {"b": (0, 5)}, 1, [(1, 5, 15)]),
])
def test_planner_at_the_borders(csa, what, slices, touched, tasks):
    assert python_plan(BORDER, slices) == (touched, tasks), "the expectation is the brute-force plan's"
    assert _plan(csa, BORDER, slices) == (0, touched, tasks)


def test_planner_with_a_hole_and_fragments_out_of_file_order(csa):
    holed = [("a", [(0, 10, 10, 20), (0, 0, 10, 0)])]                         # listed back to front; nothing covers [10, 20)
    assert _plan(csa, holed, {"a": (8, 14)}) == (0, 2, [(0, 20, 20)])
    assert _plan(csa, holed, {"a": (10, 10)}) == (0, 0, []), "a slice inside the hole lies inside the entry and touches nothing"
    assert _plan(csa, holed, {"a": (19, 2)}) == (0, 1, [(0, 20, 20)]), "the fragment that comes first in the index lies last in the file"
    assert _plan(csa, holed, {"a": (9, 1)}) == (0, 1, [(0, 10, 20)])
    for s in ({"a": (8, 14)}, {"a": (10, 10)}, {"a": (19, 2)}, {"a": (0, 1, 29, 2)}):
        assert _plan(csa, holed, s)[1:] == python_plan(holed, s)


def test_a_selection_takes_its_slices_in_plan_order(csa):
    assert _plan(csa, BORDER, {"b": (0, 5)}, names=["b"]) == (0, 1, [(1, 5, 15)])
    with pytest.raises(KeyError):
        _plan(csa, BORDER, {"a": (0, 1)}, names=["b"])
    with pytest.raises(KeyError):
        _plan(csa, BORDER, {"nothing": (0, 1)})


REFUSED = {
    "run == 0": (0, 0, 1, 1),
    "run == 0, several rows": (0, 0, 4, 3),
    "stride < run": (0, 4, 3, 2),
    "offset + run wraps": (M64 - 1, 2, 2, 1),
    "(count - 1) * stride wraps": (0, 1, 1 << 62, 5),
    "(count - 1) * stride + run wraps": (0, 2, M64 - 1, 2),
    "offset + span wraps": (M64 - 8, 1, 8, 2),
    "the last selected byte at size": (39, 2),
    "the first selected byte at size": (40, 1),
    "the last row's last byte at size": (1, 10, 15, 3),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_planner_refuses_the_slice(csa, what):
    s = REFUSED[what]
    assert _plan(csa, BORDER, {"a": s})[0] == -1
    ok = {"the last selected byte at size": (38, 2), "the first selected byte at size": (39, 1), "the last row's last byte at size": (0, 10, 15, 3),
          "stride < run": (0, 4, 4, 2), "run == 0, several rows": (0, 0, 4, 0)}.get(what, (0, 1))
    assert _plan(csa, BORDER, {"a": ok})[0] == 0, "the index parses, and the slice next to the refused one is taken"


def test_planner_wants_one_slice_per_selected_entry(csa):
    L = csa.lib()
    raw = _index(BORDER, _blocks(BORDER))
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    sl = (csa.CSADevSlice * 3)()
    nt, nf = C.c_uint32(), C.c_uint32()
    for n, want in ((1, -1), (3, -1), (2, 0)):
        assert L.CSAMI_PlanDeviceSlices(buf, len(raw), 4096, None, 0, sl, n, None, None, None, 0, C.byref(nt), C.byref(nf)) == want
    assert L.CSAMI_PlanDeviceSlices(buf, len(raw), 4096, None, 0, None, 2, None, None, None, 0, C.byref(nt), C.byref(nf)) == -1


BAD_INDEX = {
    "a fragment size near 2^64": ([("a", [(0, 0, M64 - 8, 0)])], {0: [(24, 100)]}),
    "posblock + size wraps": ([("a", [(0, M64 - 16, 32, 0)])], {0: [(24, 100)]}),
    "posfile + size wraps": ([("a", [(0, 0, 32, M64 - 16)])], {0: [(24, 100)]}),
    "an archive block past arc_size": ([("a", [(0, 0, 32, 0)])], {0: [(24, 100), (4000, 97)]}),
    "an archive block whose end wraps": ([("a", [(0, 0, 32, 0)])], {0: [(M64 - 4, 8)]}),
}


@pytest.mark.parametrize("what", list(BAD_INDEX))
def test_planner_is_as_strict_as_the_stop_planner(csa, what):
    entries, blocks = BAD_INDEX[what]
    raw = _index(entries, blocks)
    assert csa.plan_device_stops(raw, 4096)[0] == -1
    L = csa.lib()
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    sl = (csa.CSADevSlice * 1)()
    sl[0].offset, sl[0].run, sl[0].stride, sl[0].count = 0, 1, 1, 1
    nt, nf = C.c_uint32(), C.c_uint32()
    assert L.CSAMI_PlanDeviceSlices(buf, len(raw), 4096, None, 0, sl, 1, None, None, None, 0, C.byref(nt), C.byref(nf)) == -1
    good = _index([("a", [(0, 0, 32, 0)])], {0: [(24, 100)]})
    gbuf = (C.c_uint8 * len(good)).from_buffer_copy(good)
    assert L.CSAMI_PlanDeviceSlices(gbuf, len(good), 4096, None, 0, sl, 1, None, None, None, 0, C.byref(nt), C.byref(nf)) == 0
    for cut in (0, 3, 7, len(good) - 70):                                      # and a truncated buffer never parses
        assert L.CSAMI_PlanDeviceSlices(gbuf, cut, 4096, None, 0, sl, 1, None, None, None, 0, C.byref(nt), C.byref(nf)) == -1


# ---- 3. the planner's and the kernel's text on the CPU ------------------------------------------------------------------------

BIG = [1, 2, 15, 16, 17, 16383, 16384, 16385, 1 << 31, 1 << 32, 1 << 63]
LENS = [1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384]
PATTERNS = [(1, 2), (1, 16), (3, 5), (15, 16), (16, 16), (16, 17), (17, 48), (100, 1000), (4096, 4097), (16384, 16384)]


def _model_cases():
    """the cases tests/model/csa_dev_slice_model.cpp runs, counted by its rules"""
    count = 0
    for run in BIG:
        for stride in BIG:
            if stride < run:
                continue
            rows = next(c for c in (3, 2, 1) if 5 + (c - 1) * stride + run < M64)
            for ln in (1, 16, 16384):
                for row in (0, rows - 1):                          # (one row: the same row twice, as the model walks it)
                    for kind in range(5):
                        if (kind == 0 and row) or (kind >= 3 and stride == run):
                            continue
                        r0 = [0, run // 2, run - 1, run + (stride - run) // 2, stride - 1][kind]
                        if kind and r0 > M64 - 1 - ln - (5 + row * stride):
                            continue
                        count += 1
    count += 13                                                    # slice_check's table
    cuts = sum(sum(lo < hi for lo, hi in ((0, n), (1, n - 1), (n // 3, n - n // 3))) for n in LENS)
    count += 16 * 16 * len(PATTERNS) * cuts
    return count + 4 * 7 * 4


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devslice") / "csa_dev_slice_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_slice_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


def test_slice_reduce_and_slice_sum_under_the_sanitizers(model):
    """every (run, stride) pair around the powers the reduction turns on x three spans x every phase class against the 64-bit
    definition; 16 x 16 alignments x 13 lengths x 10 patterns x three [lo, hi) of slice_sum; fragments of three pieces end to end"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == f"ok {_model_cases()}"


@pytest.mark.parametrize("plant,where", [
    # the run border one byte late: the first piece of all -- one byte, and (1, 2) at phase 1 puts it into the gap
    (9, "sum sa=0 da=0 n=1 run=1 stride=2 lo=0 hi=1"),
    # phase dropped from a thread's first unit: the first length with a unit, under the first pattern whose phase there, 16 % 5, is not 0
    (10, "sum sa=0 da=0 n=16 run=3 stride=5 lo=0 hi=16"),
    # a unit across a run border stored whole: the first length with a unit, under the first pattern
    (11, "sum sa=0 da=0 n=16 run=1 stride=2 lo=0 hi=16"),
    # the row not advanced on the carry: a thread's SECOND unit (more than 256 units: 16383 bytes), under the first pattern whose
    # stride does not divide the workgroup's step of 4096 positions
    (12, "sum sa=0 da=0 n=16383 run=3 stride=5 lo=0 hi=16383"),
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, where):
    out = model(plant)
    assert out.returncode != 0
    assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
