"""CPU tier for the device archive update (include/csa_mi355x.h: CSAMI_DeviceUpdate, CSAMI_PlanDeviceUpdate): the declarations, the
exports, the ctypes mirrors, the refusal without a device, the candidate step against a plain-Python restatement of its rule over
the oracle-built archives and over crafted indices, and the text k_frag_rows runs for a piece without a destination
(csc_amd/csrc/csa_dev_write.h: gather_sum<PLANT, false>) compiled for the host with the sanitizers and run as a program of its own
(tests/model/csa_dev_sum_only_model.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import csa_cases
import csa_write_cases
from test_archive_device_host import archives  # noqa: F401  (the fixture: every CPU case as the oracle container writes it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

NEW = ["CSAMI_DeviceUpdate", "CSAMI_PlanDeviceUpdate"]
NO_BID = (1 << 64) - 1


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
                   "  const void *p[1] = {0}; unsigned char arc[64]; const uint8_t raw[8] = {0}; uint64_t bids[2]; uint32_t nt = 0, nc = 0;\n"
                   "  f.name = 0; CSA_OptionsInit(&o);\n"
                   "  u.candidates = u.reused_tasks = u.encoded_tasks = u.reused_raw_bytes = u.reused_stream_bytes = u.encoded_raw_bytes = 0;\n"
                   "  u.checked_bytes = u.decoded_bytes = u.check_waves = u.check_launches = u.decode_launches = 0;\n"
                   "  u.check_kernel_ms = u.seconds_check = 0; t[0].base_bid = UINT64_MAX; t[0].status = CSA_UPD_NEW; t[0].reserved = 0;\n"
                   "  t[1].status = CSA_UPD_REUSED + CSA_UPD_PROPS + CSA_UPD_CHANGED + CSA_UPD_BASE_BAD;\n"
                   "  if (CSAMI_PlanDeviceUpdate(raw, 8, 24, &f, 1, &o, bids, 2, &nt, &nc)) return 1;\n"
                   '  return CSAMI_DeviceUpdate(0, p, 0, 0, &f, 1, "a.csa", arc, sizeof(arc), CSAMI_UPDATE_TRUST_SUMS, &o, &s, &g, &u, t, 2); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in NEW if s not in have or s not in csa.SYMBOLS] == []


def test_ctypes_mirrors_have_the_c_layout(tmp_path, csa):
    pairs = [("CSADevUpdateTask", csa.CSADevUpdateTask, 16), ("CSADevUpdateStats", csa.CSADevUpdateStats, 104)]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   + "".join(f'  printf(" %zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in T._fields_)
                             for name, T, _ in pairs) + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, T, size in pairs:
        assert C.sizeof(T) == size
        want += [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]
    assert got == want
    assert set(csa.CSADevUpdateStats().as_dict()) == {n for n, _ in csa.CSADevUpdateStats._fields_}
    assert csa.CSADevUpdateTask().as_dict() == {"base_bid": 0, "status": 0}


def test_no_gpu_means_no_update(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    name = C.create_string_buffer(b"a")
    f = csa.CSADevFile()
    f.name, f.esize, f.offset, f.size, f.nfrags = C.cast(name, C.c_void_p), 4, 77, 78, 79
    before = bytes(f)
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    ptrs = (C.c_void_p * 1)(C.addressof(buf) + 1024)
    st, gs, us, tasks = csa.CSADevWriteStats(), csa.CSADevGatherStats(), csa.CSADevUpdateStats(), (csa.CSADevUpdateTask * 2)()
    for t in (st, gs, us, tasks):
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    o = csa.options()
    # (the base handle is not looked at either: the refusal comes first)
    assert L.CSAMI_DeviceUpdate(C.c_void_p(0x1234), ptrs, None, None, C.byref(f), 1, b"a.csa", C.addressof(buf) + 2048, 1024,
                                csa.CSAMI_UPDATE_TRUST_SUMS, C.byref(o), C.byref(st), C.byref(gs), C.byref(us), tasks, 2) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096
    for t in (st, gs, us, tasks):
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. the candidate step against its rule in plain Python -----------------------------------------------------------------

def _edate(csa):
    return int(csa.lib().CSA_DecimalTime(csa_cases.MTIME))


def python_candidates(base_index, files, split_count):
    """the candidate rule of include/csa_mi355x.h restated, every task against every task: a task of the new plan is a candidate for
    base task b when it holds a byte and the set of its fragments (name, offset, size, posblock) is the set of ALL fragments of
    the base index with bid b -> [bid or NO_BID per task of the new plan]"""
    base = {}
    for name, e in base_index.items():
        for f in e["frags"]:
            base.setdefault(f["bid"], []).append((name, f["posfile"], f["size"], f["posblock"]))
    index = {f["name"]: {"esize": f["esize"], "edate": f["edate"], "eattr": f["eattr"], "ext": b"\0\0\0\0", "frags": []} for f in files}
    out = []
    for t in orc_csa.plan_tasks(index, max(split_count, 1)):
        mine, pos = [], 0
        for name, off, size in t["files"]:
            mine.append((name, off, size, pos))
            pos += size
        hit = [b for b, theirs in base.items() if t["total"] and sorted(theirs) == sorted(mine)]
        out.append(hit[0] if hit else NO_BID)
    return out


def _opts(case, **more):
    o = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k in ("level", "dict_size", "split_count")}
    o.update(more)
    return o


def _check(csa, arch, files, opts, what):
    size, raw, index, _ = arch
    want = python_candidates(index, files, opts.get("split_count", 1))
    rc, bids, nc = csa.plan_device_update(raw, size, files, **opts)
    assert (rc, bids, nc) == (0, want, sum(b != NO_BID for b in want)), what
    return bids


@pytest.mark.parametrize("case", csa_cases.CPU_CASES)
def test_the_unchanged_table_makes_every_task_its_own_candidate(csa, archives, case):  # noqa: F811
    files, _, _ = csa_write_cases.table(case, _edate(csa), with_bytes=False)
    bids = _check(csa, archives[case], files, _opts(case), case)
    assert bids == list(range(len(bids))), "one worker wrote the base: its bids are the plan's ids"
    _check(csa, archives[case], files[::-1], _opts(case), "the order of the table does not matter")


def test_tables_that_differ_from_the_base(csa, archives):  # noqa: F811
    files, _, _ = csa_write_cases.table("mixed_tree", _edate(csa), with_bytes=False)
    opts, arch = _opts("mixed_tree"), archives["mixed_tree"]
    assert _check(csa, arch, files, opts, "unchanged") == [0, 1, 2]                       # {a.txt, b.txt}, {c.exe}, {empty, noext, e.dat}

    def edit(which, **kw):
        return [dict(f, **kw) if f["name"] == which else f for f in files]
    # one size changed: the txt task is 100000 + 70000 bytes now and sorts behind the exe task
    assert _check(csa, arch, edit("d/a.txt", esize=100000), opts, "a size") == [1, NO_BID, 2]
    assert _check(csa, arch, edit("d/b.txt", esize=70001), opts, "a size, one byte") == [NO_BID, 1, 2]
    added = files + [{"name": "d/new.dat", "esize": 10, "edate": 1, "eattr": csa_write_cases.FILE_ATTR, "offset": 0}]
    assert _check(csa, arch, added, opts, "an entry added") == [0, 1, NO_BID]
    assert _check(csa, arch, [f for f in files if f["name"] != "d/noext"], opts, "an entry removed") == [0, 1, NO_BID]
    # d/b.txt -> d/b.exe: it leaves the txt group and joins the exe group
    assert _check(csa, arch, edit("d/b.txt", name="d/b.exe"), opts, "renamed across an extension group") == [NO_BID, NO_BID, 2]
    dated = [dict(f, edate=f["edate"] + 1, eattr=f["eattr"] ^ 0x100) for f in files]
    assert _check(csa, arch, dated, opts, "edate and eattr do not enter") == [0, 1, 2]


def test_another_split_of_a_single_file(csa, archives):  # noqa: F811
    files, _, _ = csa_write_cases.table("single_split3", _edate(csa), with_bytes=False)
    arch = archives["single_split3"]
    assert _check(csa, arch, files, _opts("single_split3"), "the base's own split") == [0, 1, 2]
    assert _check(csa, arch, files, _opts("single_split3", split_count=2), "-p2") == [NO_BID] * 2
    # -p4: slices of 1.25 MiB + 4 -- no fragment of it is one of the base's
    assert set(_check(csa, arch, files, _opts("single_split3", split_count=4), "-p4")) == {NO_BID}


def _crafted(entries, blocks):
    """raw index bytes: entries {name: (esize, [(bid, posblock, size, posfile)])}, blocks {bid: [(off, size)]}"""
    index = {n: {"edate": 1, "esize": es, "eattr": csa_write_cases.FILE_ATTR,
                 "frags": [{"bid": b, "checksum": 0, "posblock": pb, "size": sz, "posfile": pf} for b, pb, sz, pf in frags]}
             for n, (es, frags) in entries.items()}
    return orc_csa.pack_index(index, blocks, csa_cases.ARCNAME), index


def _row(name, esize):
    return {"name": name, "esize": esize, "edate": 1, "eattr": csa_write_cases.FILE_ATTR, "offset": 0}


def test_crafted_indices(csa):
    blocks = {0: [(24, 100)], 1: [(124, 50)]}
    table = [_row("a.txt", 100000), _row("b.txt", 70000)]                 # one task, the smaller file first: b.txt at 0, a.txt at 70000

    def run(entries, what, files=table, blk=blocks):
        raw, index = _crafted(entries, blk)
        want = python_candidates(index, files, 1)
        rc, bids, nc = csa.plan_device_update(raw, 4096, files)
        assert (rc, bids, nc) == (0, want, sum(b != NO_BID for b in want)), what
        return bids
    same = {"a.txt": (100000, [(0, 70000, 100000, 0)]), "b.txt": (70000, [(0, 0, 70000, 0)])}
    assert run(same, "the task as the base has it") == [0]
    more = dict(same, **{"c.txt": (5, [(0, 170000, 5, 0)])})
    assert run(more, "the base task has one fragment more than the new task") == [NO_BID]
    moved = {"a.txt": (100000, [(0, 0, 100000, 0)]), "b.txt": (70000, [(0, 100000, 70000, 0)])}
    assert run(moved, "equal names and sizes, another posblock") == [NO_BID]
    apart = {"a.txt": (100000, [(1, 70000, 100000, 0)]), "b.txt": (70000, [(0, 0, 70000, 0)])}
    assert run(apart, "the fragments lie in two base tasks") == [NO_BID]
    # zero-size fragments are members of the set: an empty entry in the base task that the table lacks, one that it has
    empty = dict(same, **{"e.txt": (0, [(0, 0, 0, 0)])})
    assert run(empty, "an empty entry of the base task that the table lacks") == [NO_BID]
    assert run(empty, "... and with it", files=[_row("e.txt", 0)] + table) == [0]
    assert run(same, "an empty entry the base task lacks", files=[_row("e.txt", 0)] + table) == [NO_BID]
    # a table of nothing but empty entries: its one task holds no byte and is no candidate
    assert run({"e.txt": (0, [(0, 0, 0, 0)])}, "no byte", files=[_row("e.txt", 0), _row("f.txt", 0)]) == []
    # what does not parse, and what CSAMI_PlanDeviceLayout refuses: -1
    raw, _ = _crafted(same, blocks)
    assert csa.plan_device_update(raw[:20], 4096, table)[0] == -1
    assert csa.plan_device_update(b"", 4096, table)[0] == -1
    assert csa.plan_device_update(raw, 123, table)[0] == -1, "an archive block outside the archive"
    wrap, _ = _crafted({"a.txt": (100000, [(0, (1 << 64) - 5, 100000, 0)])}, blocks)
    assert csa.plan_device_update(wrap, 4096, table)[0] == -1, "posblock + size wraps"
    assert csa.plan_device_update(raw, 4096, table + [_row("a.txt", 1)])[0] == -1, "a table the write refuses"


# ---- 3. the kernel's text on the CPU ----------------------------------------------------------------------------------------

LENS = [1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384]
PATTERNS = 11


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devsumonly") / "csa_dev_sum_only_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_sum_only_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


def test_the_form_that_only_sums_under_the_sanitizers(model):
    """16 source alignments x 13 lengths x 11 patterns (run 1, 15, 16, 17 and 4099 among them) out of sources exactly as large as
    their hulls, against the storing form and a byte-wise sum, a destination it is handed left untouched; fragments of three pieces
    end to end against a byte-wise adler32"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == f"ok {16 * len(LENS) * PATTERNS + 4 * 7 * 4}"


@pytest.mark.parametrize("plant,how,where", [
    # the tail bytes of the form that only sums dropped: the first case, one byte that is all tail
    (6, "FAIL", "sum sa=0 n=1 run=1 stride=2"),
    # the form that only sums still stores: the first case, whose one byte lands in the canary
    (7, "FAIL", "sum sa=0 n=1 run=1 stride=2"),
    # the load window not checked against the hull's end: the units are anchored on packed position 0, so the first piece whose
    # last unit is misaligned and ends with the hull is two rows of 16 a stride of 17 apart; the sanitizer sees the load
    (5, "AT", "sum sa=0 n=32 run=16 stride=17"),
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, how, where):
    out = model(plant)
    assert out.returncode != 0
    if how == "FAIL":
        assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
    else:
        named = [l for l in out.stderr.splitlines() if l.startswith("AT ")]
        assert named[-1] == f"AT {where}" and "heap-buffer-overflow" in out.stderr and "csa_dev_read.h" in out.stderr
