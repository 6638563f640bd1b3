"""CPU tier for the early stop of the device-resident read (CSCMI_DecodeDeviceBatchStop, CSAMI_DeviceReadStop,
CSAMI_PlanDeviceStops): the declarations, the exports, the ctypes mirrors, the refusal without a device, and the host-only
planner against a plan written here in plain Python over oracle/orc_csa.py -- on archives the oracle container writes and on
crafted indices."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import cases
import csa_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

NEW = ["CSCMI_DecodeDeviceBatchStop", "CSAMI_DeviceReadStop", "CSAMI_PlanDeviceStops"]
STOP_FIELDS = ["decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csc_mi355x.h"\n#include "csa_mi355x.h"\n'
                   "int main(void){ CSCMIDevDecode j; CSCMIDevDecodeOpts o; CSCMIDevDecodeStats s; uint64_t stop = UINT64_MAX;\n"
                   "  CSADevArchive *a = 0; CSADevFile f; CSADevReadStats rs; CSADevStopStats ss; uint32_t nt = 0; uint64_t b = 0, p = 0, r = 0;\n"
                   "  const uint8_t raw[8] = {0};\n"
                   "  j.rc = 0; j.props.dict_size = 0; j.src = 0; j.src_size = 0; j.dst = 0; j.dst_cap = 0; j.produced = j.consumed = 0;\n"
                   "  o.launch_bytes = 0; s.launches = s.rounds = 0; s.kernel_ms = 0; f.name = 0; rs.tasks = 0;\n"
                   "  ss.decoded_bytes = ss.task_raw_bytes = ss.scratch_bytes = ss.stopped_tasks = 0;\n"
                   "  return CSCMI_DecodeDeviceBatchStop(0, &j, &stop, &o, &s) + CSAMI_DeviceReadStop(a, 0, 0, 0, 0, 0, &f, 1, &rs, &ss)\n"
                   "       + CSAMI_PlanDeviceStops(raw, 8, 24, 0, 0, &b, &p, &r, 1, &nt) + (int)ss.stopped_tasks; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in NEW if s not in have] == []


def test_ctypes_mirrors_have_the_c_layout(tmp_path, csa):
    from csc_amd import device
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csc_mi355x.h"\n#include "csa_mi355x.h"\nint main(void){ printf("%zu", sizeof(CSADevStopStats));\n'
                   + "".join(f'  printf(" %zu", offsetof(CSADevStopStats, {n}));\n' for n in STOP_FIELDS)
                   + '  printf(" %zu %zu %zu %zu\\n", sizeof(CSCMIDevDecode), sizeof(CSCMIDevDecodeOpts), sizeof(CSCMIDevDecodeStats), sizeof(CSADevReadStats));\n'
                   + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = csa.CSADevStopStats
    assert [n for n, _ in S._fields_] == STOP_FIELDS
    assert got[:5] == [C.sizeof(S)] + [getattr(S, n).offset for n in STOP_FIELDS] == [32, 0, 8, 16, 24]
    # the structs the new calls share with the old ones are what they were
    assert got[5:] == [C.sizeof(device.CSCMIDevDecode), C.sizeof(device.CSCMIDevDecodeOpts), C.sizeof(device.CSCMIDevDecodeStats),
                       C.sizeof(csa.CSADevReadStats)] == [96, 8, 24, 80]


def test_no_gpu_means_no_stopped_decode(prod, csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from csc_amd import device
    fn = device.bind_stop(prod)
    assert fn(0, None, None, None, None) == 0                               # nothing to do is not an error
    dst = (C.c_uint8 * 64)(*([0xA5] * 64))
    jobs = (device.CSCMIDevDecode * 3)()
    for j in jobs:
        j.props = prod.props_init(1 << 20, 3)
        j.src = 0x1000; j.src_size = 100; j.dst = C.addressof(dst); j.dst_cap = 64
        j.rc = 77; j.produced = 5; j.consumed = 6
    stats = device.CSCMIDevDecodeStats(11, 12, 13.0)
    stops = (C.c_uint64 * 3)(0, 10, device.NO_STOP)
    for s in (stops, None):
        assert fn(3, jobs, s, None, C.byref(stats)) == device.CSCMI_DEVICE_ERROR, "there is no CPU fallback"
        assert [(j.rc, j.produced, j.consumed) for j in jobs] == [(77, 5, 6)] * 3
        assert bytes(dst) == b"\xa5" * 64 and (stats.launches, stats.rounds, stats.kernel_ms) == (11, 12, 13.0)
    # the archive call: refused before it looks at its handle, and nothing of the caller's is touched
    files = (csa.CSADevFile * 2)()
    for f in files:
        f.offset = 7; f.size = 8; f.nfrags = 9; f.failed_frags = 10
    st = csa.CSADevReadStats(tasks=1, frags=2, waves=3, launches=4, decode_launches=5, readback_bytes=6, raw_bytes=7, verify_failures=8)
    ss = csa.CSADevStopStats(21, 22, 23, 24)
    for handle in (None, C.c_void_p(0x1234)):
        rc = csa.lib().CSAMI_DeviceReadStop(handle, None, 0, C.addressof(dst), 64, None, files, 2, C.byref(st), C.byref(ss))
        assert rc == csa.CSCMI_DEVICE_ERROR
        assert [(f.offset, f.size, f.nfrags, f.failed_frags) for f in files] == [(7, 8, 9, 10)] * 2
        assert (st.tasks, st.frags, st.waves, st.launches, st.decode_launches, st.readback_bytes, st.raw_bytes, st.verify_failures) == (1, 2, 3, 4, 5, 6, 7, 8)
        assert (ss.decoded_bytes, ss.task_raw_bytes, ss.scratch_bytes, ss.stopped_tasks) == (21, 22, 23, 24)
        assert bytes(dst) == b"\xa5" * 64


# ---- 2. the planner against a plain-Python plan -------------------------------------------------------------------------

SIX = {"s/a.bin": [["text", 71, 0, 150000]], "s/b.bin": [["exe", 72, 0, 100000]], "s/c.bin": [["delta", 73, 0, 120000]],
       "s/d.bin": [["random", 74, 0, 100000]], "s/e.bin": [["zeros", 110000]], "s/f.bin": [["entropy8", 75, 0, 100001]]}
TREES = {
    # six files of one extension: one task of several runs
    "six": (SIX, ["s"], {"level": 1, "dict_size": 256 << 10, "recurse": True}),
    # one file cut into three tasks (csarc -p3: slices of 1 MiB + 4, the least there is)
    "split3": ({"one.dat": [["text", 76, 0, 600000], ["zeros", 1600003]]}, ["one.dat"], {"level": 1, "dict_size": 256 << 10, "split_count": 3}),
}
SELECTIONS = {"six": [[], ["s/a.bin"], ["s/f.bin"], ["s/c.bin", "s/b.bin"], ["s"], ["nothing"]],
              "split3": [[], ["one.dat"]],
              "mixed_tree": [[], ["d/a.txt"], ["d/b.txt"], ["d/empty"], ["d/sub"], ["d/empty", "d/noext"]],
              "no_data": [[], ["e/one"]]}


def write_tree(root, files):
    for rel, parts in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path) or root, exist_ok=True)
        with open(path, "wb") as f:
            f.write(cases.build(parts))
        os.chmod(path, 0o644)
        os.utime(path, (csa_cases.MTIME, csa_cases.MTIME))


@pytest.fixture(scope="module")
def archives(orc, zalloc, tmp_path_factory):
    """{case: (archive size, raw index bytes, parsed index)}, written by the oracle container with the oracle encoder"""
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
        for case in ("six", "split3", "mixed_tree", "no_data"):
            d = tmp_path_factory.mktemp(case)
            if case in TREES:
                files, args, opts = TREES[case]
                write_tree(str(d), files)
            else:
                csa_cases.make_tree(str(d), case)
                args, opts = csa_cases.CSA_CASES[case]["args"], csa_cases.CSA_CASES[case]["opts"]
            os.chdir(d)
            arc = orc_csa.create(csa_cases.ARCNAME, args, encode=enc, **opts)
            info = orc_csa.parse(arc, dec)
            out[case] = (len(arc), info["index_raw"], info["index"])
    finally:
        os.chdir(cwd)
    return out


def python_stops(index, names):
    """include/csa_mi355x.h restated: the tasks that hold a selected fragment of non-zero size, largest sum of those first (equal
    sums by bid); stop = max(posblock + size) over the selected ones, raw over all of the bid"""
    raw, stop, total = {}, {}, {}
    for name, e in index.items():
        sel = orc_csa.isselected(list(names), name)
        for f in e["frags"]:
            raw[f["bid"]] = max(raw.get(f["bid"], 0), f["posblock"] + f["size"])
            if sel and f["size"]:
                stop[f["bid"]] = max(stop.get(f["bid"], 0), f["posblock"] + f["size"])
                total[f["bid"]] = total.get(f["bid"], 0) + f["size"]
    return [{"bid": b, "stop": stop[b], "raw": raw[b]} for b in sorted(total, key=lambda b: (-total[b], b))]


@pytest.mark.parametrize("case", list(SELECTIONS))
def test_planner_equals_the_plain_python_plan(csa, archives, case):
    arc_size, raw_index, index = archives[case]
    for names in SELECTIONS[case]:
        rc, tasks = csa.plan_device_stops(raw_index, arc_size, names)
        assert rc == 0 and tasks == python_stops(index, names), (case, names)
        assert all(0 < t["stop"] <= t["raw"] for t in tasks)
        # the same tasks, in the same order, as the layout planner lists raw sizes for
        assert [t["raw"] for t in tasks] == csa.plan_device_layout(raw_index, arc_size, names)[3]


def test_planned_stops_of_the_named_selections(csa, archives):
    arc_size, raw_index, index = archives["six"]
    plan = lambda names: csa.plan_device_stops(raw_index, arc_size, names)[1]      # noqa: E731
    (whole,) = plan([])
    assert whole["stop"] == whole["raw"] == sum(len(cases.build(p)) for p in SIX.values())     # no selection: every stop is the raw size
    by_pos = sorted(SIX, key=lambda n: index[n]["frags"][0]["posblock"])
    first, last = by_pos[0], by_pos[-1]
    (t,) = plan([first])
    f = index[first]["frags"][0]
    assert f["posblock"] == 0 and t["stop"] == f["size"] < t["raw"]               # the first file of the task: its fragment's end
    (t,) = plan([last])
    assert t["stop"] == t["raw"]                                                   # the last file: the whole task
    (t,) = plan([by_pos[1], by_pos[2]])
    f = index[by_pos[2]]["frags"][0]
    assert t["stop"] == f["posblock"] + f["size"] < t["raw"]
    assert plan(["nothing"]) == []
    # a file split over tasks: every slice's task is decoded to its end, and that is the task's raw size
    arc_size, raw_index, index = archives["split3"]
    tasks = csa.plan_device_stops(raw_index, arc_size, ["one.dat"])[1]
    assert len(tasks) == 3 == len(index["one.dat"]["frags"]) and all(t["stop"] == t["raw"] for t in tasks)
    assert sorted(t["stop"] for t in tasks) == [2200003 - 2 * 1048580, 1048580, 1048580]
    # only empty files or directories: no task
    arc_size, raw_index, index = archives["mixed_tree"]
    assert csa.plan_device_stops(raw_index, arc_size, ["d/empty"]) == (0, [])
    assert len(csa.plan_device_stops(raw_index, arc_size, ["d/empty", "d/noext"])[1]) == 1
    arc_size, raw_index, index = archives["no_data"]
    assert csa.plan_device_stops(raw_index, arc_size, []) == (0, [])


# ---- 3. crafted indices -----------------------------------------------------------------------------------------------

def _index(entries, blocks):
    """entries: [(name, [(bid, posblock, size, posfile)])]; blocks: {bid: [(off, size)]}"""
    index = {n: {"edate": 20231114221320, "esize": 1, "eattr": 0, "frags": [{"bid": b, "checksum": 0, "posblock": pb, "size": sz, "posfile": pf}
                                                                          for b, pb, sz, pf in fr]} for n, fr in entries}
    return orc_csa.pack_index(index, blocks, "out.csa")


M64 = 1 << 64
CRAFTED = {
    "a fragment size near 2^64": _index([("a", [(0, 0, M64 - 8, 0)])], {0: [(24, 100)]}),
    "posblock + size wraps": _index([("a", [(0, M64 - 16, 32, 0)])], {0: [(24, 100)]}),
    "posblock + size wraps in a file that is not selected": _index([("a", [(0, 0, 32, 0)]), ("b", [(0, M64 - 16, 32, 0)])], {0: [(24, 100)]}),
    "posfile + size wraps": _index([("a", [(0, 0, 32, M64 - 16)])], {0: [(24, 100)]}),
    "an archive block past arc_size": _index([("a", [(0, 0, 32, 0)])], {0: [(24, 100), (4000, 97)]}),
    "an archive block whose end wraps": _index([("a", [(0, 0, 32, 0)])], {0: [(M64 - 4, 8)]}),
}


@pytest.mark.parametrize("what", list(CRAFTED))
def test_crafted_index_is_refused(csa, what):
    assert csa.plan_device_stops(CRAFTED[what], 4096, [])[0] == -1
    assert csa.plan_device_stops(CRAFTED[what], 4096, ["a"])[0] == -1
    for cut in (0, 3, 7, len(CRAFTED[what]) - 9):                                       # and a truncated buffer never parses
        assert csa.plan_device_stops(CRAFTED[what][:cut], 4096, [])[0] == -1


def test_crafted_tasks_shared_and_split(csa):
    """a task two files share with a hole between them, a file whose fragments lie in two tasks (what task_bytes makes), an empty
    fragment behind everything: the stop is the end of the last SELECTED fragment of non-zero size, whatever else the task holds"""
    idx = _index([("a", [(0, 0, 100, 0), (1, 0, 50, 100)]), ("b", [(0, 300, 40, 0)]), ("c", [(1, 50, 10, 0)]), ("z", [(0, 5000, 0, 0)])],
                 {0: [(24, 100)], 1: [(124, 100)]})
    plan = lambda names: csa.plan_device_stops(idx, 4096, names)      # noqa: E731
    assert plan([]) == (0, [{"bid": 0, "stop": 340, "raw": 5000}, {"bid": 1, "stop": 60, "raw": 60}])
    assert plan(["a"]) == (0, [{"bid": 0, "stop": 100, "raw": 5000}, {"bid": 1, "stop": 50, "raw": 60}])
    assert plan(["b"]) == (0, [{"bid": 0, "stop": 340, "raw": 5000}])
    assert plan(["c", "z"]) == (0, [{"bid": 1, "stop": 60, "raw": 60}])
    assert plan(["z"]) == (0, [])
    # room for fewer entries than there are tasks: the count is still reported, nothing behind `cap` is written
    buf = (C.c_uint8 * len(idx)).from_buffer_copy(idx)
    stops = (C.c_uint64 * 2)(77, 77)
    nt = C.c_uint32()
    assert csa.lib().CSAMI_PlanDeviceStops(buf, len(idx), 4096, None, 0, None, stops, None, 1, C.byref(nt)) == 0
    assert nt.value == 2 and list(stops) == [340, 77]
