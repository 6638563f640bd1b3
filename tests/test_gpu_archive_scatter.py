"""GPU tier for the device archive over the caller's buffers (include/csa_mi355x.h: CSAMI_DeviceWriteFrom, CSAMI_DeviceReadInto,
CSAMI_DeviceCompare; csc_amd.csa.DeviceArchive.write_tensors / extract_into / compare): every entry in an allocation of its own,
at varying alignment.  A write from separate tensors must give the archive the contiguous write gives (and the reference's, where
a golden fixes it); a read into separate tensors must deliver what `extract` delivers and store nothing else; a comparison must
name exactly the entries that differ and the first byte at which they do, and write nothing at all.

`split_count` cuts only an archive of ONE non-empty entry, into slices of at least 1 MiB (csarc.cpp:516-547), so the ~200 KB entry of
plan "single" stays one task that is encoded where it lies; entries cut across tasks come from `task_bytes` (plan "fragmented")."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

import cases
import csa_cases
import csa_write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

EDGE_SIZES = [0, 1, 15, 16, 17, 4095, 16383, 16384, 16385, 32769, 70001]
OFFSETS = [0, 1, 3, 8, 15]                      # where an entry begins in its own allocation, in rotation
GUARD = 64
MiB = 1 << 20
GOLDEN_CASES = ["mixed_tree", "many_files", "single_split3", "single_split_many", "named_files_m3", "single_shadowed_by_empty",
                "single_after_empty", "no_data"]         # those of tests/test_gpu_archive_device_write.py


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "csa.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dec(orc, zalloc):
    def d(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw
    return d


def _edate(csa, t=csa_cases.MTIME):
    return int(csa.lib().CSA_DecimalTime(int(t)))


def _bytes(view):
    return view.cpu().numpy().tobytes()


def _upload(data, off=0):
    """the bytes in an allocation of their own, `off` bytes behind its start"""
    import torch
    buf = torch.empty(off + len(data) + 1, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + len(data)]
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _entries(table, content):
    """the rows of a contiguous table as entries with a tensor each (None for directories and empty files)"""
    return [{"name": f["name"], "edate": f["edate"], "eattr": f["eattr"],
             "tensor": _upload(content[f["name"]], OFFSETS[i % 5]) if f["esize"] else None} for i, f in enumerate(table)]


class Guarded:
    """n bytes between two guards of 0xA5, in an allocation of their own"""

    def __init__(self, n, off=0):
        import torch
        self.buf = torch.full((GUARD + off + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lo, self.n = GUARD + off, n
        self.view = self.buf[self.lo:self.lo + n]

    def guards_intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.lo + self.n:] == 0xA5).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all())


def _check_bus(st):
    """What crosses the bus (include/csa_mi355x.h), as tests/test_gpu_archive_device_write.py states it.  The encoder reads back 16
    bytes a stream a round; its rounds are bounded from the call's own stats: encode_launches counts, per CSCMI_EncodeDeviceBatch
    call, one flush kernel per stream, one framing launch per round and at least one encode launch per round but the last -- so
    encode_launches minus the streams (tasks, the index, the retries) is at least the rounds of all calls together."""
    tasks, frags = st["tasks"] + 1, st["frags"]                                      # the index stream counts as one task
    rounds = st["encode_launches"] - (tasks + st["retries"])
    print(f"bus: raw {st['raw_bytes']} readback {st['readback_bytes']} upload {st['upload_bytes']} rounds<= {rounds} tasks {tasks} "
          f"frags {frags} blocks {st['blocks']} launches {st['launches']} waves {st['waves']}")
    assert st["readback_bytes"] <= 16 * rounds * tasks + 8 * frags + 8 * (st["blocks"] + tasks) + 16
    tables = 24 * (st["raw_bytes"] // 16384 + frags) + 24 * frags + 32 * tasks + 24 * (st["archive_bytes"] // 65536 + 2 * tasks + 1)
    assert st["upload_bytes"] <= st["index_raw_size"] + 24 + 10 * tasks + tables
    assert st["launches"] <= 5 * st["waves"] + 2
    if st["raw_bytes"] >= MiB:
        assert st["readback_bytes"] < st["raw_bytes"] // 32 and st["upload_bytes"] < st["raw_bytes"] // 32


def _write_tensors(csa, entries, **kw):
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, **kw)
    if rc == 0:
        _check_bus(st)
        assert st["archive_bytes"] == arc.numel()
        assert [(f["size"], f["name"]) for f in st["files"]] == [(0 if e["tensor"] is None else e["tensor"].numel(), e["name"]) for e in entries]
    return rc, arc, st


SAME = ["tasks", "frags", "waves", "blocks", "launches", "encode_launches", "readback_bytes", "upload_bytes", "raw_bytes", "archive_bytes",
        "index_raw_size", "index_compressed_size", "n_entries", "retries"]


# ---- 1. goldens of the reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_write_is_the_reference_archivers(csa, golden, case):
    table, src, content = csa_write_cases.table(case, _edate(csa))
    opts = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}
    rc, arc, st = _write_tensors(csa, _entries(table, content), arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0
    assert hashlib.sha256(_bytes(arc)).hexdigest() == golden[case]["archive_sha256"]
    rc2, arc2, st2 = csa.DeviceArchive.write(table, _upload(src), arcname=csa_cases.ARCNAME, **opts)
    assert rc2 == 0 and _bytes(arc2) == _bytes(arc)
    assert {k: st[k] for k in SAME} == {k: st2[k] for k in SAME}, "the same plan, the same launches, the same bytes over the bus"


# ---- 2. edge sizes and plans ------------------------------------------------------------------------------------------------

def _edge_content():
    return {f"e/f{n:05d}.bin": (cases.build([["text", 50 + i, 0, n]]) if n else b"") for i, n in enumerate(EDGE_SIZES)}


PLANS = {
    "one_task": (_edge_content, dict(level=1, dict_size=64 << 10)),                  # many small files in one task: any posblock alignment
    "single": (lambda: {"one/only.dat": cases.build([["exe", 61, 0, 200003]])}, dict(level=2, dict_size=64 << 10, split_count=3)),
    "fragmented": (_edge_content, dict(level=1, dict_size=64 << 10, task_bytes=20000)),
    "waves": (_edge_content, dict(level=1, dict_size=64 << 10, task_bytes=20000, device_streams=2)),
}


@pytest.fixture(scope="module")
def plans(csa):
    """name -> dict(content, table, entries, arc (device), data (its bytes), st (write_tensors' stats), st_c, data_c (the contiguous
    write's), opts, ropts), each built when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            make, opts = PLANS[name]
            content = make()
            table, src = [], bytearray()
            for i, (rel, data) in enumerate(content.items()):
                off = (len(src) + 15) // 16 * 16 + OFFSETS[(i + 2) % 5]
                src.extend(bytes(off - len(src)) + data)
                table.append({"name": rel, "esize": len(data), "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "offset": off})
            rc_c, arc_c, st_c = csa.DeviceArchive.write(table, _upload(bytes(src)), **opts)
            assert rc_c == 0
            entries = _entries(table, content)
            rc, arc, st = _write_tensors(csa, entries, **opts)
            assert rc == 0
            made[name] = dict(content=content, table=table, entries=entries, arc=arc, data=_bytes(arc), st=st, st_c=st_c, data_c=_bytes(arc_c),
                              opts=opts, ropts={k: v for k, v in opts.items() if k == "device_streams"})
        return made[name]
    return get


@pytest.mark.parametrize("name", list(PLANS))
def test_write_matches_the_contiguous_write(csa, plans, name):
    p = plans(name)
    assert p["data"] == p["data_c"]
    assert {k: p["st"][k] for k in SAME} == {k: p["st_c"][k] for k in SAME}
    st = p["st"]
    if name == "one_task":
        assert st["tasks"] == 1
        assert len({e["tensor"].data_ptr() % 16 for e in p["entries"] if e["tensor"] is not None}) >= 4
    if name == "single":
        assert st["tasks"] == 1 and [f["nfrags"] for f in st["files"]] == [1]                 # encoded where it lies
    if name in ("fragmented", "waves"):
        assert st["tasks"] >= 5 and max(f["nfrags"] for f in st["files"]) >= 2                # files cut across tasks
    if name == "waves":
        assert st["waves"] == (st["tasks"] + 1) // 2 > 1


def test_write_accepts_aliasing_refuses_the_archive_and_a_short_one(csa):
    import torch
    data = cases.build([["text", 7, 0, 5000]])
    t = _upload(data, 3)
    row = {"edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    twice = [dict(row, name="a.bin", tensor=t), dict(row, name="b.bin", tensor=t[100:4100])]
    rc, arc, st = _write_tensors(csa, twice, level=1)
    assert rc == 0
    rc2, arc2, _ = csa.DeviceArchive.write([dict(row, name="a.bin", esize=5000, offset=0), dict(row, name="b.bin", esize=4000, offset=100)], t, level=1)
    assert rc2 == 0 and _bytes(arc2) == _bytes(arc)
    n = arc.numel()
    # an entry that overlaps arc by its last byte
    big = torch.full((8192 + n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    inside = [dict(row, name="a.bin", tensor=big[8192 - 4999:8192 + 1])]
    rc, out, st = csa.DeviceArchive.write_tensors(inside, arc=big[8192:], level=1)
    assert rc == -1 and out is None and st["launches"] == 0 and st["encode_launches"] == 0 and st["upload_bytes"] == 0
    assert bool((big == 0xA5).all()), "arc unchanged"
    rc, out, st = csa.DeviceArchive.write_tensors([dict(row, name="a.bin", tensor=big[8192 - 5000:8192])], arc=big[8192:], level=1)
    assert rc == 0, "touching is fine"
    # arc_cap one byte short
    big.fill_(0xA5)
    rc, out, st = csa.DeviceArchive.write_tensors(twice, arc=big[:n - 1], level=1)
    assert rc == csa.WRITE_ERROR and out is None
    assert bool((big[n - 1:] == 0xA5).all()), "the bytes behind arc_cap"


# ---- 3. read into -------------------------------------------------------------------------------------------------------------

READ_SAME = ["tasks", "frags", "waves", "launches", "decode_launches", "readback_bytes", "raw_bytes", "verify_failures"]
STOP_SAME = ["decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks"]


def _no_offset(files):
    return [{k: v for k, v in f.items() if k != "offset"} for f in files]


def _dsts(files):
    return {f["name"]: Guarded(f["size"], OFFSETS[i % 5]) for i, f in enumerate(files)}


@pytest.mark.parametrize("name", list(PLANS))
def test_read_into_equals_extract(csa, plans, name):
    p = plans(name)
    with csa.DeviceArchive.open(p["arc"]) as a:
        files = a.plan()[0]
        for stop in (False, True):
            rc0, views, st0 = a.extract(stop_early=stop, **p["ropts"])
            dsts = _dsts(files)
            rc1, st1 = a.extract_into({n: g.view for n, g in dsts.items()}, stop_early=stop, **p["ropts"])
            assert rc1 == rc0 == 0 and st1["verify_failures"] == 0
            assert _no_offset(st1["files"]) == _no_offset(st0["files"]) and all(f["offset"] == 0 for f in st1["files"])
            keys = READ_SAME + (STOP_SAME if stop else [])
            assert {k: st1[k] for k in keys} == {k: st0[k] for k in keys}
            assert st1["launches"] == 3 * st1["waves"]
            for n, g in dsts.items():
                assert _bytes(g.view) == _bytes(views[n]) == p["content"][n], n
                assert g.guards_intact(), n


def test_read_into_a_selection_with_entries_left_out(csa, plans):
    p = plans("fragmented")
    names = ["e/f00001.bin", "e/f00017.bin", "e/f16383.bin", "e/f16385.bin", "e/f32769.bin", "e/f70001.bin"]
    with csa.DeviceArchive.open(p["arc"]) as a:
        files = a.plan(names)[0]
        assert [f["name"] for f in files] == sorted(names)
        dsts = _dsts(files)
        given = {f["name"]: (dsts[f["name"]].view if i % 2 else None) for i, f in enumerate(files)}
        for stop in (False, True):
            rc_t, st_t = a.test(names, stop_early=stop)
            rc, st = a.extract_into(given, names, stop_early=stop)
            assert rc == rc_t == 0 and st["verify_failures"] == 0
            keys = READ_SAME + (STOP_SAME if stop else [])
            assert {k: st[k] for k in keys} == {k: st_t[k] for k in keys}, "an entry without a buffer is still verified, and counts for the stops"
            assert _no_offset(st["files"]) == _no_offset(st_t["files"])
            for n, g in dsts.items():
                if given[n] is None:
                    assert g.untouched(), n
                else:
                    assert _bytes(g.view) == p["content"][n] and g.guards_intact(), n


def _flipped_in_the_body(p):
    """the archive with one byte changed in the middle of its task streams, which lie between the header and the index"""
    bad = bytearray(p["data"])
    index_pos = int.from_bytes(bad[8:16], "little")
    bad[24 + (index_pos - 24) // 2] ^= 0x40
    return _upload(bytes(bad))


def test_read_into_and_compare_report_damage_as_test_does(csa, plans):
    p = plans("one_task")
    with csa.DeviceArchive.open(_flipped_in_the_body(p)) as a:
        files = a.plan()[0]
        rc_t, st_t = a.test()
        assert rc_t == -1 or st_t["verify_failures"] > 0
        dsts = _dsts(files)
        rc, st = a.extract_into({n: g.view for n, g in dsts.items()})
        assert (rc, st["verify_failures"]) == (rc_t, st_t["verify_failures"])
        assert [f["failed_frags"] for f in st["files"]] == [f["failed_frags"] for f in st_t["files"]]
        assert all(g.guards_intact() for g in dsts.values())
        rc, diffs, st = a.compare({e["name"]: e["tensor"] for e in p["entries"]})
        assert (rc, st["verify_failures"]) == (rc_t, st_t["verify_failures"])
        assert [diffs[f["name"]]["failed_frags"] for f in st_t["files"]] == [f["failed_frags"] for f in st_t["files"]]


# ---- 4. read into, refusals -----------------------------------------------------------------------------------------------------

def test_read_into_refusals_launch_nothing(csa, plans):
    import torch
    p = plans("one_task")
    n_arc = len(p["data"])
    big = torch.full((n_arc + 80000,), 0xA5, dtype=torch.uint8, device="cuda")
    big[:n_arc].copy_(p["arc"])
    with csa.DeviceArchive.open(big[:n_arc]) as a:
        files = a.plan()[0]
        sizes = {f["name"]: f["size"] for f in files}
        last, other = "e/f70001.bin", "e/f32769.bin"

        def refused(dsts, want, guarded):
            rc, st = a.extract_into(dsts)
            assert rc == want
            assert st["launches"] == 0 and st["decode_launches"] == 0 and st["tasks"] == 0 and st["readback_bytes"] == 0
            assert all(g.untouched() for g in guarded)
        # a capacity one byte short
        g = Guarded(sizes[last] - 1, 3)
        refused({last: g.view}, csa.WRITE_ERROR, [g])
        # two destinations that overlap by one byte
        g = Guarded(sizes[last] + sizes[other] - 1, 1)
        refused({last: g.view[:sizes[last]], other: g.view[sizes[last] - 1:]}, -1, [g])
        rc, st = a.extract_into({last: g.buf[:sizes[last]], other: g.buf[sizes[last]:sizes[last] + sizes[other]]})
        assert rc == 0, "touching is fine"
        # a destination that overlaps the archive by one byte
        refused({last: big[n_arc - 1:n_arc - 1 + sizes[last]]}, -1, [])
        assert _bytes(big[:n_arc]) == p["data"] and bool((big[n_arc:] == 0xA5).all())
        # the wrong n
        ptrs, caps = (C.c_void_p * len(files))(), (C.c_uint64 * len(files))()
        st = csa.CSADevReadStats()
        for n in (len(files) - 1, len(files) + 1):
            assert csa.lib().CSAMI_DeviceReadInto(a._h, None, 0, ptrs, caps, n, 0, None, None, C.byref(st), None) == -1
            assert st.launches == 0 and st.decode_launches == 0
        assert csa.lib().CSAMI_DeviceReadInto(a._h, None, 0, ptrs, caps, len(files), 0, None, None, C.byref(st), None) == 0
        # a key that is no selected entry
        g = Guarded(16)
        with pytest.raises(KeyError):
            a.extract_into({"e/nothing.bin": g.view})
        with pytest.raises(KeyError):
            a.extract_into({other: g.view}, names=[last])
        with pytest.raises(KeyError):
            a.compare({"e/nothing.bin": g.view})
        assert g.untouched()


# ---- 5. compare ---------------------------------------------------------------------------------------------------------------

def _originals(p):
    import torch
    return {e["name"]: e["tensor"] if e["tensor"] is not None else torch.empty(0, dtype=torch.uint8, device="cuda") for e in p["entries"]}


def _compare_bounds(st, index_raw_size):
    assert st["launches"] == 3 * st["waves"]
    assert st["readback_bytes"] <= 16 * st["tasks"] + 16 * st["frags"] + 24 + 10 + index_raw_size


@pytest.mark.parametrize("name", list(PLANS))
def test_compare_against_the_originals(csa, plans, name):
    p = plans(name)
    srcs = _originals(p)
    before = {n: _bytes(t) for n, t in srcs.items()}
    with csa.DeviceArchive.open(p["arc"]) as a:
        for stop in (False, True):
            rc_t, st_t = a.test(stop_early=stop, **p["ropts"])
            rc, diffs, st = a.compare(srcs, stop_early=stop, **p["ropts"])
            assert rc == rc_t == 0 and st["verify_failures"] == st_t["verify_failures"] == 0
            assert diffs == {n: {"status": 0, "first_diff": csa.NO_DIFF, "failed_frags": 0} for n in srcs}
            assert {k: st[k] for k in READ_SAME if k != "readback_bytes"} == {k: st_t[k] for k in READ_SAME if k != "readback_bytes"}
            _compare_bounds(st, p["st"]["index_raw_size"])
            ms = a.kernel_ms()
            assert ms[1] > 0 and ms[2] > 0
    assert {n: _bytes(t) for n, t in srcs.items()} == before


def test_compare_names_the_first_differing_byte(csa, plans, tmp_path):
    p = plans("fragmented")
    (tmp_path / "f.csa").write_bytes(p["data"])
    listed = {e["name"]: e for e in csa.list_entries(str(tmp_path / "f.csa"))}
    seams = {n: sorted(f["posfile"] for f in e["frags"])[1:] for n, e in listed.items()}   # a fragment of an entry ends one task, the next begins another
    assert sum(len(s) for s in seams.values()) >= 4
    assert seams["e/f32769.bin"] and seams["e/f70001.bin"]

    def position(name, n, s):
        return {"e/f00001.bin": 0, "e/f00015.bin": n - 1, "e/f00017.bin": 0, "e/f04095.bin": n - 1, "e/f16384.bin": 16383, "e/f16385.bin": 16384,
                "e/f32769.bin": s[0] if s else None, "e/f70001.bin": s[-1] - 1 if s else None}.get(name)     # the others: left as they are
    want, srcs = {}, {}
    for k, (name, data) in enumerate(p["content"].items()):
        if not data:
            continue                                                                   # the empty file: no buffer given
        at = position(name, len(data), seams[name])
        changed = bytearray(data)
        if at is not None:
            changed[at] ^= 0x20
            want[name] = at
        if name == "e/f32769.bin":                                                     # flipped twice: the smaller offset is reported
            changed[len(data) - 1] ^= 0x01
            assert at < len(data) - 1
        srcs[name] = _upload(bytes(changed), OFFSETS[(k + 1) % 5])
    assert len(want) == 8 and len(srcs) == 10
    print("flipped at", want)
    before = {n: _bytes(t) for n, t in srcs.items()}
    with csa.DeviceArchive.open(p["arc"]) as a:
        rc_t, st_t = a.test()
        rc, diffs, st = a.compare(srcs)
        assert rc == rc_t == 0 and st["verify_failures"] == 0
        _compare_bounds(st, p["st"]["index_raw_size"])
    for name in p["content"]:
        d = diffs[name]
        if name in want:
            assert (d["status"], d["first_diff"]) == (csa.CSA_DIFF_BYTES, want[name]), name
        elif name in srcs:
            assert (d["status"], d["first_diff"]) == (0, csa.NO_DIFF), name
        else:
            assert (d["status"], d["first_diff"]) == (csa.CSA_DIFF_SKIPPED, csa.NO_DIFF), name     # (the empty file: no buffer given)
    assert {n: _bytes(t) for n, t in srcs.items()} == before


def test_compare_every_edge_position_in_one_entry(csa, plans):
    """the positions the list of the issue names, each on a copy of the entry that has it: 0, size - 1, 16383, 16384 (the seam of
    two pieces) -- in plan "one_task", where the entry lies at an odd offset of its task"""
    p = plans("one_task")
    with csa.DeviceArchive.open(p["arc"]) as a:
        for name, ats in (("e/f70001.bin", [0, 70000, 16383, 16384, 16385, 65535]), ("e/f16385.bin", [16383, 16384]), ("e/f00001.bin", [0])):
            for k, at in enumerate(ats):
                changed = bytearray(p["content"][name])
                changed[at] ^= 0x80
                rc, diffs, st = a.compare({name: _upload(bytes(changed), OFFSETS[k % 5])}, [name])
                assert rc == 0 and diffs == {name: {"status": csa.CSA_DIFF_BYTES, "first_diff": at, "failed_frags": 0}}, (name, at)


def test_compare_sizes_and_entries_left_out(csa, plans):
    p = plans("fragmented")
    c = p["content"]
    short, long_, skipped, both = "e/f70001.bin", "e/f16384.bin", "e/f04095.bin", "e/f32769.bin"
    srcs = _originals(p)
    srcs[short] = _upload(c[short][:-1], 1)
    srcs[long_] = _upload(c[long_] + b"\x00", 3)
    srcs[skipped] = None
    changed = bytearray(c[both][:-1])
    changed[20000] ^= 0x04
    srcs[both] = _upload(bytes(changed), 15)
    with csa.DeviceArchive.open(p["arc"]) as a:
        rc, diffs, st = a.compare(srcs)
    assert rc == 0 and st["verify_failures"] == 0
    assert diffs[short] == {"status": csa.CSA_DIFF_SIZE, "first_diff": csa.NO_DIFF, "failed_frags": 0}, "the prefix is equal"
    assert diffs[long_] == {"status": csa.CSA_DIFF_SIZE, "first_diff": csa.NO_DIFF, "failed_frags": 0}
    assert diffs[skipped] == {"status": csa.CSA_DIFF_SKIPPED, "first_diff": csa.NO_DIFF, "failed_frags": 0}
    assert diffs[both] == {"status": csa.CSA_DIFF_SIZE | csa.CSA_DIFF_BYTES, "first_diff": 20000, "failed_frags": 0}
    assert all(d["status"] == 0 for n, d in diffs.items() if n not in (short, long_, skipped, both))


def test_compare_with_an_archive_cut_inside_its_last_task(csa, plans, dec):
    """The task streams end where the index begins.  The archive is cut in the middle of the task that lies last, and the index put
    behind the cut (its position in the header set to it), so that the archive still opens: that task now runs into bytes that are
    not its own and then past the end of the archive, where it is clipped.  A task of these sizes is one run of its decoder, and a
    run that fails delivers nothing: every entry with a fragment in that task is short, every other entry is whole and equal."""
    p = plans("fragmented")
    good = p["data"]
    info = orc_csa.parse(good, dec)
    index_pos = int.from_bytes(good[8:16], "little")
    bid, blocks = max(info["abindex"].items(), key=lambda kv: kv[1][-1][0])
    begin, size = blocks[0][0], sum(n for _, n in blocks)
    assert begin + size == index_pos and len(info["abindex"]) >= 5
    cut = begin + size // 2
    bad = good[:8] + cut.to_bytes(8, "little") + good[16:cut] + good[index_pos:]
    behind = {name for name, e in info["index"].items() for f in e["frags"] if f["bid"] == bid and f["size"]}
    assert behind and len(behind) < len(p["content"]) - 1
    srcs = _originals(p)
    before = {n: _bytes(t) for n, t in srcs.items()}
    with csa.DeviceArchive.open(_upload(bad)) as a:
        rc_t, st_t = a.test()
        rc, diffs, st = a.compare(srcs)
    print("behind the cut", sorted(behind), {n: d["status"] for n, d in diffs.items()})
    assert rc == rc_t == -1 and st["verify_failures"] == st_t["verify_failures"]
    for name, d in diffs.items():
        assert (d["status"], d["first_diff"]) == ((csa.CSA_DIFF_SHORT if name in behind else 0), csa.NO_DIFF), name
    assert {n: _bytes(t) for n, t in srcs.items()} == before


# ---- 6. round trip ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trip_entries(csa):
    content = {"t/big.txt": cases.build([["text", 91, 0, 3 * MiB]]), "t/a.exe": cases.build([["exe", 92, 0, 70001]]),
               "t/b.txt": cases.build([["text", 93, 0, 16385]]), "t/empty.txt": b""}
    row = {"edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    entries = [dict(row, name=n, tensor=_upload(d, OFFSETS[i % 5]) if d else None) for i, (n, d) in enumerate(content.items())]
    entries.append({"name": "t/", "tensor": None, "edate": _edate(csa), "eattr": csa_write_cases.DIR_ATTR})
    return content, entries


@pytest.mark.parametrize("level", [1, 3, 5])
def test_round_trip(csa, trip_entries, level):
    import torch
    content, entries = trip_entries
    rc, arc, st = _write_tensors(csa, entries, level=level, dict_size=1 << 20)
    assert rc == 0
    with csa.DeviceArchive.open(arc) as a:
        files = a.plan()[0]
        assert [f["name"] for f in files] == sorted(e["name"] for e in entries)
        dsts = _dsts(files)
        rc, rst = a.extract_into({n: g.view for n, g in dsts.items()})
        assert rc == 0 and rst["verify_failures"] == 0 and rst["launches"] == 3 * rst["waves"]
        for n, d in content.items():
            assert _bytes(dsts[n].view) == d and dsts[n].guards_intact(), n
        empty = torch.empty(0, dtype=torch.uint8, device="cuda")
        rc, diffs, cst = a.compare({e["name"]: e["tensor"] if e["tensor"] is not None else empty for e in entries})
        assert rc == 0 and cst["verify_failures"] == 0
        assert diffs == {e["name"]: {"status": 0, "first_diff": csa.NO_DIFF, "failed_frags": 0} for e in entries}
        _compare_bounds(cst, st["index_raw_size"])
