"""GPU tier for the device archive update (include/csa_mi355x.h: CSAMI_DeviceUpdate; csc_amd.csa.DeviceArchive.update): the streams
of the tasks whose composition and bytes an archive in HBM already holds are copied out of it, the others are encoded.  Bases are
written by write_tensors / write_slices with the case's options, "fresh" is that same call over the new entries, and every
successful update must give fresh byte for byte, extract to the new contents, and leave the caller's buffers and the base buffer
as they were.

The task groups of mixed_tree by the planner's rules, largest first: {a.txt, b.txt} 370000, {c.exe} 200000, {empty, noext, e.dat}
155000 (the first test pins them with device_write_plan)."""
import ctypes as C
import json
import os
import sys

import pytest

import cases
import csa_cases
import csa_write_cases
from test_gpu_archive_device import _rechop, _reindex, codec  # noqa: F401  (the base cut into extents of 1, 2, 9, 10, 11 and 4097 bytes)
from test_gpu_archive_write_slices import Scattered

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

NO_BID = (1 << 64) - 1
REUSED, NEW, PROPS, CHANGED, BASE_BAD = range(5)
TXT, EXE, DAT = 0, 1, 2                         # mixed_tree's task ids


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


def _edate(csa):
    return int(csa.lib().CSA_DecimalTime(csa_cases.MTIME))


def _bytes(view):
    return view.cpu().numpy().tobytes()


def _upload(data, off=0):
    import torch
    buf = torch.empty(off + len(data), dtype=torch.uint8, device="cuda")
    t = buf[off:]
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _opts(case):
    return {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}


def _entries(csa, case, changed=None):
    """-> (entries for write_tensors / update, {name: content}); changed: {name: new content}, None drops the entry"""
    table, _, content = csa_write_cases.table(case, _edate(csa))
    content.update({k: v for k, v in (changed or {}).items() if v is not None})
    out = []
    for f in table:
        if changed and f["name"] in changed and changed[f["name"]] is None:
            content.pop(f["name"])
            continue
        data = content.get(f["name"])
        out.append({"name": f["name"], "edate": f["edate"], "eattr": f["eattr"], "tensor": _upload(data) if data else None})
    return out, content


def _base(csa, case, **opts):
    entries, content = _entries(csa, case)
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **(opts or _opts(case)))
    assert rc == 0
    return arc, content


def _fresh(csa, entries, **opts):
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0
    return _bytes(arc), st


def _update(csa, base, entries, content, trust=False, arc=None, want=None, **opts):
    """update over the base tensor; on success: arc == `want` (fresh), it extracts to `content` (None: not checked here), and nothing
    of the caller's or the base's was written -> (rc, archive bytes, stats)"""
    mine = [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries]
    theirs = _bytes(base)
    with csa.DeviceArchive.open(base) as a:
        rc, out, st = a.update(entries, arcname=csa_cases.ARCNAME, arc=arc, trust_sums=trust, **opts)
    assert [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries] == mine, "nothing of the caller's is written"
    assert _bytes(base) == theirs, "nothing of the base is written"
    if rc != 0:
        return rc, None, st
    got = _bytes(out)
    assert st["archive_bytes"] == len(got) and st["launches"] <= 5 * st["waves"] + 2 and st["check_launches"] == 3 * st["check_waves"]
    assert st["reused_tasks"] + st["encoded_tasks"] == len(st["tasks"])
    assert st["reused_tasks"] == sum(t["status"] == REUSED for t in st["tasks"])
    assert all((t["base_bid"] == NO_BID) == (t["status"] == NEW) for t in st["tasks"])
    if trust:
        assert st["decoded_bytes"] == st["decode_launches"] == 0
    if want is not None:
        assert got == want, "byte for byte the fresh write's archive"
    if content is not None:
        with csa.DeviceArchive.open(out) as a:
            rc_x, views, xst = a.extract()
        assert rc_x == 0 and xst["verify_failures"] == 0
        assert {n: _bytes(v) for n, v in views.items() if not n.endswith("/")} == content
    return rc, got, st


def _status(st):
    return [t["status"] for t in st["tasks"]]


@pytest.fixture(scope="module")
def mixed(csa):
    """mixed_tree written once: (the archive tensor, its bytes, {name: content})"""
    arc, content = _base(csa, "mixed_tree")
    return arc, _bytes(arc), content


# ---- 1. nothing changed ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_nothing_changed_copies_every_stream(csa, mixed, trust):
    base, data, content = mixed
    entries, _ = _entries(csa, "mixed_tree")
    files = [{"name": e["name"], "esize": 0 if e["tensor"] is None else e["tensor"].numel(), "edate": e["edate"], "eattr": e["eattr"]} for e in entries]
    assert csa.device_write_plan(files, **_opts("mixed_tree"))[::3] == (0, 725000), "three tasks (their totals: below)"
    assert csa.device_write_plan(files, **_opts("mixed_tree"))[1] == 3
    fresh, fst = _fresh(csa, entries, **_opts("mixed_tree"))
    rc, got, st = _update(csa, base, entries, content, trust, want=fresh, **_opts("mixed_tree"))
    assert rc == 0 and got == data
    assert st["tasks"] == [{"base_bid": b, "status": REUSED} for b in (TXT, EXE, DAT)]
    assert (st["candidates"], st["reused_tasks"], st["encoded_tasks"], st["encoded_raw_bytes"]) == (3, 3, 0, 0)
    assert st["reused_raw_bytes"] == 370000 + 200000 + 155000 == st["checked_bytes"] == st["raw_bytes"]
    assert st["reused_stream_bytes"] == len(data) - 24 - st["index_compressed_size"]
    assert st["gathered_tasks"] == st["inplace_tasks"] == st["retries"] == 0, "the gather statistics count encoded tasks only"
    assert st["check_waves"] == 1 and st["blocks"] == fst["blocks"] and st["frags"] == fst["frags"]
    if not trust:
        assert st["decoded_bytes"] == 725000 and st["decode_launches"] > 0


# ---- 2. one byte ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_one_changed_byte_encodes_its_task_alone(csa, mixed, trust):
    base, data, content = mixed
    b = bytearray(content["d/b.txt"]); b[35000] ^= 1
    entries, new = _entries(csa, "mixed_tree", {"d/b.txt": bytes(b)})
    fresh, _ = _fresh(csa, entries, **_opts("mixed_tree"))
    rc, got, st = _update(csa, base, entries, new, trust, want=fresh, **_opts("mixed_tree"))
    assert rc == 0 and got != data
    assert st["tasks"] == [{"base_bid": TXT, "status": CHANGED}, {"base_bid": EXE, "status": REUSED}, {"base_bid": DAT, "status": REUSED}]
    assert (st["encoded_tasks"], st["encoded_raw_bytes"], st["gathered_tasks"]) == (1, 370000, 1)


# ---- 3. the adler32 collision ---------------------------------------------------------------------------------------------------

def test_equal_sums_are_told_apart_only_by_the_bytes(csa, mixed):
    base, data, content = mixed
    old = content["d/a.txt"]
    i = next(k for k in range(1000, len(old) - 2) if old[k] < 255 and old[k + 1] >= 2 and old[k + 2] < 255)
    b = bytearray(old); b[i] += 1; b[i + 1] -= 2; b[i + 2] += 1           # A keeps its sum, and so does B: +1 * (n - i) - 2 * (n - i - 1) + (n - i - 2) = 0
    assert bytes(b) != old and csa.adler32(bytes(b)) == csa.adler32(old)
    entries, new = _entries(csa, "mixed_tree", {"d/a.txt": bytes(b)})
    fresh, _ = _fresh(csa, entries, **_opts("mixed_tree"))
    rc, got, st = _update(csa, base, entries, new, want=fresh, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [CHANGED, REUSED, REUSED]
    # the documented limit of trust_sums: the contents are taken for equal, and the archive holds the OLD bytes
    rc, got, st = _update(csa, base, entries, content, trust=True, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [REUSED] * 3 and got == data != fresh


# ---- 4. another order of the tasks --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_a_shorter_entry_reorders_the_tasks(csa, mixed, trust):
    base, data, content = mixed
    entries, new = _entries(csa, "mixed_tree", {"d/a.txt": content["d/a.txt"][:100000]})
    fresh, _ = _fresh(csa, entries, **_opts("mixed_tree"))
    rc, got, st = _update(csa, base, entries, new, trust, want=fresh, **_opts("mixed_tree"))
    assert rc == 0     # exe 200000, txt 170000, dat 155000 against the base's txt, exe, dat
    assert [(t["base_bid"], t["status"]) for t in st["tasks"]] == [(EXE, REUSED), (NO_BID, NEW), (DAT, REUSED)]


# ---- 5. composition -------------------------------------------------------------------------------------------------------------

def test_composition_changes(csa, mixed):
    base, data, content = mixed
    opts = _opts("mixed_tree")
    for what, changed in [("an entry added", {"d/new.dat": None}), ("an entry removed", {"d/noext": None})]:
        entries, new = _entries(csa, "mixed_tree", changed if what == "an entry removed" else None)
        if what == "an entry added":
            new["d/new.dat"] = cases.build([["delta", 9, 0, 3000]])
            entries.append({"name": "d/new.dat", "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": _upload(new["d/new.dat"])})
        fresh, _ = _fresh(csa, entries, **opts)
        rc, got, st = _update(csa, base, entries, new, want=fresh, **opts)
        assert rc == 0 and [(t["base_bid"], t["status"]) for t in st["tasks"]] == [(TXT, REUSED), (EXE, REUSED), (NO_BID, NEW)], what
    entries, new = _entries(csa, "mixed_tree")
    entries = [dict(e, edate=e["edate"] + 1, eattr=e["eattr"] ^ 0x100) for e in entries]
    fresh, _ = _fresh(csa, entries, **opts)
    rc, got, st = _update(csa, base, entries, new, want=fresh, **opts)
    assert rc == 0 and _status(st) == [REUSED] * 3 and got != data and len(got) - st["index_compressed_size"] == len(data) - _index_csize(data)


def _index_csize(arc):
    return int.from_bytes(arc[16:20], "little")


# ---- 6. other properties ------------------------------------------------------------------------------------------------------

def test_another_dictionary_size_reuses_only_equal_property_bytes(csa, mixed, orc):
    base, data, content = mixed
    opts = dict(_opts("mixed_tree"), dict_size=180000)
    want = [REUSED if orc.write_properties(orc.props_init(min(180000, total), 2)) == orc.write_properties(orc.props_init(min(1 << 20, total), 2))
            else PROPS for total in (370000, 200000, 155000)]
    assert want[DAT] == REUSED and PROPS in want
    entries, new = _entries(csa, "mixed_tree")
    fresh, _ = _fresh(csa, entries, **opts)
    for trust in (False, True):
        rc, got, st = _update(csa, base, entries, new, trust, want=fresh, **opts)
        assert rc == 0 and _status(st) == want and st["candidates"] == 3 and got != data
        assert st["checked_bytes"] == sum(t for t, w in zip((370000, 200000, 155000), want) if w == REUSED), "a task that is out is not checked"


# ---- 7. a base cut into other blocks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_interleaved_base_extents_give_the_canonical_table(csa, mixed, codec, trust):  # noqa: F811
    import torch
    _, data, content = mixed
    chopped, ab = _rechop(data, orc_csa.parse(data, codec[1]), codec)
    assert chopped != data and any(v[0][1] < 10 for v in ab.values()), "one task's first extent is shorter than the property bytes"
    base = _upload(chopped, 3)
    entries, new = _entries(csa, "mixed_tree")
    room = torch.full((5 + len(data) + 7,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, got, st = _update(csa, base, entries, new, trust, arc=room[5:5 + len(data)], want=data, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [REUSED] * 3 and got != chopped
    assert _bytes(room[:5]) == b"\xa5" * 5 and _bytes(room[5 + len(data):]) == b"\xa5" * 7


# ---- 8. a damaged base stream -------------------------------------------------------------------------------------------------

def test_a_flipped_byte_in_the_base_is_not_reused(csa, mixed, codec):  # noqa: F811
    _, data, content = mixed
    info = orc_csa.parse(data, codec[1])
    bid = max(info["abindex"], key=lambda b: sum(n for _, n in info["abindex"][b]))
    o, n = info["abindex"][bid][0]
    bad = bytearray(data); bad[o + n // 2] ^= 0x40
    entries, new = _entries(csa, "mixed_tree")
    rc, got, st = _update(csa, _upload(bytes(bad)), entries, new, want=data, **_opts("mixed_tree"))
    assert rc == 0 and [t["base_bid"] for t in st["tasks"]] == [TXT, EXE, DAT]         # (the largest STREAM is the one that compresses worst)
    assert st["tasks"][bid]["status"] in (BASE_BAD, CHANGED) and [s for i, s in enumerate(_status(st)) if i != bid] == [REUSED, REUSED]


def test_a_wrong_checksum_in_the_base_index_does_not_survive(csa, mixed, codec):  # noqa: F811
    _, data, content = mixed
    info = orc_csa.parse(data, codec[1])
    index = {n: dict(e, frags=[dict(f) for f in e["frags"]]) for n, e in info["index"].items()}
    index["d/b.txt"]["frags"][0]["checksum"] ^= 1
    base = _upload(_reindex(data, info, codec, index=index))
    entries, new = _entries(csa, "mixed_tree")
    # verify compares bytes: the task is reused and its fragments get the sums of this pass; trust_sums sees a sum that differs
    rc, got, st = _update(csa, base, entries, new, want=data, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [REUSED] * 3
    rc, got, st = _update(csa, base, entries, new, trust=True, want=data, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [CHANGED, REUSED, REUSED]


def test_a_reused_stream_that_does_not_end_at_its_length_is_refused(csa, mixed, codec):  # noqa: F811
    """trust_sums trusts the base's stream; what the block-table walk over the placed stream can still see is its framing"""
    _, data, content = mixed
    info = orc_csa.parse(data, codec[1])
    o, n = info["abindex"][EXE][0]
    bad = bytearray(data); bad[o + 10] ^= 0x40                    # the first coder block's flag byte: "the payload is exactly one block"
    entries, new = _entries(csa, "mixed_tree")
    rc, got, st = _update(csa, _upload(bytes(bad)), entries, None, trust=True, **_opts("mixed_tree"))
    assert rc == -1 and _status(st) == [REUSED] * 3
    rc, got, st = _update(csa, _upload(bytes(bad)), entries, new, want=data, **_opts("mixed_tree"))
    assert rc == 0 and _status(st) == [REUSED, BASE_BAD, REUSED]


# ---- 9. tasks encoded where they lie ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def split3(csa):
    """single_split3 written once, and the fresh write of it with one byte of the middle third changed"""
    base, content = _base(csa, "single_split3")
    b = bytearray(content["big.bin"]); b[len(b) // 2] ^= 0x55
    entries, new = _entries(csa, "single_split3", {"big.bin": bytes(b)})
    fresh, fst = _fresh(csa, entries, **_opts("single_split3"))
    return base, entries, new, fresh, fst


@pytest.mark.parametrize("trust", [False, True])
def test_single_file_split_in_three(csa, split3, trust):
    base, entries, new, fresh, fst = split3
    rc, got, st = _update(csa, base, entries, new, trust, want=fresh, **_opts("single_split3"))
    assert rc == 0 and fst["tasks"] == 3 and _status(st) == [REUSED, CHANGED, REUSED]
    assert (st["inplace_tasks"], st["gathered_tasks"]) == (1, 0)
    # with trust_sums the check's sums of the changed task are kept: it is not summed a second time
    assert st["plain_pieces"] == (0 if trust else -(-st["encoded_raw_bytes"] // 16384))


# ---- 10. slices -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_strided_slices(csa, trust):
    opts = dict(level=1, dict_size=64 << 10)
    rows = [("s/a.b0", cases.build([["text", 70, 0, 1000 * 90]]), 1000, 1003, 90), ("s/b.b1", cases.build([["exe", 71, 0, 15 * 5000]]), 15, 16, 5000),
            ("s/c.b2", cases.build([["text", 72, 0, 1000 * 70]]), 1000, 1003, 70), ("s/d.b0", cases.build([["text", 73, 0, 15 * 300]]), 15, 16, 300)]
    sc = Scattered(csa, rows)
    rc, base, bst = csa.DeviceArchive.write_slices(sc.entries, arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0 and bst["tasks"] == 3
    c = bytearray(rows[1][1]); c[40000] ^= 0x11
    rows[1] = (rows[1][0], bytes(c)) + rows[1][2:]
    new = Scattered(csa, rows)
    rc, fresh, fst = csa.DeviceArchive.write_slices(new.entries, arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0
    rc, got, st = _update(csa, base, new.entries, new.content, trust, want=_bytes(fresh), **opts)
    assert rc == 0 and new.unchanged(), "the gaps are still 0xA5"
    assert sorted(_status(st)) == [REUSED, REUSED, CHANGED] and st["encoded_raw_bytes"] == 75000
    assert st["checked_bytes"] == st["raw_bytes"] == 90000 + 75000 + 70000 + 4500
    # every entry is longer than its run, and no 16 KiB piece of a packed fragment lies inside a run of 1000 or 15 bytes: whatever
    # the check summed (trust) or compared (verify) it took across run borders, through the rows form of its kernel
    assert all(e["slice"][1] < 4500 <= e["slice"][1] * e["slice"][3] for e in new.entries)
    assert st["periodic_pieces"] == -(-75000 // 16384), "the gather statistics: the one encoded task's pieces"


# ---- 11. several waves ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trust", [False, True])
def test_many_files_in_several_waves(csa, trust):
    opts = dict(_opts("many_files"), device_streams=4)
    base, content = _base(csa, "many_files", **opts)
    changed = {}
    for name in ("m/f00.a0", "m/f05.f2", "m/same3.log"):
        b = bytearray(content[name]); b[len(b) // 3] ^= 0x21
        changed[name] = bytes(b)
    entries, new = _entries(csa, "many_files", changed)
    fresh, fst = _fresh(csa, entries, **opts)
    rc, got, st = _update(csa, base, entries, new, trust, want=fresh, **opts)
    assert rc == 0 and len(st["tasks"]) == fst["tasks"] > 8
    assert _status(st).count(CHANGED) == 3 == st["encoded_tasks"] and _status(st).count(REUSED) == fst["tasks"] - 3
    assert st["check_waves"] == -(-fst["tasks"] // 4) > 1 and st["waves"] == fst["waves"] > 1
    assert st["launches"] <= 5 * st["waves"] + 2 and st["check_launches"] == 3 * st["check_waves"]


# ---- 12. a base the reference wrote ---------------------------------------------------------------------------------------------

def test_the_reference_archivers_golden_as_the_base(csa):
    import hashlib
    with open(os.path.join(ROOT, "tests", "golden", "csa.json")) as f:
        golden = json.load(f)["named_files_m3"]
    entries, content = _entries(csa, "named_files_m3")
    fresh, _ = _fresh(csa, entries, **_opts("named_files_m3"))
    assert hashlib.sha256(fresh).hexdigest() == golden["archive_sha256"], "the base IS the reference's archive"
    for trust in (False, True):
        rc, got, st = _update(csa, _upload(fresh, 1), entries, content, trust, want=fresh, **_opts("named_files_m3"))
        assert rc == 0 and set(_status(st)) == {REUSED} and st["encoded_tasks"] == 0


# ---- 13. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(csa, mixed):
    import torch
    base, data, content = mixed
    opts = _opts("mixed_tree")
    entries, new = _entries(csa, "mixed_tree")
    # arc inside, and one byte into, the base buffer
    both = torch.empty(2 * len(data) + 64, dtype=torch.uint8, device="cuda")
    both[:len(data)].copy_(base)
    for lo in (0, len(data) - 1):
        rc, got, st = _update(csa, both[:len(data)], entries, None, arc=both[lo:], **opts)
        assert rc == -1 and (st["launches"], st["encode_launches"], st["check_launches"], st["candidates"], st["upload_bytes"]) == (0, 0, 0, 0, 0)
    rc, got, st = _update(csa, both[:len(data)], entries, new, arc=both[len(data):], want=data, **opts)
    assert rc == 0, "ranges that touch do not overlap"
    # one byte short
    room = torch.full((len(data) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, got, st = _update(csa, base, entries, None, arc=room[:len(data) - 1], **opts)
    assert rc == csa.WRITE_ERROR and _bytes(room[len(data) - 1:]) == b"\xa5" * 9
    # base == NULL is CSAMI_DeviceWriteSlices; task_cap bounds what is filled
    L = csa.lib()
    n = len(entries)
    ptrs = (C.c_void_p * n)(*[e["tensor"].data_ptr() if e["tensor"] is not None else None for e in entries])
    files = [{"name": e["name"], "esize": 0 if e["tensor"] is None else e["tensor"].numel(), "edate": e["edate"], "eattr": e["eattr"]} for e in entries]
    o = csa.options(**opts)
    torch.cuda.synchronize()
    for handle in (None, "base"):
        arr, keep = csa._write_table(files)
        st, gs, us = csa.CSADevWriteStats(), csa.CSADevGatherStats(), csa.CSADevUpdateStats()
        tasks = (csa.CSADevUpdateTask * 3)()
        C.memset(tasks, 0x5A, C.sizeof(tasks))
        room.fill_(0xA5)
        torch.cuda.synchronize()
        with csa.DeviceArchive.open(base) as a:
            rc = L.CSAMI_DeviceUpdate(a._h if handle else None, ptrs, None, None, arr, n, csa_cases.ARCNAME.encode(), C.c_void_p(room.data_ptr()),
                                      room.numel(), 0, C.byref(o), C.byref(st), C.byref(gs), C.byref(us), tasks, 2 if handle else 3)
        assert rc == 0 and _bytes(room[:st.archive_bytes]) == data and _bytes(room[len(data):]) == b"\xa5" * 8
        if handle:
            assert [(t.base_bid, t.status) for t in tasks[:2]] == [(TXT, REUSED), (EXE, REUSED)] and us.reused_tasks == 3
            assert bytes(tasks)[32:] == b"\x5a" * 16, "no more than task_cap entries are filled"
        else:
            assert bytes(tasks) == b"\x5a" * 48 and bytes(us) == bytes(C.sizeof(us)) and gs.gathered_tasks == 2 and gs.inplace_tasks == 1
