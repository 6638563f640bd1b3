"""GPU tier for the device archive's update in place (include/csa_mi355x.h: CSAMI_DeviceUpdateInPlace;
csc_amd.csa.DeviceArchive.update_in_place): the new archive takes the base's place in the caller's buffer -- the encoded streams are
held in scratch until every size is known, the reused streams move inside the buffer (k_move_extents), the rest is placed.

The yardstick of every successful case is the out-of-place update of the same base and entries (the parent's code), which itself
equals the fresh write: buf[:archive_bytes] is that archive byte for byte, the SAME DeviceArchive object extracts the new contents
without a reopen, the per-task status and every statistic the contract names are the out-of-place call's, nothing behind buf_cap and
nothing of the caller's is written.  Every refusal leaves the buffer byte for byte the base.

The data: mixed_tree (three tasks, 725 kB) and a tree of twelve tasks of 40 to 90 kB entries, at level 2; the twelve-task tree also
at levels 1 and 3."""
import os
import sys

import pytest

import cases
import csa_cases
import csa_write_cases
from test_gpu_archive_device import _rechop, _reindex, codec  # noqa: F401
from test_gpu_archive_update import _bytes, _edate, _entries, _fresh, _opts, _status, _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

REUSED, NEW, PROPS, CHANGED, BASE_BAD = range(5)
CHUNK = 32768
GUARD = 256
MODES = ("verify", "sums", "digests")
# what st shares with the out-of-place call (launches, waves, kernel_ms, upload_bytes, readback_bytes and the times are its own)
SAME = ("tasks", "frags", "blocks", "encode_launches", "raw_bytes", "archive_bytes", "index_raw_size", "index_compressed_size", "n_entries", "retries",
        "selected_bytes", "hull_bytes", "periodic_pieces", "plain_pieces", "gathered_tasks", "inplace_tasks",
        "candidates", "reused_tasks", "encoded_tasks", "reused_raw_bytes", "reused_stream_bytes", "encoded_raw_bytes", "checked_bytes",
        "decoded_bytes", "check_waves", "check_launches", "decode_launches",
        "digest_frags", "digest_leaves", "digested_bytes", "digest_launches", "mismatches", "first_mismatch")


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


def _flags(mode):
    return {"trust_sums": mode == "sums", "trust_digests": mode == "digests"}


def _mk(csa, items):
    """[(name, bytes)] -> (entries, {name: content})"""
    return ([{"name": n, "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": _upload(d) if d else None} for n, d in items],
            dict(items))


def _yardstick(csa, base_bytes, entries, mode, opts, digests=False):
    """the out-of-place update of the base -> (the new archive's bytes, its stats, the base's digest table or None)"""
    base = _upload(base_bytes)
    with csa.DeviceArchive.open(base) as a:
        table = None
        if mode == "digests":
            rc, table, _ = a.digests()
            assert rc == 0
        rc, out, st = a.update(entries, arcname=csa_cases.ARCNAME, base_digests=table, digests=digests, **_flags(mode), **opts)
    assert rc == 0
    return _bytes(out), st, table


class InPlace:
    """the base in a buffer of `cap` bytes with a guard behind it, opened; .run() is update_in_place with the checks every case makes"""

    def __init__(self, csa, base_bytes, cap):
        import torch
        self.csa, self.base, self.cap = csa, base_bytes, cap
        self.room = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.room[:len(base_bytes)].copy_(torch.frombuffer(bytearray(base_bytes), dtype=torch.uint8))
        self.a = csa.DeviceArchive.open(self.room[:len(base_bytes)])

    def close(self):
        self.a.close()

    def run(self, entries, mode, opts, table=None, digests=False):
        mine = [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries]
        rc, view, st = self.a.update_in_place(entries, buf=self.room[:self.cap], arcname=csa_cases.ARCNAME, base_digests=table, digests=digests,
                                              **_flags(mode), **opts)
        assert _bytes(self.room[self.cap:]) == b"\xa5" * GUARD, "nothing behind buf_cap is written"
        assert [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries] == mine, "nothing of the caller's is written"
        if rc == 0:
            assert view.data_ptr() == self.room.data_ptr() and view.numel() == st["archive_bytes"]
            reused = st["reused_tasks"]
            assert st["launches"] <= 5 * st["waves"] + 2 + -(-reused // 2048), "the bound the header states"
            assert st["move_launches"] <= 3 and st["parked_moves"] <= st["moves"] and st["parked_bytes"] <= st["moved_bytes"]
            self.base = _bytes(view)
        else:
            assert view is None
            assert _bytes(self.room[:len(self.base)]) == self.base, "a refusal comes before the first store into the buffer"
        return rc, view, st

    def extracts(self, content):
        """the same object, no reopen"""
        rc, views, xst = self.a.extract()
        assert rc == 0 and xst["verify_failures"] == 0
        assert {n: _bytes(v) for n, v in views.items() if not n.endswith("/")} == content


def _check(csa, base_bytes, entries, content, mode, opts, cap=None, fresh=True):
    """one successful case against its yardstick -> (in-place stats, out-of-place stats, new archive bytes)"""
    want, ost, table = _yardstick(csa, base_bytes, entries, mode, opts)
    if fresh:
        assert want == _fresh(csa, entries, **opts)[0], "the yardstick is the fresh write"
    ip = InPlace(csa, base_bytes, max(len(want), len(base_bytes)) if cap is None else cap)
    try:
        rc, view, st = ip.run(entries, mode, opts, table)
        assert rc == 0
        assert _bytes(view) == want, "byte for byte the out-of-place update's archive"
        assert st["tasks"] == ost["tasks"] and _status(st) == _status(ost)
        assert {k: st[k] for k in SAME if k in ost and k != "tasks"} == {k: ost[k] for k in SAME if k in ost and k != "tasks"}
        assert [(f["name"], f["size"], f["nfrags"]) for f in st["files"]] == [(f["name"], f["size"], f["nfrags"]) for f in ost["files"]]
        ip.extracts(content)
        with csa.DeviceArchive.open(_upload(want)) as b:
            assert ip.a.plan() == b.plan(), "the handle describes the new archive as CSAMI_DeviceOpen would"
    finally:
        ip.close()
    return st, ost, want


@pytest.fixture(scope="module")
def mixed(csa):
    """mixed_tree written once: (its bytes, {name: content})"""
    entries, content = _entries(csa, "mixed_tree")
    data, _ = _fresh(csa, entries, **_opts("mixed_tree"))
    return data, content


OPTS12 = dict(level=2, dict_size=1 << 20)


def _twelve():
    """twelve extensions, twelve tasks: every third one two entries of 40 kB and a bit, the others one entry of 66 to 88 kB; the
    totals differ, so the largest-first order of the tasks is that of the totals"""
    items = []
    for k in range(12):
        if k % 3 == 0:
            items += [(f"t/f{k:02d}a.e{k:02d}", cases.build([["text", 40 + k, 0, 40000 + 300 * k]])),
                      (f"t/f{k:02d}b.e{k:02d}", cases.build([["exe", 60 + k, 0, 40100 + 300 * k]]))]
        else:
            items.append((f"t/f{k:02d}.e{k:02d}", cases.build([[("text", "exe", "delta")[k % 3], 80 + k, 0, 66000 + 2000 * k]])))
    return items


FIRST, LAST = "t/f11.e11", "t/f01.e01"         # the entry of the largest task (88000) and of the smallest (68000)


@pytest.fixture(scope="module")
def twelve(csa):
    """{level: (the archive's bytes, [(name, content)])}, each written once"""
    items = _twelve()
    out = {}

    def get(level):
        if level not in out:
            entries, _ = _mk(csa, items)
            files = [{"name": e["name"], "esize": e["tensor"].numel(), "edate": e["edate"], "eattr": e["eattr"]} for e in entries]
            assert csa.device_write_plan(files, **dict(OPTS12, level=level))[1] == 12
            out[level] = (_fresh(csa, entries, **dict(OPTS12, level=level))[0], items)
        return out[level]
    return get


def _with(items, changed):
    """items with {name: new content | None (dropped)}, and new names appended"""
    out = [(n, changed.get(n, d)) for n, d in items if not (n in changed and changed[n] is None)]
    return out + [(n, d) for n, d in changed.items() if d is not None and n not in dict(items)]


# ---- 1. nothing changed -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_nothing_changed_moves_nothing(csa, mixed, mode):
    data, content = mixed
    entries, _ = _entries(csa, "mixed_tree")
    st, ost, want = _check(csa, data, entries, content, mode, _opts("mixed_tree"))
    assert want == data and _status(st) == [REUSED] * 3
    assert st["moves"] == st["moved_bytes"] == st["move_launches"] == st["held_stream_bytes"] == 0


# ---- 2. a stream in front grows, shrinks; the last one changes ----------------------------------------------------------------

@pytest.mark.parametrize("level", [2, 1, 3])
@pytest.mark.parametrize("what", ["random", "zeros"])
def test_task_0_replaced_moves_everything_behind_it(csa, twelve, what, level):
    data, items = twelve(level)
    opts = dict(OPTS12, level=level)
    # (its first 20000 bytes: the stream grows, or shrinks, by less than a chunk)
    new = (cases.build([["random", 7, 0, 20000]]) if what == "random" else bytes(20000)) + dict(items)[FIRST][20000:]
    entries, content = _mk(csa, _with(items, {FIRST: new}))
    st, ost, want = _check(csa, data, entries, content, "sums", opts, fresh=level == 2)
    assert _status(st) == [CHANGED] + [REUSED] * 11
    shift = int.from_bytes(want[8:16], "little") - int.from_bytes(data[8:16], "little")         # (of the index, and so of every stream behind task 0)
    assert (0 < shift < CHUNK) if what == "random" else (-CHUNK < shift < 0)
    # eleven streams back to back, one shift: one move; each chunk's destination overlaps its own source and its neighbour's
    assert (st["moves"], st["parked_moves"], st["move_launches"]) == (1, 0, 1) and st["moved_bytes"] == st["reused_stream_bytes"] > CHUNK
    assert 0 < st["held_stream_bytes"] < 88000 + 88000 // 8 + 65536


def test_the_last_task_changed_rewrites_only_the_tail(csa, twelve):
    data, items = twelve(2)
    entries, content = _mk(csa, _with(items, {LAST: cases.build([["exe", 99, 0, 68000]])}))
    st, ost, want = _check(csa, data, entries, content, "verify", OPTS12)
    assert _status(st) == [REUSED] * 11 + [CHANGED] and st["moves"] == st["moved_bytes"] == st["move_launches"] == 0
    assert want[24:24 + st["reused_stream_bytes"]] == data[24:24 + st["reused_stream_bytes"]] and want != data


def test_an_entry_added_in_front_and_one_dropped(csa, twelve):
    """the new entry's task is the largest, so it sorts first: every stream moves right by more than any stream is long; the dropped
    entry's task leaves a hole the ones behind it close"""
    data, items = twelve(2)
    entries, content = _mk(csa, _with(items, {"t/new.zzz": cases.build([["random", 8, 0, 95000]]), "t/f05.e05": None}))
    st, ost, want = _check(csa, data, entries, content, "sums", OPTS12)
    assert _status(st) == [NEW] + [REUSED] * 11 and st["parked_moves"] == 0
    assert st["moved_bytes"] == st["reused_stream_bytes"] and st["moves"] == 2


# ---- 3. bases whose streams do not lie back to back in id order -----------------------------------------------------------------

@pytest.mark.parametrize("mode", ["verify", "sums"])
def test_interleaved_base_extents(csa, mixed, codec, mode):  # noqa: F811
    data, content = mixed
    chopped, ab = _rechop(data, orc_csa.parse(data, codec[1]), codec)
    entries, _ = _entries(csa, "mixed_tree")
    st, ost, want = _check(csa, chopped, entries, content, mode, _opts("mixed_tree"), fresh=False)
    assert want == data != chopped and _status(st) == [REUSED] * 3
    assert st["moved_bytes"] > 0 and st["moves"] > 3


def test_streams_in_reverse_id_order_are_parked(csa, mixed, codec):  # noqa: F811
    data, content = mixed
    info = orc_csa.parse(data, codec[1])
    body, ab = bytearray(), {}
    for bid in sorted(info["abindex"], reverse=True):
        s = b"".join(data[o:o + n] for o, n in info["abindex"][bid])
        ab[bid] = [(24 + len(body), len(s))]
        body += s
    base = _reindex(data, info, codec, body=body, abindex=ab)
    assert base != data and base[24:24 + len(body)] == bytes(body)
    entries, _ = _entries(csa, "mixed_tree")
    st, ost, want = _check(csa, base, entries, content, "sums", _opts("mixed_tree"), fresh=False)
    assert want == data and _status(st) == [REUSED] * 3
    assert st["parked_moves"] > 0 and st["parked_bytes"] > 0 and st["move_launches"] >= 2


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------

def test_spare_capacity_is_grown_into(csa, twelve):
    import torch
    data, items = twelve(2)
    spare = 64 << 10
    room = torch.full((len(data) + spare + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    entries, _ = _mk(csa, items)
    rc, arc, _ = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, arc=room[:len(data) + spare], **OPTS12)
    assert rc == 0 and _bytes(arc) == data and arc.data_ptr() == room.data_ptr()
    entries, content = _mk(csa, _with(items, {"t/f00a.e00": cases.build([["random", 9, 0, 40000]])}))
    want, ost, _ = _yardstick(csa, data, entries, "sums", OPTS12)
    assert len(data) < len(want) <= len(data) + spare
    with csa.DeviceArchive.open(arc) as a:
        rc, view, st = a.update_in_place(entries, buf=room[:len(data) + spare], arcname=csa_cases.ARCNAME, trust_sums=True, **OPTS12)
        assert rc == 0 and _bytes(view) == want and _status(st) == _status(ost)
        assert _bytes(room[len(data) + spare:]) == b"\xa5" * GUARD
        rc, views, xst = a.extract()
        assert rc == 0 and xst["verify_failures"] == 0 and {n: _bytes(v) for n, v in views.items()} == content


def test_exact_capacity_and_one_byte_less(csa, twelve):
    data, items = twelve(2)
    entries, content = _mk(csa, _with(items, {FIRST: cases.build([["random", 7, 0, 88000]])}))
    st, ost, want = _check(csa, data, entries, content, "sums", OPTS12, cap=None)
    assert len(want) > len(data) + 1, "buf_cap == the new archive's size succeeded (and is more than the base's)"
    ip = InPlace(csa, data, len(want) - 1)
    try:
        rc, view, st = ip.run(entries, "sums", OPTS12)
        assert rc == csa.WRITE_ERROR
        ip.extracts(dict(items))                   # the object still describes the base
    finally:
        ip.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_buffer_alone(csa, mixed, codec):  # noqa: F811
    data, content = mixed
    opts = _opts("mixed_tree")
    entries, _ = _entries(csa, "mixed_tree")
    ip = InPlace(csa, data, len(data) + 8192)
    try:
        table = ip.a.digests()[1]
        # both trust flags; TRUST_DIGESTS without a table
        rc, _, st = ip.a.update_in_place(entries, buf=ip.room[:ip.cap], arcname=csa_cases.ARCNAME, trust_sums=True, trust_digests=True,
                                         base_digests=table, **opts)
        assert rc == -1 and _bytes(ip.room[:len(data)]) == data
        assert ip.run(entries, "digests", opts, table=None)[0] == -1
        # a hull overlapping the buffer: an entry that lies in the spare room behind the archive, and one inside the archive
        for lo in (len(data), 100):
            inside = [dict(e) for e in entries]
            k = next(i for i, e in enumerate(inside) if e["name"] == "d/noext")                     # (5000 bytes)
            inside[k]["tensor"] = ip.room[lo:lo + inside[k]["tensor"].numel()]
            rc, _, st = ip.a.update_in_place(inside, buf=ip.room[:ip.cap], arcname=csa_cases.ARCNAME, trust_sums=True, **opts)
            assert rc == -1 and (st["launches"], st["check_launches"], st["move_launches"]) == (0, 0, 0)
            assert _bytes(ip.room[:len(data)]) == data
        # buf_cap < arc_size: the Python layer refuses a smaller tensor and one that begins elsewhere; the library refuses the size
        with pytest.raises(ValueError):
            ip.a.update_in_place(entries, buf=ip.room[:len(data) - 1], arcname=csa_cases.ARCNAME, **opts)
        with pytest.raises(ValueError):
            ip.a.update_in_place(entries, buf=ip.room[1:ip.cap], arcname=csa_cases.ARCNAME, **opts)
        whole = ip.a._arc
        ip.a._arc = whole[:len(data) - 1]          # (so that the default buf is one byte short of the handle's archive)
        rc, _, st = ip.a.update_in_place(entries, arcname=csa_cases.ARCNAME, trust_sums=True, **opts)
        ip.a._arc = whole
        assert rc == -1 and st["check_launches"] == 0 and _bytes(ip.room[:len(data)]) == data
        ip.extracts(content)
        assert ip.run(entries, "sums", opts)[0] == 0, "and the handle is still good for an update"
    finally:
        ip.close()
    # a reused stream cut short in the base: one byte off its last extent, the index adjusted
    info = orc_csa.parse(data, codec[1])
    ab = {bid: list(v) for bid, v in info["abindex"].items()}
    o, n = ab[1][-1]
    ab[1][-1] = (o, n - 1)
    ip = InPlace(csa, _reindex(data, info, codec, abindex=ab), len(data) + 8192)
    try:
        rc, _, st = ip.run(entries, "sums", opts)
        assert rc == -1 and _status(st) == [REUSED] * 3 and st["move_launches"] == 0
    finally:
        ip.close()


# ---- 6. again and again inside one buffer ---------------------------------------------------------------------------------------

def test_three_updates_in_a_row_on_one_object(csa, twelve):
    data, items = twelve(2)
    ip = InPlace(csa, data, len(data) + (256 << 10))
    try:
        rc, table, _ = ip.a.digests()
        assert rc == 0
        for step, (name, new) in enumerate([("t/f03a.e03", cases.build([["random", 21, 0, 40900]])), (FIRST, bytes(88000)),
                                            ("t/f07.e07", cases.build([["text", 23, 0, 80000]]))]):
            items = _with(items, {name: new})
            entries, content = _mk(csa, items)
            before = ip.base
            rc, view, st = ip.run(entries, "digests", OPTS12, table=table, digests=True)
            assert rc == 0 and _status(st).count(CHANGED) == 1 and _status(st).count(REUSED) == 11, step
            assert _bytes(view) == _fresh(csa, entries, **OPTS12)[0] != before
            ip.extracts(content)
            table = st["digests"]
        rc, _, dst = ip.a.digests(expect=table)
        assert rc == 0 and dst["mismatches"] == 0 and dst["first_mismatch"] == csa.NO_MISMATCH and dst["verify_failures"] == 0
    finally:
        ip.close()


# ---- 7. a few hundred chunks through the flag chain -------------------------------------------------------------------------------

def test_a_move_of_nine_mib_by_a_few_bytes(csa):
    """the tasks lie largest first, so the stream that changes size lies in FRONT of the large one only if its task is larger: 9 MiB and
    64 KiB of zeros with a few other bytes, whose stream is a few hundred bytes, in front of 9 MiB that do not compress"""
    import torch
    opts = dict(level=1, dict_size=1 << 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    big = torch.randint(0, 256, (9 << 20,), dtype=torch.uint8, device="cuda", generator=g)
    front = torch.zeros((9 << 20) + (64 << 10), dtype=torch.uint8, device="cuda")

    def entries():
        return [{"name": "m/a.zer", "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": front},
                {"name": "m/b.rnd", "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": big}]
    rc, arc, bst = csa.DeviceArchive.write_tensors(entries(), arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0 and bst["tasks"] == 2
    data = _bytes(arc)
    front[4 << 20:(4 << 20) + 100] = torch.randint(0, 256, (100,), dtype=torch.uint8, device="cuda", generator=g)
    want, ost, _ = _yardstick(csa, data, entries(), "sums", opts)
    shift = int.from_bytes(want[8:16], "little") - int.from_bytes(data[8:16], "little")
    assert 0 < abs(shift) < CHUNK and _status(ost) == [CHANGED, REUSED]
    ip = InPlace(csa, data, max(len(want), len(data)))
    try:
        rc, view, st = ip.run(entries(), "sums", opts)
        assert rc == 0 and _status(st) == [CHANGED, REUSED]
        assert (st["moves"], st["parked_moves"], st["move_launches"]) == (1, 0, 1) and st["moved_bytes"] == st["reused_stream_bytes"] > 8 << 20
        assert torch.equal(view.cpu(), torch.frombuffer(bytearray(want), dtype=torch.uint8)), "byte for byte the out-of-place update's archive"
        rc, views, xst = ip.a.extract()
        assert rc == 0 and xst["verify_failures"] == 0 and torch.equal(views["m/b.rnd"], big) and torch.equal(views["m/a.zer"], front)
    finally:
        ip.close()
