"""GPU tier for the fragment digests of the device archive (include/csa_mi355x.h: CSAMI_DeviceDigestSlices, CSAMI_DeviceUpdateDigests,
CSAMI_DeviceReadDigests; csc_amd.csa.DeviceArchive.digest_slices / write_tensors / write_slices / update / digests): one BLAKE2s
tree-mode digest per fragment of the index in a table in HBM, which the next update trusts in the place of a decode.  The checker is
csc_amd.csa.fragment_digest -- hashlib with stock parameters -- over fragment bounds that come from listing the archives."""
import hashlib
import json
import os
import sys

import pytest

import cases
import csa_cases
import csa_write_cases
from test_gpu_archive_device import _rechop, codec  # noqa: F401
from test_gpu_archive_write_slices import Scattered

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

REUSED, NEW, PROPS, CHANGED, BASE_BAD = range(5)
SIZES = [0, 1, 55, 63, 64, 65, 127, 128, 16383, 16384, 16385, 32768, 49153]          # the model's
NO_MISMATCH = (1 << 64) - 1


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


def _opts(case="mixed_tree"):
    return {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}


def _rows(table):
    return [r.hex() for r in _split(_bytes(table))]


def _split(b):
    return [b[i:i + 32] for i in range(0, len(b), 32)]


def _want(csa, arc_bytes, content, dec):
    """the digest table of an archive: hashlib over every fragment of its listing, the entries in byte-wise name order"""
    index = orc_csa.parse(arc_bytes, dec)["index"]
    out = []
    for name in sorted(index, key=lambda n: n.encode("latin-1") if isinstance(n, str) else bytes(n)):
        for f in index[name]["frags"]:
            out.append(csa.fragment_digest(content.get(name, b"")[f["posfile"]:f["posfile"] + f["size"]]).hex())
    return out


def _entries(csa, case="mixed_tree", changed=None, off=0, extra=()):
    """-> (entries for write_tensors / update, {name: content}); every tensor `off` bytes behind an allocation's start"""
    table, _, content = csa_write_cases.table(case, _edate(csa))
    content.update(changed or {})
    out = []
    for f in table:
        data = content.get(f["name"])
        out.append({"name": f["name"], "edate": f["edate"], "eattr": f["eattr"], "tensor": _upload(data, off) if data else None})
    for name, data in extra:
        content[name] = data
        out.append({"name": name, "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": _upload(data, off) if data else None})
    return out, content


def _single(n):
    return bytes(cases.build([["delta", 1000 + n, 0, n]])) if n else b""


EXTRA = [(f"s/{n:05d}.q{k:02d}", _single(n)) for k, n in enumerate(SIZES)]          # an extension each: no two share a task's tail


@pytest.fixture(scope="module")
def mixed(csa, codec):  # noqa: F811
    """mixed_tree written once with its table: (archive tensor, its bytes, {name: content}, the table tensor, the hashlib table)"""
    entries, content = _entries(csa)
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, digests=True, **_opts())
    assert rc == 0
    data = _bytes(arc)
    return arc, data, content, st["digests"], _want(csa, data, content, codec[1])


def _collision(csa, old):
    i = next(k for k in range(1000, len(old) - 2) if old[k] < 255 and old[k + 1] >= 2 and old[k + 2] < 255)
    b = bytearray(old); b[i] += 1; b[i + 1] -= 2; b[i + 2] += 1
    assert bytes(b) != old and csa.adler32(bytes(b)) == csa.adler32(old)
    return bytes(b)


def _status(st):
    return [t["status"] for t in st["tasks"]]


def _update(csa, base, entries, **kw):
    mine = [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries]
    theirs = _bytes(base)
    with csa.DeviceArchive.open(base) as a:
        rc, out, st = a.update(entries, arcname=csa_cases.ARCNAME, **kw)
    assert [None if e["tensor"] is None else _bytes(e["tensor"]) for e in entries] == mine, "nothing of the caller's is written"
    assert _bytes(base) == theirs, "nothing of the base is written"
    return rc, (None if out is None else _bytes(out)), st


def _zeroed(st):
    return all(st[k] == 0 for k in ("launches", "encode_launches", "check_launches", "candidates", "upload_bytes", "digest_launches", "digest_frags",
                                    "digested_bytes", "mismatches", "first_mismatch"))


# ---- 1. digest_slices ----------------------------------------------------------------------------------------------------------

def test_digest_slices_is_hashlib_over_every_fragment_at_every_alignment(csa, codec):  # noqa: F811
    entries, content = _entries(csa, extra=EXTRA)
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **_opts())
    assert rc == 0
    want = _want(csa, _bytes(arc), content, codec[1])
    assert len(want) == csa.device_write_frag_count([dict(e, esize=0 if e["tensor"] is None else e["tensor"].numel()) for e in entries], **_opts())[1]
    assert set(csa.fragment_digest(d).hex() for _, d in EXTRA) <= set(want), "each extra entry is one fragment"
    for off in range(16):
        entries, _ = _entries(csa, off=off, extra=EXTRA)
        rc, table, ds = csa.DeviceArchive.digest_slices(entries, arcname=csa_cases.ARCNAME, **_opts())
        assert rc == 0 and _rows(table) == want, off
        assert (ds["digest_frags"], ds["digest_launches"], ds["mismatches"], ds["first_mismatch"]) == (len(want), 2, 0, NO_MISMATCH)
        assert ds["digested_bytes"] == sum(len(c) for c in content.values())
        assert ds["digest_leaves"] == sum(max(1, -(-len(c) // 16384)) for c in content.values()), "every entry here is one fragment"


# ---- 2. the write with a table ---------------------------------------------------------------------------------------------------

def test_write_with_digests_writes_the_same_archive(csa, mixed):
    arc, data, content, table, want = mixed
    entries, _ = _entries(csa)
    rc, plain, pst = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **_opts())
    rc2, again, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, digests=True, **_opts())
    assert rc == rc2 == 0 and _bytes(plain) == _bytes(again) == data
    assert _rows(st["digests"]) == _rows(table) == want
    assert st["launches"] <= 5 * st["waves"] + 2 and st["digest_launches"] == 2
    same = ("tasks", "frags", "waves", "blocks", "launches", "encode_launches", "readback_bytes", "upload_bytes", "raw_bytes", "archive_bytes",
            "index_raw_size", "index_compressed_size", "n_entries", "retries")
    assert {k: st[k] for k in same} == {k: pst[k] for k in same}, "every existing statistic is what it is without the table"
    assert csa.DeviceArchive.digest_slices(entries, arcname=csa_cases.ARCNAME, **_opts())[1].cpu().tolist() == table.cpu().tolist()


# ---- 3. strided entries ----------------------------------------------------------------------------------------------------------

def test_strided_entries_are_digested_as_their_packed_bytes(csa, codec):  # noqa: F811
    rows = [("m/cols.bin", bytes(cases.build([["delta", 5, 0, 96 * 700]])), 96, 256, 700),          # a column block: 67200 bytes, five leaves
            ("m/thin.dat", bytes(cases.build([["delta", 6, 0, 5 * 4000]])), 5, 9, 4000),             # run < 16
            ("m/full.txt", bytes(cases.build([["delta", 7, 0, 64 * 300]])), 64, 64, 300),            # run == stride
            ("m/none.txt", b"", 0, 0, 0)]
    sc = Scattered(csa, rows)
    rc, arc, st = csa.DeviceArchive.write_slices(sc.entries, arcname=csa_cases.ARCNAME, digests=True, level=2)
    rc2, flat, fst = csa.DeviceArchive.write_tensors(sc.packed, arcname=csa_cases.ARCNAME, digests=True, level=2)
    assert rc == rc2 == 0 and sc.unchanged() and _bytes(arc) == _bytes(flat)
    want = _want(csa, _bytes(arc), sc.content, codec[1])
    assert len(want) == 4 and _rows(st["digests"]) == _rows(fst["digests"]) == want
    rc, table, ds = csa.DeviceArchive.digest_slices(sc.entries, arcname=csa_cases.ARCNAME, level=2)
    assert rc == 0 and _rows(table) == want and sc.unchanged()
    for (name, content, *_), e in zip(rows, sc.entries):          # and each one alone (an empty file alone gets no task and no fragment)
        rc, table, ds = csa.DeviceArchive.digest_slices([e], arcname=csa_cases.ARCNAME, level=2)
        assert rc == 0 and _rows(table) == ([csa.fragment_digest(content).hex()] if content else []), name


# ---- 4. the collision -------------------------------------------------------------------------------------------------------------

def test_equal_sums_are_told_apart_by_the_digests(csa, mixed):
    base, data, content, table, want = mixed
    new = _collision(csa, content["d/a.txt"])
    entries, _ = _entries(csa, changed={"d/a.txt": new})
    rc, fresh, _ = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **_opts())
    assert rc == 0
    rc, got, st = _update(csa, base, entries, base_digests=table, trust_digests=True, **_opts())
    assert rc == 0 and _status(st) == [CHANGED, REUSED, REUSED]
    assert got == _bytes(fresh) != data
    assert st["decoded_bytes"] == st["decode_launches"] == 0
    assert st["mismatches"] == 1 and st["check_launches"] == 3 * st["check_waves"] and st["launches"] <= 5 * st["waves"] + 2
    # (what the sums alone make of it: the old bytes under the new table)
    rc, got, st = _update(csa, base, entries, trust_sums=True, **_opts())
    assert rc == 0 and _status(st) == [REUSED] * 3 and got == data


# ---- 5. nothing changed, and the table handed on ---------------------------------------------------------------------------------

def test_nothing_changed_hands_the_table_on(csa, mixed):
    base, data, content, table, want = mixed
    entries, _ = _entries(csa)
    rc, got, st = _update(csa, base, entries, base_digests=table, trust_digests=True, digests=True, **_opts())
    assert rc == 0 and _status(st) == [REUSED] * 3 and got == data
    assert st["decoded_bytes"] == st["decode_launches"] == 0 and (st["mismatches"], st["first_mismatch"]) == (0, NO_MISMATCH)
    assert _rows(st["digests"]) == _rows(table) == want
    assert st["digests"].data_ptr() != table.data_ptr()
    # the output table is the base table of the next update, over the archive just written
    b = bytearray(content["d/sub/c.exe"]); b[100] ^= 0x10
    entries2, _ = _entries(csa, changed={"d/sub/c.exe": bytes(b)})
    rc, fresh, _ = csa.DeviceArchive.write_tensors(entries2, arcname=csa_cases.ARCNAME, **_opts())
    rc2, got2, st2 = _update(csa, _upload(got, 3), entries2, base_digests=st["digests"], trust_digests=True, digests=True, **_opts())
    assert rc == rc2 == 0 and _status(st2) == [REUSED, CHANGED, REUSED] and got2 == _bytes(fresh)
    changed = [i for i, (x, y) in enumerate(zip(_rows(st2["digests"]), want)) if x != y]
    assert len(changed) == 1 and st2["first_mismatch"] == changed[0] and _rows(st2["digests"])[changed[0]] == csa.fragment_digest(bytes(b)).hex()


# ---- 6. one flipped bit in the base table -----------------------------------------------------------------------------------------

def test_a_flipped_bit_in_the_base_table_encodes_that_task(csa, mixed, codec):  # noqa: F811
    base, data, content, table, want = mixed
    index = orc_csa.parse(data, codec[1])["index"]
    names = sorted(index, key=lambda n: n.encode("latin-1"))
    at = [(n, f["bid"]) for n in names for f in index[n]["frags"]]
    entries, _ = _entries(csa)
    for which in ("d/b.txt", "d/empty"):                                   # (the empty entry's fragment has a digest too)
        i = next(k for k, (n, _) in enumerate(at) if n == which)
        bad = table.clone()
        bad[i, 17] ^= 0x04
        rc, got, st = _update(csa, base, entries, base_digests=bad, trust_digests=True, **_opts())
        assert rc == 0 and got == data, "the task is encoded again, to the same stream"
        assert _status(st) == [CHANGED if b == at[i][1] else REUSED for b in range(3)]
        assert (st["mismatches"], st["first_mismatch"]) == (1, i)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals(csa, mixed):
    import torch
    base, data, content, table, want = mixed
    entries, _ = _entries(csa)
    n = table.shape[0]
    longer = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
    longer[:n] = table
    room = torch.full((len(data) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    inside = room[len(data) - 32:len(data) - 32 + 32 * n].view(n, 32)
    refused = [("a table one row too long", dict(base_digests=longer, trust_digests=True)),
               ("a table one row too short", dict(base_digests=table[:n - 1], trust_digests=True)),
               ("both trust flags", dict(base_digests=table, trust_digests=True, trust_sums=True)),
               ("trust_digests without a table", dict(trust_digests=True)),
               ("the base table inside arc", dict(base_digests=inside, trust_digests=True, arc=room[:len(data)])),
               ("the output table inside arc", dict(digests=inside, arc=room[:len(data)])),
               ("the output table is the base table", dict(base_digests=table, digests=table, trust_digests=True))]
    for what, kw in refused:
        rc, got, st = _update(csa, base, entries, **dict(_opts(), **kw))
        assert rc == -1 and _zeroed(st), what
    assert _bytes(room) == b"\xa5" * room.numel()
    # the output table over a caller's buffer
    t = next(e["tensor"] for e in entries if e["tensor"] is not None and e["tensor"].numel() >= 32 * n)
    rc, got, st = _update(csa, base, entries, **dict(_opts(), digests=t[:32 * n].view(n, 32)))
    assert rc == -1 and _zeroed(st)
    # room for one digest less than the plan's fragments
    short = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    rc, got, st = _update(csa, base, entries, **dict(_opts(), digests=short[:n - 1], arc=room[:len(data)]))
    assert rc == csa.WRITE_ERROR and _zeroed(st)
    assert _bytes(short) == b"\xa5" * (32 * n) and _bytes(room) == b"\xa5" * room.numel()
    rc, tab, ds = csa.DeviceArchive.digest_slices(entries, arcname=csa_cases.ARCNAME, **_opts())
    assert rc == 0


# ---- 8. the table of an archive ----------------------------------------------------------------------------------------------------

def _digests(csa, arc_bytes, off, want, expect=None):
    with csa.DeviceArchive.open(_upload(arc_bytes, off)) as a:
        rc, table, st = a.digests(expect=expect, **_opts())
        tst = a.test(**_opts())[1]
    assert _rows(table) == want
    assert all(st[k] == tst[k] for k in ("tasks", "frags", "waves", "launches", "decode_launches", "raw_bytes")), "the read is csarc t's"
    return rc, table, st


def test_the_table_of_an_archive(csa, mixed, codec):  # noqa: F811
    base, data, content, table, want = mixed
    rc, got, st = _digests(csa, data, 0, want)
    assert rc == 0 and st["verify_failures"] == 0 and st["digest_frags"] == len(want) and st["mismatches"] == 0
    assert st["digest_launches"] == 2 * (st["waves"] + 1), "a pass a wave, and one for the empty fragments"
    # the base cut into other blocks: the streams are gathered, the table is the same
    chopped, _ = _rechop(data, orc_csa.parse(data, codec[1]), codec)
    rc, got, st = _digests(csa, chopped, 5, want, expect=table)
    assert rc == 0 and (st["verify_failures"], st["mismatches"], st["first_mismatch"]) == (0, 0, NO_MISMATCH)
    # an archive the reference wrote
    with open(os.path.join(ROOT, "tests", "golden", "csa.json")) as f:
        golden = json.load(f)["named_files_m3"]
    entries, gcontent = _entries(csa, "named_files_m3")
    rc, garc, _ = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, **_opts("named_files_m3"))
    assert rc == 0 and hashlib.sha256(_bytes(garc)).hexdigest() == golden["archive_sha256"], "byte for byte the reference's archive"
    gwant = _want(csa, _bytes(garc), gcontent, codec[1])
    with csa.DeviceArchive.open(garc) as a:
        rc, gtable, gst = a.digests(**_opts("named_files_m3"))
    assert rc == 0 and _rows(gtable) == gwant and gst["verify_failures"] == 0
    # one flipped digest in the expected table, of a fragment with bytes and of an empty one
    for i in (next(k for k, w in enumerate(want) if w != csa.fragment_digest(b"").hex()), want.index(csa.fragment_digest(b"").hex())):
        bad = table.clone()
        bad[i, 0] ^= 1
        keep = _bytes(bad)
        rc, got, st = _digests(csa, data, 1, want, expect=bad)
        assert (st["mismatches"], st["first_mismatch"], st["verify_failures"]) == (1, i, 1), "a mismatch counts as a failed checksum does"
        assert _bytes(bad) == keep, "the expected table is only read"


# ---- 9. nothing written outside the contracts ------------------------------------------------------------------------------------

def test_canaries_around_the_output_table(csa, mixed):
    import torch
    base, data, content, table, want = mixed
    entries, _ = _entries(csa)
    n = table.shape[0]
    for lead in (1, 16):
        room = torch.full((lead + 32 * n + 7,), 0xC3, dtype=torch.uint8, device="cuda")
        out = room[lead:lead + 32 * n].view(n, 32)
        keep = _bytes(table)
        rc, got, st = _update(csa, base, entries, base_digests=table, trust_digests=True, digests=out, **_opts())
        assert rc == 0 and got == data and _rows(out) == want
        assert _bytes(room[:lead]) == b"\xc3" * lead and _bytes(room[lead + 32 * n:]) == b"\xc3" * 7
        assert _bytes(table) == keep, "the base table is only read"
        room.fill_(0xC3)
        rc, got, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, digests=out, **_opts())
        assert rc == 0 and _bytes(got) == data and _rows(out) == want
        assert _bytes(room[:lead]) == b"\xc3" * lead and _bytes(room[lead + 32 * n:]) == b"\xc3" * 7


# ---- 10. more than one wave --------------------------------------------------------------------------------------------------------

def test_more_than_one_wave_gives_the_same_tables(csa, mixed):
    base, data, content, table, want = mixed
    entries, _ = _entries(csa)
    how = dict(_opts(), hbm_budget=1 << 20, device_streams=1)
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, arcname=csa_cases.ARCNAME, digests=True, **how)
    assert rc == 0 and st["waves"] >= 2 and _bytes(arc) == data and _rows(st["digests"]) == want and st["digest_launches"] == 2
    new = _collision(csa, content["d/a.txt"])
    entries2, _ = _entries(csa, changed={"d/a.txt": new})
    rc, fresh, _ = csa.DeviceArchive.write_tensors(entries2, arcname=csa_cases.ARCNAME, **_opts())
    one = _update(csa, base, entries2, base_digests=table, trust_digests=True, digests=True, **_opts())
    many = _update(csa, base, entries2, base_digests=table, trust_digests=True, digests=True, **how)
    assert one[0] == many[0] == rc == 0 and many[2]["waves"] >= 2 and many[2]["check_waves"] >= 2
    assert one[1] == many[1] == _bytes(fresh) and _status(one[2]) == _status(many[2]) == [CHANGED, REUSED, REUSED]
    assert _rows(one[2]["digests"]) == _rows(many[2]["digests"])
    with csa.DeviceArchive.open(base) as a:
        rc, t2, st2 = a.digests(**how)
    assert rc == 0 and st2["waves"] >= 2 and _rows(t2) == want
