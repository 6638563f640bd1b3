"""GPU tier for entries gathered from strided slices of the caller's buffers (include/csa_mi355x.h: CSAMI_DeviceWriteSlices;
csc_amd.csa.DeviceArchive.write_slices, csa.tensor_slice).  An entry's bytes are what its slice selects of a buffer, packed row
after row, and the archive must be byte for byte the one the contiguous write (write_tensors over the packed bytes -- the path the
neighbouring files pin to the reference's goldens) gives, or the golden itself where there is one.

`scatter` lays an entry's packed content out under its slice in a buffer of offset + hull + 5 bytes in which every byte that is not
selected is 0xA5 -- on the host, then uploaded; after every call the buffers must be byte for byte what they were."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import cases
import csa_cases
import csa_write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = ["mixed_tree", "named_files_m3", "single_split3"]
GAPS = (1, 15, 16, 17, 4099)
GATHER_KEYS = ["selected_bytes", "hull_bytes", "periodic_pieces", "plain_pieces", "gathered_tasks", "inplace_tasks"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "csa.json")) as f:
        return json.load(f)


def _edate(csa, t=csa_cases.MTIME):
    return int(csa.lib().CSA_DecimalTime(int(t)))


def _bytes(view):
    return view.cpu().numpy().tobytes()


def _upload(data):
    import torch
    t = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _hull(s):
    return (s[3] - 1) * s[2] + s[1] if s[3] else 0


def scatter(content, run, stride, count, i, offset=None):
    """-> (host bytes of the buffer, the slice): `content`, run * count bytes, under (offset, run, stride, count) in a buffer of
    offset + hull + 5 bytes, offset = 1 + 3 * i unless given; every byte that is not selected is 0xA5"""
    assert len(content) == run * count and (count <= 1 or stride >= run)
    offset = 1 + 3 * i if offset is None else offset
    s = (offset, run, stride if count > 1 else run, count)
    buf = np.full(offset + _hull(s) + 5, 0xA5, dtype=np.uint8)
    if count:
        rows = np.lib.stride_tricks.as_strided(buf[offset:], shape=(count, run), strides=(s[2], 1))
        rows[:] = np.frombuffer(content, dtype=np.uint8).reshape(count, run)
    return buf.tobytes(), s


class Scattered:
    """entries [(name, content, run, stride, count)] scattered and uploaded; .entries for write_slices, .packed for write_tensors"""

    def __init__(self, csa, rows, offsets=None, eattr=csa_write_cases.FILE_ATTR):
        self.host, self.entries, self.packed, self.content = [], [], [], {}
        for i, (name, content, run, stride, count) in enumerate(rows):
            row = {"name": name, "edate": _edate(csa), "eattr": eattr}
            if content is None:                                    # a directory
                self.host.append(None)
                self.entries.append(dict(row, eattr=csa_write_cases.DIR_ATTR, tensor=None, slice=None))
                self.packed.append(dict(row, eattr=csa_write_cases.DIR_ATTR, tensor=None))
                continue
            host, s = scatter(content, run, stride, count, i, None if offsets is None else offsets[i])
            self.host.append(host)
            self.content[name] = content
            self.entries.append(dict(row, tensor=_upload(host), slice=s))
            self.packed.append(dict(row, tensor=_upload(content) if content else None))

    def unchanged(self):
        return all(h is None or _bytes(e["tensor"]) == h for h, e in zip(self.host, self.entries))


def _write_slices(csa, sc, **kw):
    rc, arc, st = csa.DeviceArchive.write_slices(sc.entries, **kw)
    assert sc.unchanged(), "nothing of the caller's is written"
    if rc == 0:
        assert st["archive_bytes"] == arc.numel() and st["launches"] <= 5 * st["waves"] + 2
        assert st["selected_bytes"] == sum(len(c) for c in sc.content.values()) == st["raw_bytes"]
        assert st["hull_bytes"] == sum(_hull(e["slice"]) for e in sc.entries if e["slice"])
    return rc, arc, st


def _contiguous(csa, sc, **kw):
    rc, arc, st = csa.DeviceArchive.write_tensors(sc.packed, **kw)
    assert rc == 0
    return _bytes(arc), st


# ---- 1. goldens of the reference ----------------------------------------------------------------------------------------

def _rows_of(esize):
    count = max(c for c in range(1, 65) if esize % c == 0)
    return esize // count, count


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_sliced_write_is_the_reference_archivers(csa, golden, case):
    table, _, content = csa_write_cases.table(case, _edate(csa))
    rows, counts = [], []
    for i, f in enumerate(table):
        if f["eattr"] == csa_write_cases.DIR_ATTR:
            rows.append((f["name"], None, 0, 0, 0))
        elif not f["esize"]:
            rows.append((f["name"], b"", 0, 0, 0))
        else:
            run, count = _rows_of(f["esize"])
            counts.append(count)
            rows.append((f["name"], content[f["name"]], run, run + GAPS[i % 5], count))
    assert counts and all(c > 1 for c in counts), "every non-empty entry is rows with gaps between them"
    assert sorted(counts) == sorted({"mixed_tree": [60, 56, 64, 60, 50], "named_files_m3": [64, 60], "single_split3": [64]}[case])
    sc = Scattered(csa, rows)
    opts = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}
    rc, arc, st = _write_slices(csa, sc, arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0
    assert hashlib.sha256(_bytes(arc)).hexdigest() == golden[case]["archive_sha256"]
    assert st["periodic_pieces"] > 0 and st["inplace_tasks"] == 0 and 1 <= st["gathered_tasks"] <= st["tasks"]
    if case == "single_split3":
        assert rows[0][2] == 81920 > 16384 and st["tasks"] == 3, "runs longer than a piece, and fragments that begin inside a run"


# ---- 2. alignments and small runs ---------------------------------------------------------------------------------------

RUNS = [1, 3, 7, 15, 16, 17, 31, 33, 4097]
COUNTS = [1, 2, 5, 1000]


def _small_rows(ext):
    """48 entries: every run with every count (5 and 1000 capped so that no entry passes 40 KiB) and with at least three of the
    strides run, run + 1, run + 13.  Then run = 16384, a piece exactly: one row of it, two rows of it, and the byte range of 16385
    bytes next to it (no run * count with run = 16384 gives that size).  ext(i): the extension of entry i."""
    rows = []
    for i in range(48):
        q, j = divmod(i, 9)
        run, count = RUNS[j], COUNTS[(q + j) % 4]
        if count > 2:
            count = min(count, 40960 // run)
        rows.append((f"s/e{i:02d}.{ext(i)}", cases.build([["text", 300 + i, 0, run * count]]), run, run + (0, 1, 13)[(j + q) % 3], count))
    for k, (run, count) in enumerate([(16384, 1), (16385, 1), (16384, 2)]):
        rows.append((f"s/e{48 + k}.{ext(48 + k)}", cases.build([["exe", 400 + k, 0, run * count]]), run, run + 13, count))
    return rows


SMALL_OPTS = dict(level=1, dict_size=64 << 10)


@pytest.fixture(scope="module")
def small(csa):
    """the second test's entries in one extension: (Scattered, the sliced write's archive bytes and stats, the device archive)"""
    sc = Scattered(csa, _small_rows(lambda i: "bin"), offsets=[i % 16 for i in range(51)])
    rc, arc, st = _write_slices(csa, sc, **SMALL_OPTS)
    assert rc == 0
    return sc, _bytes(arc), st, arc


def test_alignments_and_small_runs(csa, small):
    sc, data, st, arc = small
    want, st_c = _contiguous(csa, sc, **SMALL_OPTS)
    assert data == want
    seen = {(e["slice"][1], e["slice"][3]) for e in sc.entries}
    assert {r for r, _ in seen} >= set(RUNS) | {16384} and {c for _, c in seen} >= {1, 2, 5, 1000}
    assert st["periodic_pieces"] > 0 and st["gathered_tasks"] >= 1
    assert st["periodic_pieces"] + st["plain_pieces"] >= sum((len(c) + 16383) // 16384 for c in sc.content.values())
    same = ("tasks", "frags", "waves", "blocks", "readback_bytes", "raw_bytes", "archive_bytes")
    assert {k: st[k] for k in same} == {k: st_c[k] for k in same}
    import torch
    with csa.DeviceArchive.open(arc) as a:
        dsts = {n: torch.full((len(c) + 2,), 0xA5, dtype=torch.uint8, device="cuda") for n, c in sc.content.items()}
        rc, rst = a.extract_into({n: t[1:1 + len(sc.content[n])] for n, t in dsts.items()})
        assert rc == 0 and rst["verify_failures"] == 0
        for n, t in dsts.items():
            assert _bytes(t) == b"\xa5" + sc.content[n] + b"\xa5", n


# ---- 3. column blocks -----------------------------------------------------------------------------------------------------

def test_column_blocks_round_trip(csa):
    import torch
    rows_n, width = 200, 1000
    m = np.frombuffer(cases.build([["text", 77, 0, rows_n * width]]), dtype=np.uint8).reshape(rows_n, width)
    dev = _upload(m.tobytes())
    row = {"name": "w", "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    rc, full, _ = csa.DeviceArchive.write_tensors([dict(row, tensor=dev)], level=1)
    assert rc == 0
    bounds = [0, 1, 16, 33, 160, 400, 417, 999, 1000]              # eight ranks; widths 1, 15, 17, 127, 240, 17, 582, 1
    with csa.DeviceArchive.open(full) as whole:
        for c0, c1 in zip(bounds, bounds[1:]):
            s = csa.rows_slice(width, 0, rows_n, c0, c1)
            packed = np.ascontiguousarray(m[:, c0:c1]).tobytes()
            rc, arc, st = csa.DeviceArchive.write_slices([dict(row, tensor=dev, slice=s)], level=1)
            assert rc == 0 and st["selected_bytes"] == len(packed) and st["launches"] <= 5 * st["waves"] + 2
            rc_c, arc_c, _ = csa.DeviceArchive.write_tensors([dict(row, tensor=_upload(packed))], level=1)
            assert rc_c == 0 and _bytes(arc) == _bytes(arc_c), (c0, c1)
            with csa.DeviceArchive.open(arc) as mine:
                rc_x, views, _ = mine.extract()
            rc_s, got, sst = whole.extract_slices({"w": s})
            assert rc_x == rc_s == 0 and sst["verify_failures"] == 0
            assert _bytes(got["w"]) == _bytes(views["w"]) == packed, (c0, c1)
    assert _bytes(dev) == m.tobytes()
    # a block of float32 columns, as a view
    m2d = torch.frombuffer(bytearray(m.tobytes()), dtype=torch.float32).reshape(rows_n, width // 4).cuda()
    view = m2d[:, 37:101]
    base, s = csa.tensor_slice(view)
    assert s == (148, 256, 1000, 200) and base.data_ptr() == m2d.data_ptr() and base.numel() == rows_n * width
    rc, arc, st = csa.DeviceArchive.write_slices([dict(row, tensor=base, slice=s)], level=1)
    rc_c, arc_c, _ = csa.DeviceArchive.write_tensors([dict(row, tensor=view.contiguous().view(-1).view(torch.uint8))], level=1)
    assert rc == rc_c == 0 and _bytes(arc) == _bytes(arc_c)
    assert _bytes(base) == m.tobytes()


# ---- 4. where a task is encoded -----------------------------------------------------------------------------------------

def test_where_a_task_is_encoded(csa):
    content = cases.build([["exe", 5, 0, 160000]])
    opts = dict(level=1, dict_size=64 << 10)
    seen = {}
    for what, rows, kw in [
        ("one range at an odd offset", [("a.bin", content, 160000, 160000, 1)], {}),
        ("the same bytes as two rows", [("a.bin", content, 80000, 80001, 2)], {}),
        ("fragments inside single runs", [("a.bin", content, 40000, 40013, 4)], dict(task_bytes=20000)),
        ("fragments across runs", [("a.bin", content, 32000, 32013, 5)], dict(task_bytes=20000)),
    ]:
        sc = Scattered(csa, rows, offsets=[7])
        rc, arc, st = _write_slices(csa, sc, **opts, **kw)
        want, st_c = _contiguous(csa, sc, **opts, **kw)
        assert rc == 0 and _bytes(arc) == want, what
        assert st["launches"] <= 5 * st["waves"] + 2 and st["tasks"] == st_c["tasks"], what
        seen[what] = {k: st[k] for k in GATHER_KEYS + ["tasks"]}
    print(seen)
    s = seen["one range at an odd offset"]
    assert (s["inplace_tasks"], s["gathered_tasks"], s["periodic_pieces"], s["plain_pieces"]) == (1, 0, 0, 10)
    s = seen["the same bytes as two rows"]
    assert (s["inplace_tasks"], s["gathered_tasks"], s["periodic_pieces"], s["plain_pieces"]) == (0, 1, 1, 9)
    s = seen["fragments inside single runs"]
    assert (s["tasks"], s["inplace_tasks"], s["gathered_tasks"], s["periodic_pieces"], s["plain_pieces"]) == (8, 8, 0, 0, 16)
    s = seen["fragments across runs"]                              # [20000, 40000), [60000, 80000), [80000, 100000), [120000, 140000) cross a border
    assert (s["tasks"], s["inplace_tasks"], s["gathered_tasks"], s["periodic_pieces"]) == (8, 4, 4, 4)


# ---- 5. several waves -------------------------------------------------------------------------------------------------------

def test_several_waves_give_the_same_archive(csa):
    sc = Scattered(csa, _small_rows(lambda i: f"b{i % 6}"), offsets=[i % 16 for i in range(51)])
    rc1, arc1, st1 = _write_slices(csa, sc, **SMALL_OPTS)
    rc2, arc2, st2 = _write_slices(csa, sc, device_streams=2, **SMALL_OPTS)
    assert rc1 == rc2 == 0 and _bytes(arc1) == _bytes(arc2)
    assert st1["waves"] == 1 and st2["tasks"] == st1["tasks"] >= 3 and st2["waves"] == (st2["tasks"] + 1) // 2 > 1
    assert st2["launches"] <= 5 * st2["waves"] + 2
    assert {k: st1[k] for k in GATHER_KEYS} == {k: st2[k] for k in GATHER_KEYS}
    assert _contiguous(csa, sc, **SMALL_OPTS)[0] == _bytes(arc1)


# ---- 6. CSAMI_DeviceWriteFrom is this call with whole-entry slices ------------------------------------------------------------

def test_write_tensors_is_unchanged(csa):
    import torch
    sizes = [0, 1, 15, 16, 17, 4095, 16383, 16384, 16385, 32769, 70001]                  # tests/test_gpu_archive_scatter.py's edge sizes, one task
    entries = []
    for i, n in enumerate(sizes):
        buf = torch.empty(16 + n, dtype=torch.uint8, device="cuda")
        t = buf[(0, 1, 3, 8, 15)[i % 5]:][:n]
        if n:
            t.copy_(torch.frombuffer(bytearray(cases.build([["text", 50 + i, 0, n]])), dtype=torch.uint8))
        entries.append({"name": f"e/f{n:05d}.bin", "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "tensor": t if n else None})
    rc, arc, st = csa.DeviceArchive.write_tensors(entries, **SMALL_OPTS)
    ms = csa.device_write_kernel_ms()
    whole = [dict(e, slice=(0, e["tensor"].numel()) if e["tensor"] is not None else None) for e in entries]
    rc_s, arc_s, st_s = csa.DeviceArchive.write_slices(whole, **SMALL_OPTS)
    assert rc == rc_s == 0 and _bytes(arc) == _bytes(arc_s)
    keys = ["tasks", "frags", "waves", "blocks", "launches", "readback_bytes", "upload_bytes", "raw_bytes", "archive_bytes"]
    assert {k: st[k] for k in keys} == {k: st_s[k] for k in keys}
    assert (st_s["periodic_pieces"], st_s["gathered_tasks"], st_s["inplace_tasks"]) == (0, 1, 0)
    # the reckoning of what crosses the bus (include/csa_mi355x.h), exactly, for this one gathered task: 24 bytes a piece
    assert st["tasks"] == 1 and st["retries"] == 0
    pieces, frags = sum((n + 16383) // 16384 for n in sizes), sum(n > 0 for n in sizes)
    data = _bytes(arc)
    stream = int.from_bytes(data[8:16], "little") - 24 - 10                             # the task's stream behind its property bytes
    istream = st["index_compressed_size"] - 10
    want = (24 * pieces + 24 * frags                                                     # k_frag_pieces' and k_frag_fold's tables
            + 32                                                                         # k_block_table's job
            + 10 + 24 * (1 + (stream + 65535) // 65536)                                  # placement: property bytes, and the pieces
            + st["index_raw_size"]
            + 24 + 10 + 24 * (2 + (istream + 65535) // 65536))                           # the header, the index's property bytes, the pieces
    assert st["upload_bytes"] == want
    assert st["launches"] == 5, "gather and sum, fold, block table, placement; the index's placement"
    assert ms[0] > 0 and all(m >= 0 for m in ms)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def _raw_call(csa, ptrs, sizes, slices, esizes, arc, with_sizes=True, with_slices=True, **opts):
    """CSAMI_DeviceWriteSlices as given -> (rc, write stats, gather stats)"""
    import torch
    n = len(esizes)
    keep = [C.create_string_buffer(f"r{i}.bin".encode()) for i in range(n)]
    files = (csa.CSADevFile * max(n, 1))()
    for f, k, e in zip(files, keep, esizes):
        f.name, f.esize, f.edate, f.eattr = C.cast(k, C.c_void_p), e, _edate(csa), csa_write_cases.FILE_ATTR
    pa = (C.c_void_p * max(n, 1))(*ptrs)
    sa = (C.c_uint64 * max(n, 1))(*sizes)
    sl = (csa.CSADevSlice * max(n, 1))()
    for a, s in zip(sl, slices):
        a.offset, a.run, a.stride, a.count = s
    st, gs, o = csa.CSADevWriteStats(), csa.CSADevGatherStats(), csa.options(**opts)
    for t in (st, gs):
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    torch.cuda.synchronize()
    rc = csa.lib().CSAMI_DeviceWriteSlices(pa, sa if with_sizes else None, sl if with_slices else None, files, n, b"out.csa",
                                           C.c_void_p(arc.data_ptr()), int(arc.numel()), C.byref(o), C.byref(st), C.byref(gs))
    return rc, st, gs


def test_refusals_launch_nothing(csa):
    import torch
    M64 = 1 << 64
    content = cases.build([["text", 9, 0, 6000]])
    host, s = scatter(content, 1000, 1500, 6, 0)                   # offset 1, hull 8500, the buffer 8506 bytes
    big = torch.full((16384 + 65536,), 0xA5, dtype=torch.uint8, device="cuda")
    buf, arc = big[:len(host)], big[16384:]
    buf.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
    p, n = buf.data_ptr(), len(host)

    def refused(what, want, ptrs, sizes, slices, esizes, arc=arc, **kw):
        rc, st, gs = _raw_call(csa, ptrs, sizes, slices, esizes, arc, **kw)
        assert rc == want, what
        assert bytes(st) == bytes(C.sizeof(st)) and bytes(gs) == bytes(C.sizeof(gs)), what
        assert bool((big[len(host):] == 0xA5).all()) and _bytes(buf) == host, what

    ok = _raw_call(csa, [p], [n], [s], [6000], arc)
    assert ok[0] == 0 and ok[1].launches == 5 and ok[2].selected_bytes == 6000 and ok[2].hull_bytes == 8500
    big[len(host):].fill_(0xA5)
    refused("slices == NULL", -1, [p], [n], [s], [6000], with_slices=False)
    refused("sizes == NULL", -1, [p], [n], [s], [6000], with_sizes=False)
    refused("esize one more than run * count", -1, [p], [n], [s], [6001])
    refused("esize one less than run * count", -1, [p], [n], [s], [5999])
    refused("the last selected byte at sizes[i]", -1, [p], [8500], [s], [6000])          # (it is byte 1 + 8500 - 1 of the buffer)
    assert _raw_call(csa, [p], [8501], [s], [6000], arc)[0] == 0, "and one byte more room is enough"
    big[len(host):].fill_(0xA5)
    refused("run == 0 with count > 0", -1, [p], [n], [(1, 0, 5, 3)], [0])
    refused("stride < run with count > 1", -1, [p], [n], [(1, 1000, 999, 6)], [6000])
    refused("(count - 1) * stride wraps", -1, [p], [n], [(1, 1, 1 << 62, 5)], [5])
    refused("offset + hull wraps", -1, [p], [M64 - 1], [(M64 - 8, 1, 8, 2)], [2])
    refused("count == 0 with esize > 0", -1, [p], [n], [(0, 1000, 1500, 0)], [6000])
    refused("a NULL buffer with count > 0", -1, [None], [n], [s], [6000])
    refused("an archive that does not fit", csa.WRITE_ERROR, [p], [n], [s], [6000], arc=big[16384:16384 + 23])
    assert _raw_call(csa, [None, p], [0, n], [(0, 0, 0, 0), s], [0, 6000], arc)[0] == 0, "count == 0 goes with esize == 0 and a NULL buffer"
    big[len(host):].fill_(0xA5)
    # a hull that overlaps arc by a GAP byte only: rows of 1000 bytes 1500 apart, the archive inside the gap behind the first
    wide = torch.full((1 << 17,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, st, gs = _raw_call(csa, [wide.data_ptr()], [wide.numel()], [(0, 1000, 70000, 2)], [2000], wide[1000:70000])
    assert rc == -1 and bytes(st) == bytes(C.sizeof(st)) and bytes(gs) == bytes(C.sizeof(gs)) and bool((wide == 0xA5).all())
    rc, st, gs = _raw_call(csa, [wide.data_ptr()], [wide.numel()], [(0, 1000, 70000, 2)], [2000], wide[71000:])
    assert rc == 0 and bool((wide[:71000] == 0xA5).all()), "touching is fine"
    # a short archive: WRITE_ERROR, and the bytes behind arc_cap untouched
    need = ok[1].archive_bytes
    big[len(host):].fill_(0xA5)
    rc, st, gs = _raw_call(csa, [p], [n], [s], [6000], big[16384:16384 + need - 1])
    assert rc == csa.WRITE_ERROR and bool((big[16384 + need - 1:] == 0xA5).all()) and _bytes(buf) == host
    rc, st, gs = _raw_call(csa, [p], [n], [s], [6000], big[16384:16384 + need])
    assert rc == 0 and st.archive_bytes == need and bool((big[16384 + need:] == 0xA5).all())


# ---- 8. compare closes the loop -------------------------------------------------------------------------------------------

def test_compare_closes_the_loop(csa, small):
    import torch
    sc, data, st, arc = small
    packed = {e["name"]: e["tensor"] for e in sc.packed}
    with csa.DeviceArchive.open(arc) as a:
        rc, diffs, cst = a.compare(packed)
        assert rc == 0 and cst["verify_failures"] == 0 and all(d["status"] == 0 for d in diffs.values())
    # one byte inside a run of one source flipped -- row 3, byte 2000 of an entry of rows of 4097 bytes -- and the archive written again
    k = next(i for i, e in enumerate(sc.entries) if e["slice"][1] == 4097 and e["slice"][3] > 3)
    name, (off, run, stride, count) = sc.entries[k]["name"], sc.entries[k]["slice"]
    flipped = sc.entries[k]["tensor"].clone()
    flipped[off + 3 * stride + 2000] ^= 0x10
    entries = [dict(e, tensor=flipped) if i == k else e for i, e in enumerate(sc.entries)]
    rc, arc2, _ = csa.DeviceArchive.write_slices(entries, **SMALL_OPTS)
    assert rc == 0 and sc.unchanged()
    with csa.DeviceArchive.open(arc2) as a:
        rc, diffs, cst = a.compare(packed)
        assert rc == 0 and cst["verify_failures"] == 0
        assert diffs[name] == {"status": csa.CSA_DIFF_BYTES, "first_diff": 3 * run + 2000, "failed_frags": 0}
        assert all(d["status"] == 0 for n, d in diffs.items() if n != name)
