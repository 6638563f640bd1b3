"""GPU tier for reading into and comparing against strided slices of the caller's buffers (include/csa_mi355x.h:
CSAMI_DeviceReadIntoSlices, CSAMI_DeviceCompareSlices; csc_amd.csa.DeviceArchive.extract_into_slices, compare_slices): the way back of
tests/test_gpu_archive_write_slices.py, whose `scatter` lays an entry's packed content out under its slice in a buffer of offset + hull
+ 5 bytes with 0xA5 in every byte that is not selected.  A read into a buffer that is 0xA5 everywhere must give exactly that buffer:
the selected bytes, and every gap byte, every byte in front of the hull and the five behind it still 0xA5."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import cases
import csa_cases
import csa_write_cases
import test_gpu_archive_write_slices as ws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = ["tasks", "frags", "waves", "launches", "readback_bytes", "raw_bytes", "verify_failures"]
_bytes, _upload, _edate, _hull, scatter, Scattered = ws._bytes, ws._upload, ws._edate, ws._hull, ws.scatter, ws.Scattered


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "csa.json")) as f:
        return json.load(f)


def _blank(n):
    import torch
    return torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")


def _blanks(sc):
    """{name: (a buffer as large as the entry's scattered one, 0xA5 everywhere, the entry's slice)}"""
    return {e["name"]: (_blank(len(h)), e["slice"]) for h, e in zip(sc.host, sc.entries) if h is not None}


def _hosts(sc):
    return {e["name"]: h for h, e in zip(sc.host, sc.entries) if h is not None}


def _read(csa, a, dsts, **kw):
    rc, st = a.extract_into_slices(dsts, **kw)
    assert st["launches"] == 3 * st["waves"]
    return rc, st


# ---- 1. goldens of the reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ws.GOLDEN_CASES)
def test_goldens_are_read_into_slices(csa, golden, case):
    table, _, content = csa_write_cases.table(case, _edate(csa))
    rows = []
    for i, f in enumerate(table):
        if f["eattr"] == csa_write_cases.DIR_ATTR:
            rows.append((f["name"], None, 0, 0, 0))
        elif not f["esize"]:
            rows.append((f["name"], b"", 0, 0, 0))
        else:
            run, count = ws._rows_of(f["esize"])
            rows.append((f["name"], content[f["name"]], run, run + ws.GAPS[i % 5], count))
    sc = Scattered(csa, rows)
    opts = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}
    rc, arc, _ = csa.DeviceArchive.write_tensors(sc.packed, arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0 and hashlib.sha256(_bytes(arc)).hexdigest() == golden[case]["archive_sha256"]
    dsts = {n: d for n, d in _blanks(sc).items() if d[1][3]}
    assert dsts and all(d[1][3] > 1 for d in dsts.values())
    with csa.DeviceArchive.open(arc) as a:
        rc, st = _read(csa, a, dsts)
    assert rc == 0 and st["verify_failures"] == 0 and st["periodic_pieces"] > 0
    for n, (t, _) in dsts.items():
        assert _bytes(t) == _hosts(sc)[n], n


# ---- 2. alignments and small runs ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(csa):
    """the 51 entries of the write's second test, scattered, and the archive write_slices makes of them"""
    sc = Scattered(csa, ws._small_rows(lambda i: "bin"), offsets=[i % 16 for i in range(51)])
    rc, arc, _ = csa.DeviceArchive.write_slices(sc.entries, **ws.SMALL_OPTS)
    assert rc == 0
    return sc, arc


def test_alignments_and_small_runs(csa, small):
    sc, arc = small
    dsts = _blanks(sc)
    with csa.DeviceArchive.open(arc) as a:
        rc, st = _read(csa, a, dsts)
    assert rc == 0 and st["verify_failures"] == 0
    for n, (t, _) in dsts.items():
        assert _bytes(t) == _hosts(sc)[n], n
    assert st["periodic_pieces"] > 0
    assert st["periodic_pieces"] + st["plain_pieces"] >= sum((len(c) + 16383) // 16384 for c in sc.content.values())
    assert st["hull_bytes"] == sum(_hull(e["slice"]) for e in sc.entries)
    assert st["selected_bytes"] == sum(len(c) for c in sc.content.values()) == st["raw_bytes"]


# ---- 3. reassembly --------------------------------------------------------------------------------------------------------

BOUNDS = [0, 1, 16, 33, 160, 400, 417, 999, 1000]                  # eight ranks; widths 1, 15, 17, 127, 240, 17, 582, 1


def test_column_blocks_are_reassembled_in_one_call(csa):
    import torch
    rows_n, width = 200, 1000
    m = np.frombuffer(cases.build([["text", 77, 0, rows_n * width]]), dtype=np.uint8).reshape(rows_n, width)
    dev = _upload(m.tobytes())
    row = {"edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    slices = {f"w{k}": csa.rows_slice(width, 0, rows_n, c0, c1) for k, (c0, c1) in enumerate(zip(BOUNDS, BOUNDS[1:]))}
    rc, arc, _ = csa.DeviceArchive.write_slices([dict(row, name=n, tensor=dev, slice=s) for n, s in slices.items()], level=1)
    assert rc == 0
    full = _blank(3 + rows_n * width + 5)
    body = full[3:3 + rows_n * width]
    with csa.DeviceArchive.open(arc) as a:
        rc, st = _read(csa, a, {n: (body, s) for n, s in slices.items()})
        assert rc == 0 and st["verify_failures"] == 0 and st["periodic_pieces"] > 0
        assert st["selected_bytes"] == rows_n * width and st["hull_bytes"] == sum(_hull(s) for s in slices.values())
        assert _bytes(full) == b"\xa5" * 3 + m.tobytes() + b"\xa5" * 5
        # the same through the comparison: eight interleaved slices of one matrix, all equal
        rc, diffs, _ = a.compare_slices({n: (body, s) for n, s in slices.items()})
        assert rc == 0 and all(d["status"] == 0 for d in diffs.values())
    # a block of float32 columns, given as a view
    m2d = torch.frombuffer(bytearray(m.tobytes()), dtype=torch.float32).reshape(rows_n, width // 4).cuda()
    rc, arc, _ = csa.DeviceArchive.write_slices([dict(row, name="v", tensor=csa.tensor_slice(m2d[:, 37:101])[0],
                                                      slice=csa.tensor_slice(m2d[:, 37:101])[1])], level=1)
    assert rc == 0
    back = _blank(rows_n * width).view(torch.float32).reshape(rows_n, width // 4)
    with csa.DeviceArchive.open(arc) as a:
        rc, st = _read(csa, a, {"v": back[:, 37:101]})
        assert rc == 0 and st["verify_failures"] == 0 and st["selected_bytes"] == rows_n * 256
        rc, diffs, _ = a.compare_slices({"v": m2d[:, 37:101]})
        assert rc == 0 and diffs["v"]["status"] == 0
    want = np.full((rows_n, width), 0xA5, dtype=np.uint8)
    want[:, 148:404] = m[:, 148:404]
    assert back.view(torch.uint8).cpu().numpy().tobytes() == want.tobytes()


# ---- 4. one read path -------------------------------------------------------------------------------------------------------

EDGE_SIZES = [0, 1, 15, 16, 17, 4095, 16383, 16384, 16385, 32769, 70001]


def test_extract_into_is_this_call_with_whole_buffer_slices(csa):
    import torch
    content = {f"e/f{n:05d}.b{i % 4}": cases.build([["text", 50 + i, 0, n]]) for i, n in enumerate(EDGE_SIZES)}
    row = {"edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    rc, arc, wst = csa.DeviceArchive.write_tensors([dict(row, name=n, tensor=_upload(c) if c else None) for n, c in content.items()],
                                                   task_bytes=40000, **ws.SMALL_OPTS)
    assert rc == 0 and wst["tasks"] >= 3 and max(f["nfrags"] for f in wst["files"]) >= 2      # several tasks, an entry cut across two

    def bufs():
        return {n: _blank(16 + len(c) + 5)[(0, 1, 3, 8, 15)[i % 5]:][:len(c)] for i, (n, c) in enumerate(content.items())}
    with csa.DeviceArchive.open(arc) as a:
        for kw in ({}, {"device_streams": 2}):
            one, two = bufs(), bufs()
            rc1, st1 = a.extract_into(one, **kw)
            rc2, st2 = _read(csa, a, {n: (t, (0, t.numel())) for n, t in two.items()}, **kw)
            assert rc1 == rc2 == 0
            for n, c in content.items():
                assert _bytes(one[n]) == _bytes(two[n]) == c, n
                base = two[n]._base if two[n]._base is not None else two[n]
                assert bool((base == 0xA5).sum() >= base.numel() - len(c)), n
            assert {k: st1[k] for k in SAME} == {k: st2[k] for k in SAME}
            assert st2["periodic_pieces"] == 0 and st2["plain_pieces"] >= sum((len(c) + 16383) // 16384 for c in content.values())
            assert st2["selected_bytes"] == st2["hull_bytes"] == sum(EDGE_SIZES)
            assert (st2["waves"] > 1) == bool(kw)


# ---- 5. oversized, short and verify-only destinations ---------------------------------------------------------------------

def test_oversized_short_and_verify_only_destinations(csa, small):
    sc, arc = small
    k = next(i for i, e in enumerate(sc.entries) if e["slice"][1] == 33 and e["slice"][3] > 3)
    name, (off, run, stride, count) = sc.entries[k]["name"], sc.entries[k]["slice"]
    host = sc.host[k]
    with csa.DeviceArchive.open(arc) as a:
        # three rows more than the entry has: they stay as they were
        big = _blank(len(host) + 3 * stride)
        rc, st = _read(csa, a, {name: (big, (off, run, stride, count + 3))}, names=[name])
        assert rc == 0 and st["selected_bytes"] == run * count and st["hull_bytes"] == (count + 2) * stride + run
        assert _bytes(big) == host + b"\xa5" * (3 * stride)
        # one row fewer: refused, nothing launched
        short = _blank(len(host))
        rc, st = a.extract_into_slices({name: (short, (off, run, stride, count - 1))}, names=[name])
        assert rc == csa.WRITE_ERROR and st["launches"] == 0 and st["selected_bytes"] == 0 and bool((short == 0xA5).all())
        # every second entry verified only
        dsts = _blanks(sc)
        some = {n: (d if i % 2 else None) for i, (n, d) in enumerate(dsts.items())}
        rc, st = _read(csa, a, some)
        rc_all, st_all = a.extract_into({})
        assert rc == rc_all == 0 and {k: st[k] for k in SAME} == {k: st_all[k] for k in SAME}
        for i, (n, (t, _)) in enumerate(dsts.items()):
            assert _bytes(t) == (_hosts(sc)[n] if i % 2 else b"\xa5" * t.numel()), n
        # a selection, stopped early
        pick = [sc.entries[i]["name"] for i in (3, 17)]
        full, early = {n: _blanks(sc)[n] for n in pick}, {n: _blanks(sc)[n] for n in pick}
        rc1, st1 = _read(csa, a, full, names=pick)
        rc2, st2 = _read(csa, a, early, names=pick, stop_early=True)
        assert rc1 == rc2 == 0 and st2["stopped_tasks"] > 0 and st2["decoded_bytes"] < st2["task_raw_bytes"]
        for n in pick:
            assert _bytes(full[n][0]) == _bytes(early[n][0]) == _hosts(sc)[n], n


# ---- 6. a damaged archive ---------------------------------------------------------------------------------------------------

def test_damage_is_reported_and_delivered_as_extract_into_does(csa):
    sc = Scattered(csa, ws._small_rows(lambda i: f"b{i % 6}"), offsets=[i % 16 for i in range(51)])
    rc, arc, wst = csa.DeviceArchive.write_slices(sc.entries, **ws.SMALL_OPTS)
    assert rc == 0 and wst["tasks"] >= 3
    good = _bytes(arc)
    index_pos = int.from_bytes(good[8:16], "little")
    flipped = bytearray(good)
    flipped[24 + (index_pos - 24) // 2] ^= 0x40                    # one byte inside a task stream
    cut = index_pos - (index_pos - 24) // 8                        # the last archive block cut short, the index put behind the cut
    short = good[:8] + cut.to_bytes(8, "little") + good[16:cut] + good[index_pos:]
    for what, bad in (("flipped", bytes(flipped)), ("cut", short)):
        with csa.DeviceArchive.open(_upload(bad)) as a:
            packed = {n: _blank(len(c)) for n, c in sc.content.items()}
            rc_p, st_p = a.extract_into(packed)
            assert rc_p == -1 or st_p["verify_failures"] > 0, what
            dsts = _blanks(sc)
            rc, st = _read(csa, a, dsts)
            assert (rc, st["verify_failures"]) == (rc_p, st_p["verify_failures"]), what
            assert [f["failed_frags"] for f in st["files"]] == [f["failed_frags"] for f in st_p["files"]], what
            undelivered = 0
            for e in sc.entries:
                got = _bytes(packed[e["name"]])
                undelivered += got != sc.content[e["name"]]
                off, run, stride, count = e["slice"]
                assert _bytes(dsts[e["name"]][0]) == scatter(got, run, stride, count, 0, off)[0], (what, e["name"])
            print(what, "rc", rc, "verify_failures", st["verify_failures"], "entries not delivered whole", undelivered)
            assert undelivered > 0, what


# ---- 7. compare -------------------------------------------------------------------------------------------------------------

def test_compare_against_slices(csa, small):
    import torch
    sc, arc = small
    srcs = {e["name"]: (e["tensor"], e["slice"]) for e in sc.entries}
    k = next(i for i, e in enumerate(sc.entries) if e["slice"][1] == 4097 and e["slice"][3] > 3 and e["slice"][2] > 4097)
    name, (off, run, stride, count) = sc.entries[k]["name"], sc.entries[k]["slice"]
    other = sc.entries[k - 1]["name"]
    with csa.DeviceArchive.open(arc) as a:
        rc, diffs, st = a.compare_slices(srcs)
        assert rc == 0 and st["verify_failures"] == 0 and st["launches"] == 3 * st["waves"] and st["periodic_pieces"] > 0
        assert all(d == {"status": 0, "first_diff": csa.NO_DIFF, "failed_frags": 0} for d in diffs.values())
        assert st["selected_bytes"] == sum(len(c) for c in sc.content.values()) and st["hull_bytes"] == sum(_hull(e["slice"]) for e in sc.entries)
        changed = sc.entries[k]["tensor"].clone()
        changed[off + 3 * stride + 2000] ^= 0x10                   # row 3, byte 2000
        rc, diffs, _ = a.compare_slices(dict(srcs, **{name: (changed, (off, run, stride, count))}))
        assert rc == 0 and diffs[name] == {"status": csa.CSA_DIFF_BYTES, "first_diff": 3 * run + 2000, "failed_frags": 0}
        assert all(d["status"] == 0 for n, d in diffs.items() if n != name)
        gap = sc.entries[k]["tensor"].clone()
        gap[off + 3 * stride + run] ^= 0x10                        # the first gap byte behind row 3
        gap[off - 1 if off else off + run] ^= 0x10                 # and the byte in front of the hull (or one more gap byte)
        gap[off + _hull((off, run, stride, count))] ^= 0x10        # and the first guard byte behind it
        rc, diffs, _ = a.compare_slices(dict(srcs, **{name: (gap, (off, run, stride, count))}))
        assert rc == 0 and all(d["status"] == 0 for d in diffs.values())
        # one row short, one row long: the rest is compared, and equal -- or not
        long = torch.cat([changed, _blank(stride)])
        for rows, tensor, want in ((count - 1, sc.entries[k]["tensor"], csa.CSA_DIFF_SIZE), (count + 1, long, csa.CSA_DIFF_SIZE | csa.CSA_DIFF_BYTES),
                                   (3, changed, csa.CSA_DIFF_SIZE), (4, changed, csa.CSA_DIFF_SIZE | csa.CSA_DIFF_BYTES)):
            rc, diffs, st = a.compare_slices({name: (tensor, (off, run, stride, rows))}, names=[name])
            assert rc == 0 and diffs[name]["status"] == want, rows
            assert diffs[name]["first_diff"] == (3 * run + 2000 if want & csa.CSA_DIFF_BYTES else csa.NO_DIFF), rows
            assert st["selected_bytes"] == min(rows, count) * run
        # an entry left out is verified only; hulls may alias each other
        rc, diffs, _ = a.compare_slices({name: srcs[name], other: srcs[name]}, names=[name, other, sc.entries[k + 1]["name"]])
        assert rc == 0 and diffs[name]["status"] == 0 and diffs[sc.entries[k + 1]["name"]]["status"] == csa.CSA_DIFF_SKIPPED
        assert diffs[other]["status"] & (csa.CSA_DIFF_SIZE | csa.CSA_DIFF_BYTES)
    assert sc.unchanged() and _bytes(changed[:len(sc.host[k])]) != sc.host[k]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------

def _raw(csa, a, compare, ptrs, sizes, slices, n=None, with_sizes=True, with_slices=True):
    """CSAMI_DeviceReadIntoSlices / CSAMI_DeviceCompareSlices as given, over statistics marked 0x5A -> (rc, the three statistics)"""
    import torch
    n = len(ptrs) if n is None else n
    pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    sa = (C.c_uint64 * max(len(ptrs), 1))(*sizes)
    sl = (csa.CSADevSlice * max(len(ptrs), 1))()
    for x, s in zip(sl, slices):
        x.offset, x.run, x.stride, x.count = s
    st, ss, sp, o = csa.CSADevReadStats(), csa.CSADevStopStats(), csa.CSADevSpreadStats(), csa.options()
    for t in (st, ss, sp):
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    files, diffs = (csa.CSADevFile * max(n, 1))(), (csa.CSADevDiff * max(n, 1))()
    head = (a._h, None, 0, pa, sa if with_sizes else None, sl if with_slices else None, n, 0, C.byref(o), files)
    torch.cuda.synchronize()
    if compare:
        rc = csa.lib().CSAMI_DeviceCompareSlices(*head, diffs, C.byref(st), C.byref(ss), C.byref(sp))
    else:
        rc = csa.lib().CSAMI_DeviceReadIntoSlices(*head, C.byref(st), C.byref(ss), C.byref(sp))
    return rc, (st, ss, sp)


def test_refusals_launch_nothing(csa):
    M64 = 1 << 64
    row = {"edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR}
    content = [cases.build([["text", 9 + i, 0, 6000]]) for i in range(2)]
    rc, arc, _ = csa.DeviceArchive.write_tensors([dict(row, name=f"r{i}.bin", tensor=_upload(c)) for i, c in enumerate(content)], level=1)
    assert rc == 0 and arc.numel() >= 6000
    s = (1, 1000, 1500, 6)                                         # hull 8500, the buffer 8506 bytes
    big = _blank(2 * 8506)
    p, n = big.data_ptr(), 8506
    two = ([p, p + n], [n, n], [s, s])
    with csa.DeviceArchive.open(arc) as a:
        def refused(what, want, ptrs, sizes, slices, both=True, **kw):
            for compare in ((False, True) if both else (False,)):
                rc, stats = _raw(csa, a, compare, ptrs, sizes, slices, **kw)
                assert rc == want, (what, compare)
                assert all(bytes(t) == bytes(C.sizeof(t)) for t in stats), (what, compare)
                assert bool((big == 0xA5).all()), (what, compare)

        refused("slices == NULL", -1, *two, with_slices=False)
        refused("sizes == NULL", -1, *two, with_sizes=False)
        refused("n is not the plan's", -1, [p], [n], [s])
        refused("n is not the plan's", -1, [p, p + n, p], [n, n, n], [s, s, s])
        refused("the last selected byte at sizes[i]", -1, [p, p + n], [n, 8500], [s, s])
        refused("run == 0 with count > 0", -1, [p, p + n], [n, n], [s, (1, 0, 5, 3)])
        refused("stride < run with count > 1", -1, [p, p + n], [n, n], [(1, 1000, 999, 6), s])
        refused("(count - 1) * stride wraps", -1, [p, p + n], [n, M64 - 1], [s, (1, 1, 1 << 62, 5)])
        refused("offset + hull wraps", -1, [p, p + n], [n, M64 - 1], [s, (M64 - 8, 1, 8, 2)])
        refused("a destination one row short", csa.WRITE_ERROR, [p, p + n], [n, n], [s, (1, 1000, 1500, 5)], both=False)
        refused("two destinations that share their bytes", -1, [p, p], [n, n], [s, s], both=False)
        refused("two column blocks that share one column", -1, [p, p], [2 * n, 2 * n], [(0, 1000, 1500, 6), (999, 1000, 1500, 6)], both=False)
        refused("a byte range one byte longer than the gap it lies in", -1, [p, p], [2 * n, 2 * n], [(0, 1000, 6500, 6), (1000, 6000, 6000, 1)][::-1],
                both=False)
        refused("the archive itself as a buffer", -1, [p, arc.data_ptr()], [n, arc.numel()], [s, (0, 6000, 6000, 1)])
        # what is accepted: the verify-only entry's slice is not looked at; interleaved destinations; aliased sources
        rc, (st, _, sp) = _raw(csa, a, False, [p, None], [n, 0], [s, (1, 0, 5, 3)])
        assert rc == 0 and st.launches == 3 and sp.selected_bytes == 6000 and sp.hull_bytes == 8500
        assert _bytes(big[:n]) == scatter(content[0], 1000, 1500, 6, 0, 1)[0] and bool((big[n:] == 0xA5).all())
        big.fill_(0xA5)
        rc, (st, _, sp) = _raw(csa, a, False, [p, p], [2 * n, 2 * n], [(0, 500, 1000, 12), (500, 500, 1000, 12)])
        assert rc == 0 and sp.periodic_pieces > 0
        inter = np.full(2 * n, 0xA5, dtype=np.uint8)
        inter[:12000].reshape(12, 2, 500)[:, 0, :] = np.frombuffer(content[0], dtype=np.uint8).reshape(12, 500)
        inter[:12000].reshape(12, 2, 500)[:, 1, :] = np.frombuffer(content[1], dtype=np.uint8).reshape(12, 500)
        assert _bytes(big) == inter.tobytes()
        rc, stats = _raw(csa, a, True, [p, p], [2 * n, 2 * n], [(0, 500, 1000, 12), (0, 500, 1000, 12)])
        assert rc == 0 and _bytes(big) == inter.tobytes(), "aliased hulls are fine where nothing is written"
    # an archive that lies inside a gap of a hull
    rc, one, _ = csa.DeviceArchive.write_tensors([dict(row, name="g.bin", tensor=_upload(content[0][:2000]))], level=1)
    assert rc == 0 and one.numel() < 60000
    wide = _blank(1 << 17)
    wide[2000:2000 + one.numel()].copy_(one)
    before = _bytes(wide)
    with csa.DeviceArchive.open(wide[2000:2000 + one.numel()]) as a:
        for compare in (False, True):
            rc, stats = _raw(csa, a, compare, [wide.data_ptr()], [wide.numel()], [(0, 1000, 70000, 2)])
            assert rc == -1 and all(bytes(t) == bytes(C.sizeof(t)) for t in stats) and _bytes(wide) == before
        rc, stats = _raw(csa, a, False, [wide.data_ptr() + 70000], [wide.numel() - 70000], [(0, 1000, 30000, 2)])
        assert rc == 0 and _bytes(wide[:70000]) == before[:70000], "a hull that clears the archive is fine"
        assert _bytes(wide[70000:71000]) + _bytes(wide[100000:101000]) == content[0][:2000]
