"""One small scenario over every entry point of the device archive (csc_amd.csa.DeviceArchive), and what each call reports:
rc, the files table, the diffs, the tasks, every integer statistic and the adler32 of what it produced.  Shared by
tools/make_golden_archive_stats.py, which records it into tests/golden/archive_stats.json, and tests/test_gpu_archive_stats.py,
which holds the library to that record: the launch, piece and byte counters of the archive layer are pinned, not bounded.

The entries are mixed_tree's (tests/csa_cases.py: two directories, an empty file) and d/sub/q.bin of 40 000 bytes -- three 16 KiB
pieces, the last short.  Each lies under a slice of a buffer of its own (SHAPES); the archive is read as written, where a stream of
one extent is decoded in place, and cut into extents of 1, 2, 9, 10, 11 and 4097 bytes (_rechop), where the property bytes cross
extents and the streams are gathered.  Every call runs with device_streams=2: more than one wave, more than one check wave."""
import os
import sys

import cases
import csa_cases
import csa_write_cases
from test_gpu_archive_device import _rechop
from test_gpu_archive_write_slices import Scattered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "archive_stats.json")
OPTS = dict(level=1, dict_size=64 << 10, device_streams=2)
EXTRA = "d/sub/q.bin"
# name -> (run, stride): rows of 24 bytes 40 apart (periodic, sub-block copies), rows of 5 bytes 7 apart (the byte path), one run
# above 16 KiB (every piece whole), rows of 20 000 bytes (whole pieces and pieces across a border); d/empty is the slice of count 0
SHAPES = {"d/a.txt": (24, 40), "d/b.txt": (5, 7), "d/sub/c.exe": (200000, 200000), "d/sub/e.dat": (150000, 150000), "d/noext": (5000, 5000),
          EXTRA: (20000, 20013)}
# what extract_slices reads of the entries: the same four kinds of slice; an entry without one is not read
READ_SLICES = {"d/a.txt": (100, 24, 40, 5000), "d/b.txt": (3, 5, 7, 9000), "d/sub/c.exe": (1000, 40000), "d/sub/e.dat": (0, 0, 0, 0),
               EXTRA: (0, 40000)}
FLIP = ("d/sub/c.exe", 123457)                  # the byte that the "changed" calls change
TIME_KEYS = ("kernel_ms", "check_kernel_ms")    # and seconds_*: the fields that are left out


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _stats(st):
    """every field of a stats dict but the times; a field that is neither an integer, a list nor a time fails the record"""
    out = {}
    for k, v in st.items():
        if k.startswith("seconds_") or k in TIME_KEYS:
            assert isinstance(v, float), k
            continue
        assert isinstance(v, (int, list)) and not isinstance(v, bool), (k, v)
        out[k] = v
    return out


def record(csa, codec, times=None):
    """-> {call: {"rc", "stats" (files and tasks among them), "diffs" / "adler32" where the call has them}}; times: a dict that gets
    every call's (seconds_total, kernel_ms)"""
    import torch
    edate = int(csa.lib().CSA_DecimalTime(csa_cases.MTIME))
    table, _, content = csa_write_cases.table("mixed_tree", edate)
    table.append({"name": EXTRA, "esize": 40000, "edate": edate, "eattr": csa_write_cases.FILE_ATTR, "offset": 0})
    content[EXTRA] = cases.build([["random", 6, 0, 40000]])
    rows = []
    for f in table:
        data = content.get(f["name"])
        if f["eattr"] == csa_write_cases.DIR_ATTR:
            rows.append((f["name"], None, 0, 0, 0))
        elif not data:
            rows.append((f["name"], b"", 0, 0, 0))
        else:
            run, stride = SHAPES[f["name"]]
            assert len(data) % run == 0
            rows.append((f["name"], data, run, stride, len(data) // run))
    sc = Scattered(csa, rows)
    packed = {e["name"]: e["tensor"] for e in sc.packed}
    sliced = {e["name"]: (e["tensor"], e["slice"]) for e in sc.entries if e["tensor"] is not None}
    out = {}

    def put(key, rc, st, arc=None, diffs=None):
        out[key] = {"rc": rc, "stats": _stats(st)}
        if times is not None:
            times[key] = (st["seconds_total"], st["kernel_ms"])
        if diffs is not None:
            out[key]["diffs"] = diffs
        if arc is not None:
            out[key]["adler32"] = csa.adler32(_bytes(arc))

    # ---- the three writes
    src, files, pos = bytearray(), [], 0
    for f in table:
        data = content.get(f["name"], b"")
        files.append(dict(f, offset=pos))
        src += data + bytes(-len(data) % 16 + 3)
        pos = len(src)
    src_dev = torch.frombuffer(src, dtype=torch.uint8).cuda()
    rc, arc, st = csa.DeviceArchive.write(files, src_dev, arcname=csa_cases.ARCNAME, **OPTS)
    put("write", rc, st, arc)
    rc, base, st = csa.DeviceArchive.write_tensors(sc.packed, arcname=csa_cases.ARCNAME, **OPTS)
    put("write_tensors", rc, st, base)
    rc, arc, st = csa.DeviceArchive.write_slices(sc.entries, arcname=csa_cases.ARCNAME, **OPTS)
    put("write_slices", rc, st, arc)
    assert rc == 0 and _bytes(arc) == _bytes(base) and sc.unchanged()

    # ---- one byte changed: in the packed tensor, and under the slice
    name, at = FLIP
    k = next(i for i, e in enumerate(sc.entries) if e["name"] == name)
    off, run, stride, _ = sc.entries[k]["slice"]
    flipped_p, flipped_s = sc.packed[k]["tensor"].clone(), sc.entries[k]["tensor"].clone()
    flipped_p[at] ^= 0x10
    flipped_s[off + at // run * stride + at % run] ^= 0x10
    changed = [dict(e, tensor=flipped_s) if i == k else e for i, e in enumerate(sc.entries)]
    changed_p = [dict(e, tensor=flipped_p) if i == k else e for i, e in enumerate(sc.packed)]

    plain = _bytes(base)
    chopped, ab = _rechop(plain, orc_csa.parse(plain, codec[1]), codec)
    assert all(len(v) == 7 for v in ab.values()) and len(ab) >= 3
    for how, data in (("plain", plain), ("chopped", chopped)):
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        with csa.DeviceArchive.open(dev) as a:
            rc, views, st = a.extract(**OPTS)
            put(f"{how}/extract", rc, st, torch.cat([views[f["name"]] for f in st["files"]]))
            put(f"{how}/test", *a.test(**OPTS))
            rc, views, st = a.extract(stop_early=True, **OPTS)
            put(f"{how}/extract_stop", rc, st, torch.cat([views[f["name"]] for f in st["files"]]))
            dsts = {n: torch.zeros_like(t) for n, t in packed.items() if t is not None}
            rc, st = a.extract_into(dsts, **OPTS)
            put(f"{how}/extract_into", rc, st, torch.cat([dsts[n] for n in sorted(dsts)]))
            rc, got, st = a.extract_slices(READ_SLICES, **OPTS)
            put(f"{how}/extract_slices", rc, st, torch.cat([got[n] for n in sorted(got)]))
            dsts = {n: (torch.full_like(t, 0xA5), s) for n, (t, s) in sliced.items()}
            rc, st = a.extract_into_slices(dsts, **OPTS)
            put(f"{how}/extract_into_slices", rc, st, torch.cat([dsts[n][0] for n in sorted(dsts)]))
            assert all(_bytes(dsts[n][0]) == _bytes(sliced[n][0]) for n in dsts)
            for what, p, s in (("equal", packed[name], sliced[name]), ("changed", flipped_p, (flipped_s, sliced[name][1]))):
                rc, diffs, st = a.compare({**packed, name: p}, **OPTS)
                put(f"{how}/compare/{what}", rc, st, diffs=diffs)
                rc, diffs, st = a.compare_slices({**sliced, name: s}, **OPTS)
                put(f"{how}/compare_slices/{what}", rc, st, diffs=diffs)
            # the update under slices over the archive as written, over whole tensors over the cut one: check waves with and without rows
            same, other = (sc.entries, changed) if how == "plain" else (sc.packed, changed_p)
            for trust in (False, True):
                for what, entries in (("same", same), ("changed", other)):
                    rc, arc, st = a.update(entries, arcname=csa_cases.ARCNAME, trust_sums=trust, **OPTS)
                    put(f"{how}/update/{'trust' if trust else 'verify'}/{what}", rc, st, arc)
    assert sc.unchanged()
    return out
