"""GPU tier for the device-resident archive read (include/csa_mi355x.h: CSAMI_DeviceOpen / Plan / Read / Close; csc_amd.csa.DeviceArchive):
a `.csa` uploaded to device memory must come out as the files' bytes in device memory -- gathered by k_gather_extents, decoded in
place by CSCMI_DecodeDeviceBatch, scattered and summed by k_frag_pieces, verified by k_frag_fold.  The expected bytes are the
trees' own content and what oracle/orc_csa.py extracts with the oracle decoder; archives are written once per module by `csa.add`
(and by the reference archiver where oracle/_ref travelled with the snapshot).
"""
import os
import subprocess
import sys

import pytest

import cases
import csa_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

CSARC_REF = os.path.join(ROOT, "oracle", "_ref", "csarc_ref")
HAVE_REF = os.path.exists(CSARC_REF)

EDGE_SIZES = [1, 15, 16, 17, 4095, 16383, 16384, 16385, 32769, 70001]
WHOLE = ["mixed_tree", "many_files", "single_shadowed_by_empty", "single_after_empty", "no_data", "frag_edges", "frag_edges_single"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def codec(orc, zalloc):
    def enc(data, dict_size, level):
        rc, s = orc.encode(data, props=orc.props_init(dict_size, level), alloc=zalloc)
        assert rc == 0
        return s

    def dec(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw
    return enc, dec


def _write_tree(root, files):
    content = {}
    for rel, parts in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        content[rel] = cases.build(parts) if parts else b""
        with open(path, "wb") as f:
            f.write(content[rel])
        os.utime(path, (csa_cases.MTIME, csa_cases.MTIME))
    return content


@pytest.fixture(scope="module")
def arcs(csa, tmp_path_factory):
    """{name: (path of the archive, its bytes, {relpath: content})}, written once"""
    out = {}
    cwd = os.getcwd()
    try:
        for case in WHOLE[:5]:
            d = tmp_path_factory.mktemp(case)
            content = csa_cases.make_tree(str(d), case)
            os.chdir(d)
            spec = csa_cases.CSA_CASES[case]
            assert csa.add(csa_cases.ARCNAME, spec["args"], overwrite=True, **spec["opts"])[0] == 0
            out[case] = (str(d / csa_cases.ARCNAME), (d / csa_cases.ARCNAME).read_bytes(), content)
        d = tmp_path_factory.mktemp("frag_edges")
        content = _write_tree(str(d), {f"e/f{n:05d}.bin": [["text", 50 + i, 0, n]] for i, n in enumerate(EDGE_SIZES)})
        os.chdir(d)
        assert csa.add("out.csa", ["e"], overwrite=True, recurse=True, level=1, dict_size=64 << 10, task_bytes=20000)[0] == 0
        out["frag_edges"] = (str(d / "out.csa"), (d / "out.csa").read_bytes(), content)
        d = tmp_path_factory.mktemp("frag_edges_single")
        content = _write_tree(str(d), {"one/only.dat": [["exe", 61, 0, 100003]]})
        os.chdir(d)
        assert csa.add("out.csa", ["one/only.dat"], overwrite=True, level=2, dict_size=64 << 10, split_count=7)[0] == 0
        out["frag_edges_single"] = (str(d / "out.csa"), (d / "out.csa").read_bytes(), content)
    finally:
        os.chdir(cwd)
    return out


def _upload(data, off=0, pad=0):
    """the bytes in device memory, `off` bytes into their allocation (torch allocations are 512-byte aligned)"""
    import torch
    buf = torch.empty(off + len(data) + pad, dtype=torch.uint8, device="cuda")
    t = buf[off:off + len(data)]
    t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    assert t.data_ptr() % 16 == off % 16
    return t


def _open(csa, data, off=0):
    return csa.DeviceArchive.open(_upload(data, off))


def _bytes(view):
    return view.cpu().numpy().tobytes()


def _stored(info, name):
    return sum(f["size"] for f in info["index"][name]["frags"])


def _check_stats(st, index_rsize):
    assert st["launches"] == 3 * st["waves"]
    assert 24 + 10 + index_rsize <= st["readback_bytes"] <= 24 + 10 + index_rsize + 16 * st["tasks"] + 8 * st["frags"]


# ---- 1. whole archives --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", WHOLE)
def test_whole_archive(csa, arcs, codec, case):
    path, arc, content = arcs[case]
    info = orc_csa.parse(arc, codec[1])
    with _open(csa, arc) as a:
        files, total = a.plan()
        rc, views, st = a.extract()
        assert rc == 0 and st["verify_failures"] == 0 and st["files"] == files
        listed = csa.list_entries(path)
        assert [(f["name"], f["esize"], f["edate"], f["eattr"], f["nfrags"]) for f in files] == \
               [(e["name"], e["esize"], e["edate"], e["eattr"], len(e["frags"])) for e in listed]
        off = 0
        for f, e in zip(files, listed):
            assert f["offset"] == off and f["size"] == max([x["posfile"] + x["size"] for x in e["frags"]], default=0) and f["failed_frags"] == 0
            off += (f["size"] + 15) // 16 * 16
        assert off == total
        for rel, data in content.items():
            if rel in info["index"]:
                assert _bytes(views[rel]) == (data if _stored(info, rel) == len(data) else b""), rel
        if case in ("mixed_tree", "frag_edges", "frag_edges_single"):
            want, bad = orc_csa.extract(arc, codec[1])
            assert not bad and all(_bytes(views[n]) == d for n, d in want.items() if _stored(info, n) == len(d))
        _check_stats(st, info["index_rsize"])
        assert st["tasks"] == len(info["abindex"]) and st["raw_bytes"] == sum(_stored(info, n) for n in info["index"])
        assert st["frags"] == sum(1 for e in info["index"].values() for x in e["frags"] if x["size"])
        rc, st = a.test()
        assert rc == 0 and st["verify_failures"] == 0 and all(f["failed_frags"] == 0 for f in st["files"])
        _check_stats(st, info["index_rsize"])
    if case == "frag_edges":
        assert max(len(e["frags"]) for e in info["index"].values()) >= 2 and len(info["abindex"]) >= 5       # files cut across tasks
    if case == "no_data":
        assert st["waves"] == 0 and st["launches"] == 0 and total == 0


# ---- 2. a task of more than one decode launch ----------------------------------------------------------------------------

def test_task_above_four_mib(csa, tmp_path, monkeypatch):
    content = _write_tree(str(tmp_path), {"big.txt": [["text", 77, 0, 5 << 20]]})
    monkeypatch.chdir(tmp_path)
    assert csa.add("big.csa", ["big.txt"], overwrite=True, level=1, dict_size=1 << 20)[0] == 0
    with _open(csa, (tmp_path / "big.csa").read_bytes()) as a:
        rc, views, st = a.extract()
    assert rc == 0 and st["verify_failures"] == 0 and st["tasks"] == 1 and st["decode_launches"] > 1
    assert _bytes(views["big.txt"]) == content["big.txt"]


# ---- 3. selection: nothing outside the covered ranges is written ---------------------------------------------------------

@pytest.mark.parametrize("names", [["*.txt"], ["d/sub"], ["d/empty"]])
def test_selection_leaves_the_rest_of_dst_alone(csa, arcs, names):
    import torch
    _, arc, content = arcs["mixed_tree"]
    with _open(csa, arc) as a:
        files, total = a.plan(names)
        assert [f["name"] for f in files] == [n for n in ["d/", "d/a.txt", "d/b.txt", "d/empty", "d/noext", "d/sub/", "d/sub/c.exe", "d/sub/e.dat"]
                                              if orc_csa.isselected(names, n)]
        buf = torch.full((64 + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, views, st = a.extract(names, dst=buf[64:64 + total])
    assert rc == 0 and st["verify_failures"] == 0
    got = buf.cpu().numpy()
    want = bytearray(b"\xa5" * len(got))
    for f in files:
        data = content.get(f["name"], b"")
        assert f["size"] == len(data)
        want[64 + f["offset"]:64 + f["offset"] + f["size"]] = data
        assert _bytes(views[f["name"]]) == data
    assert got.tobytes() == bytes(want)
    assert st["tasks"] == {"*.txt": 1, "d/sub": 2, "d/empty": 0}[names[0]]


# ---- 4. alignment ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arc_off,dst_off", [(1, 1), (7, 9), (15, 15)])
def test_any_alignment_of_archive_and_destination(csa, arcs, arc_off, dst_off):
    import torch
    _, arc, content = arcs["mixed_tree"]
    with _open(csa, arc, arc_off) as a:
        total = a.plan()[1]
        buf = torch.full((dst_off + total + 33,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, views, st = a.extract(dst=buf[dst_off:dst_off + total])
        assert buf.data_ptr() % 16 == 0
    assert rc == 0 and st["verify_failures"] == 0
    for rel, data in content.items():
        assert _bytes(views[rel]) == data, rel
    got = buf.cpu().numpy().tobytes()
    assert got[:dst_off] == b"\xa5" * dst_off and got[dst_off + total:] == b"\xa5" * 33


# ---- 5. interleaved extents ---------------------------------------------------------------------------------------------

def _reindex(arc, info, codec, body=None, index=None, abindex=None):
    """the archive with another body and / or index: header + body + the index re-encoded with the oracle encoder (csarc.cpp:251)"""
    body = arc[24:info["index_pos"]] if body is None else body
    raw = orc_csa.pack_index(info["index"] if index is None else index, info["abindex"] if abindex is None else abindex, csa_cases.ARCNAME)
    istream = codec[0](raw, 256 * 1024, 2)
    head = b"CSA" + orc_csa.MAGIC_NUM.to_bytes(4, "little") + b"1" + (24 + len(body)).to_bytes(8, "little") \
        + len(istream).to_bytes(4, "little") + len(raw).to_bytes(4, "little")
    return head + bytes(body) + istream


def _rechop(arc, info, codec):
    """every task's stream cut into extents of 1, 2, 9, 10, 11 and 4097 bytes (each task starts the list elsewhere) and a rest, and the
    extents of the tasks dealt out in turn"""
    cuts = [1, 2, 9, 10, 11, 4097]
    parts = {}
    for k, bid in enumerate(sorted(info["abindex"])):
        s = b"".join(arc[o:o + n] for o, n in info["abindex"][bid])
        sizes = cuts[2 * k % 6:] + cuts[:2 * k % 6]
        assert len(s) > sum(sizes)
        parts[bid], pos = [], 0
        for n in sizes + [len(s) - sum(sizes)]:
            parts[bid].append(s[pos:pos + n])
            pos += n
    body, ab = bytearray(), {bid: [] for bid in parts}
    for i in range(7):
        for bid in sorted(parts):
            ab[bid].append((24 + len(body), len(parts[bid][i])))
            body += parts[bid][i]
    return _reindex(arc, info, codec, body=body, abindex=ab), ab


def test_interleaved_extents(csa, arcs, codec):
    _, arc, content = arcs["mixed_tree"]
    info = orc_csa.parse(arc, codec[1])
    chopped, ab = _rechop(arc, info, codec)
    assert len(ab) == 3 and sorted(n for _, n in ab[min(ab)][:6]) == [1, 2, 9, 10, 11, 4097]
    assert any(v[0][1] < 10 for v in ab.values()), "one task's first extent is shorter than the property bytes"
    assert ab[0][1][0] > ab[1][0][0] > ab[0][0][0], "the tasks interleave"
    want, bad = orc_csa.extract(chopped, codec[1])
    assert not bad and all(want[n] == d for n, d in content.items())
    with _open(csa, chopped, 3) as a:
        rc, views, st = a.extract()
        assert rc == 0 and st["verify_failures"] == 0 and st["tasks"] == 3 and st["waves"] == 1 and st["launches"] == 3
        for rel, data in content.items():
            assert _bytes(views[rel]) == data, rel
        rc, st = a.test(["d/sub/c.exe"])
        assert rc == 0 and st["verify_failures"] == 0 and st["tasks"] == 1


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/csarc_ref not in this snapshot")
def test_archive_written_by_four_reference_workers(csa, tmp_path):
    content = csa_cases.make_tree(str(tmp_path), "many_files")
    argv = list(csa_cases.csarc_argv("many_files"))
    argv.insert(1, "-t4")                          # four workers: blocks of different tasks interleave in the file
    subprocess.run([CSARC_REF] + argv, cwd=tmp_path, check=True, capture_output=True)
    with _open(csa, (tmp_path / csa_cases.ARCNAME).read_bytes()) as a:
        rc, views, st = a.extract()
    assert rc == 0 and st["verify_failures"] == 0 and st["launches"] == 3 * st["waves"]
    for rel, data in content.items():
        assert _bytes(views[rel]) == data, rel


# ---- 6. several waves -------------------------------------------------------------------------------------------------

def test_several_waves(csa, arcs):
    _, arc, content = arcs["many_files"]
    with _open(csa, arc) as a:
        rc, views, st = a.extract(hbm_budget=64 << 20)        # a task is reckoned at 25 MiB and more: two to a wave
        rc1, _, st1 = a.extract(device_streams=1)
    assert rc == 0 and st["verify_failures"] == 0 and st["waves"] >= 3 and st["launches"] == 3 * st["waves"]
    assert rc1 == 0 and st1["waves"] == st1["tasks"] == st["tasks"]
    for rel, data in content.items():
        assert _bytes(views[rel]) == data, rel


# ---- 7. damaged archives ------------------------------------------------------------------------------------------------

def _both(csa, data, tmp_path, name):
    """(rc, verify_failures) of csa.test on the bytes written to a file, and of DeviceArchive.test on the bytes uploaded"""
    p = tmp_path / name
    p.write_bytes(data)
    rc_f, st_f = csa.test(str(p))
    try:
        with _open(csa, data) as a:
            rc_d, st_d = a.test()
            got = (rc_d, st_d["verify_failures"])
    except ValueError as e:
        got = (e.rc, 0)
    print(f"{name}: file path {(rc_f, st_f['verify_failures'])}, device path {got}")
    return (rc_f, st_f["verify_failures"]), got


def test_damaged_header_and_index(csa, arcs):
    _, arc, _ = arcs["mixed_tree"]
    bad = bytearray(arc); bad[1] = ord("X")
    with pytest.raises(ValueError) as e:
        _open(csa, bytes(bad))
    assert e.value.rc == 1
    with pytest.raises(ValueError) as e:
        _open(csa, arc[:20])
    assert e.value.rc == 1
    bad = bytearray(arc); bad[8:16] = (len(arc) + 1).to_bytes(8, "little")
    with pytest.raises(ValueError) as e:
        _open(csa, bytes(bad))
    assert e.value.rc == -1
    index_pos = int.from_bytes(arc[8:16], "little")
    bad = bytearray(arc); bad[index_pos + 40] ^= 0x10
    try:
        _open(csa, bytes(bad)).close()                                       # a clean open ...
    except ValueError as e:
        assert e.rc == -1                                                    # ... or -1


def test_damaged_bodies_answer_as_the_file_path_does(csa, arcs, codec, tmp_path):
    _, arc, _ = arcs["mixed_tree"]
    info = orc_csa.parse(arc, codec[1])
    # an extent beyond the archive: the second half of the largest task's stream is said to lie far behind the end
    bid = max(info["abindex"], key=lambda b: sum(n for _, n in info["abindex"][b]))
    (o, n), rest = info["abindex"][bid][0], info["abindex"][bid][1:]
    ab = dict(info["abindex"]); ab[bid] = [(o, n // 2), (1 << 40, n - n // 2)] + rest
    want, got = _both(csa, _reindex(arc, info, codec, abindex=ab), tmp_path, "extent.csa")
    assert got == want and got[0] == -1
    # a flipped byte in the middle of that stream
    bad = bytearray(arc); bad[o + n // 2] ^= 0x40
    want, got = _both(csa, bytes(bad), tmp_path, "flip.csa")
    assert got == want and (got[0] == -1 or got[1] > 0)
    # the body cut in half: the index position lies behind the end
    want, got = _both(csa, arc[:len(arc) // 2], tmp_path, "half.csa")
    assert got == want == (-1, 0)


def test_wrong_checksum_in_the_index_is_counted_not_fatal(csa, arcs, codec):
    _, arc, content = arcs["mixed_tree"]
    info = orc_csa.parse(arc, codec[1])
    index = {n: dict(e, frags=[dict(f) for f in e["frags"]]) for n, e in info["index"].items()}
    index["d/b.txt"]["frags"][0]["checksum"] ^= 1
    with _open(csa, _reindex(arc, info, codec, index=index)) as a:
        rc, views, st = a.extract()
        assert rc == 0 and st["verify_failures"] == 1                        # csa_io.h:331-332
        assert {f["name"]: f["failed_frags"] for f in st["files"] if f["failed_frags"]} == {"d/b.txt": 1}
        assert all(_bytes(views[n]) == d for n, d in content.items())        # the bytes are delivered all the same
        rc, st = a.test(["d/a.txt"])
        assert rc == 0 and st["verify_failures"] == 0


# ---- 8. a destination one byte short -------------------------------------------------------------------------------------

def test_dst_cap_one_byte_short(csa, arcs):
    import torch
    _, arc, _ = arcs["mixed_tree"]
    with _open(csa, arc) as a:
        total = a.plan()[1]
        buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, views, st = a.extract(dst=buf[:total - 1])
    assert rc == csa.WRITE_ERROR and views == {}
    assert (st["launches"], st["decode_launches"], st["waves"], st["tasks"], st["readback_bytes"]) == (0, 0, 0, 0, 0)
    assert bool((buf == 0xA5).all())
