"""GPU tier for the device-resident archive write (include/csa_mi355x.h: CSAMI_DeviceWrite; csc_amd.csa.DeviceArchive.write): file
bytes uploaded to device memory must come out as the `.csa` that `csarc a -t1` writes for the same entries -- fragments gathered
and summed by k_frag_pieces / k_frag_fold, encoded by CSCMI_EncodeDeviceBatch, block tables by k_block_table, streams placed by
k_gather_extents.  The expected bytes are the reference archiver's (tests/golden/csa.json) and what CSA_Add writes from a tree on
disk.  Every write of this file also has to keep the bus contract (_check_bus)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import cases
import csa_cases
import csa_write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

CSARC_REF = os.path.join(ROOT, "oracle", "_ref", "csarc_ref")
HAVE_REF = os.path.exists(CSARC_REF)
EDGE_SIZES = [1, 15, 16, 17, 4095, 16383, 16384, 16385, 32769, 70001]
GOLDEN_CASES = ["mixed_tree", "many_files", "single_split3", "single_split_many", "named_files_m3", "single_shadowed_by_empty",
                "single_after_empty", "no_data"]         # (not chunk_edges_m5: one 4 MiB level-5 stream, about 7 s)
MiB = 1 << 20


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


def _upload(data, off=0):
    import torch
    buf = torch.empty(off + len(data) + 1, dtype=torch.uint8, device="cuda")
    t = buf[off:off + len(data)]
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _bytes(view):
    return view.cpu().numpy().tobytes()


def _check_bus(st):
    """What crosses the bus (include/csa_mi355x.h).  The encoder reads back 16 bytes a stream a round; its rounds are bounded from
    the call's own stats: encode_launches counts, per CSCMI_EncodeDeviceBatch call, one flush kernel per stream, one framing launch
    per round and at least one encode launch per round but the last -- so encode_launches minus the streams (tasks, the index,
    the retries) is at least the rounds of all calls together."""
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


def _write(csa, files, src, **kw):
    rc, arc, st = csa.DeviceArchive.write(files, src, **kw)
    if rc == 0:
        _check_bus(st)
        assert st["archive_bytes"] == arc.numel()
        assert [(f["size"], f["name"]) for f in st["files"]] == [(f["esize"], f["name"]) for f in files]
    return rc, arc, st


def _edate(csa, t=csa_cases.MTIME):
    return int(csa.lib().CSA_DecimalTime(int(t)))


# ---- 1. goldens of the reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_archive_is_the_reference_archivers(csa, golden, case):
    files, src, _ = csa_write_cases.table(case, _edate(csa))
    opts = {k: v for k, v in csa_cases.CSA_CASES[case]["opts"].items() if k != "recurse"}
    rc, arc, st = _write(csa, files, _upload(src), arcname=csa_cases.ARCNAME, **opts)
    assert rc == 0
    g = golden[case]
    assert (st["archive_bytes"], st["index_raw_size"], st["index_compressed_size"]) == (g["archive_size"], g["index_rsize"], g["index_csize"])
    assert hashlib.sha256(_bytes(arc)).hexdigest() == g["archive_sha256"]
    assert st["n_entries"] == len(files) and st["raw_bytes"] == sum(f["esize"] for f in st["files"] if f["nfrags"])
    if case == "no_data":
        assert st["waves"] == 0 and st["tasks"] == 0 and st["launches"] == 1
    if case == "single_split3":
        assert st["tasks"] == 3 and [f["nfrags"] for f in st["files"]] == [3]


# ---- 2., 3. the same bytes as the file path -------------------------------------------------------------------------------

def _tree(root, spec):
    content = {}
    for rel, parts in spec.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        content[rel] = cases.build(parts) if parts else b""
        with open(path, "wb") as f:
            f.write(content[rel])
        os.utime(path, (csa_cases.MTIME + 60, csa_cases.MTIME + 60))
    return content


def _table_of_tree(csa, root, names, residue=0):
    """the entries CSA_Add finds for `names` (files, or directories taken with recurse), attributes from os.stat"""
    files, src = [], bytearray()

    def entry(rel):
        sb = os.lstat(os.path.join(root, rel))
        isdir = os.path.isdir(os.path.join(root, rel))
        data = b"" if isdir else open(os.path.join(root, rel), "rb").read()
        off = (len(src) + 15) // 16 * 16 + residue
        src.extend(bytes(off - len(src)) + data)
        files.append({"name": rel + "/" if isdir else rel, "esize": len(data), "edate": _edate(csa, sb.st_mtime),
                      "eattr": ord("u") + (sb.st_mode << 8), "offset": off})
        if isdir:
            for n in sorted(os.listdir(os.path.join(root, rel))):
                entry(rel + "/" + n)
    for n in names:
        entry(n)
    return files, bytes(src)


TREES = {
    "frag_edges": ({f"e/f{n:05d}.bin": [["text", 50 + i, 0, n]] for i, n in enumerate(EDGE_SIZES)}, ["e"],
                   dict(level=1, dict_size=64 << 10, task_bytes=20000)),
    "frag_edges_single": ({"one/only.dat": [["exe", 61, 0, 100003]]}, ["one/only.dat"], dict(level=2, dict_size=64 << 10, split_count=7)),
    "incompressible": ({"r/noise.bin": [["random", 81, 0, 5 * MiB // 2]]}, ["r"], dict(level=1, dict_size=1 << 20)),
    "across_a_chunk": ({"t/a.txt": [["text", 82, 0, 2 * MiB + 1]], "t/b.txt": [["text", 83, 0, 2 * MiB]]}, ["t"], dict(level=1, dict_size=1 << 20)),
}


@pytest.fixture(scope="module")
def trees(csa, tmp_path_factory):
    """{name: (table, source bytes, the archive CSA_Add wrote, options, content)}, each built when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            spec, args, opts = TREES[name]
            d = tmp_path_factory.mktemp(name)
            content = _tree(str(d), spec)
            cwd = os.getcwd()
            os.chdir(d)
            try:
                assert csa.add("out.csa", args, overwrite=True, recurse=True, **opts)[0] == 0
            finally:
                os.chdir(cwd)
            files, src = _table_of_tree(csa, str(d), args)
            made[name] = (files, src, (d / "out.csa").read_bytes(), opts, content, str(d))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(TREES))
def test_archive_is_what_the_file_path_writes(csa, trees, dec, name):
    files, src, want, opts, _, _ = trees(name)
    rc, arc, st = _write(csa, files, _upload(src), **opts)
    assert rc == 0 and _bytes(arc) == want
    info = orc_csa.parse(want, dec)
    assert st["blocks"] == sum(len(v) for v in info["abindex"].values()) and st["tasks"] == len(info["abindex"])
    if name == "frag_edges":
        assert max(f["nfrags"] for f in st["files"]) >= 2 and st["tasks"] >= 5                # files cut across tasks
    if name == "frag_edges_single":
        assert [f["nfrags"] for f in st["files"]] == [len(info["abindex"])]                  # every task encoded where it lies
    if name == "incompressible":
        assert len(info["abindex"]) == 1 and len(info["abindex"][0]) >= 3                    # a block table beyond one block
    if name == "across_a_chunk":
        assert st["tasks"] == 1 and st["frags"] == 2


# ---- 4. alignment ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_res,arc_res", [(1, 1), (7, 9), (15, 15)])
def test_any_alignment_of_source_and_archive(csa, golden, src_res, arc_res):
    import torch
    files, src, _ = csa_write_cases.table("mixed_tree", _edate(csa), residue=src_res)
    assert all(f["offset"] % 16 == src_res for f in files if f["esize"])
    opts = {k: v for k, v in csa_cases.CSA_CASES["mixed_tree"]["opts"].items() if k != "recurse"}
    g = golden["mixed_tree"]
    buf = torch.full((64 + arc_res + g["archive_size"] + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rc, arc, st = _write(csa, files, _upload(src), arc=buf[64 + arc_res:], **opts)
    assert rc == 0 and st["archive_bytes"] == g["archive_size"]
    got = _bytes(buf)
    assert hashlib.sha256(got[64 + arc_res:64 + arc_res + g["archive_size"]]).hexdigest() == g["archive_sha256"]
    assert got[:64 + arc_res] == b"\xa5" * (64 + arc_res), "the bytes in front of arc"
    assert got[64 + arc_res + g["archive_size"]:] == b"\xa5" * 4096, "the bytes of arc at and behind archive_bytes"


# ---- 5. waves -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", [{"device_streams": 2}, {"hbm_budget": 1 << 20}])
def test_several_waves_give_the_same_archive(csa, golden, how):
    files, src, _ = csa_write_cases.table("many_files", _edate(csa))
    opts = {k: v for k, v in csa_cases.CSA_CASES["many_files"]["opts"].items() if k != "recurse"}
    rc, arc, st = _write(csa, files, _upload(src), **opts, **how)
    assert rc == 0 and hashlib.sha256(_bytes(arc)).hexdigest() == golden["many_files"]["archive_sha256"]
    assert st["waves"] > 1 and st["launches"] <= 5 * st["waves"] + 2
    assert st["waves"] == ((st["tasks"] + 1) // 2 if "device_streams" in how else st["tasks"])


# ---- 6. capacity -----------------------------------------------------------------------------------------------------------

def test_capacity_is_exact(csa, golden):
    import torch
    files, src, _ = csa_write_cases.table("mixed_tree", _edate(csa))
    opts = {k: v for k, v in csa_cases.CSA_CASES["mixed_tree"]["opts"].items() if k != "recurse"}
    n = golden["mixed_tree"]["archive_size"]
    dev = _upload(src)
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, arc, st = _write(csa, files, dev, arc=buf[:n], **opts)
    assert rc == 0 and hashlib.sha256(_bytes(arc)).hexdigest() == golden["mixed_tree"]["archive_sha256"]
    assert _bytes(buf[n:]) == b"\xa5" * 64
    buf.fill_(0xA5)
    rc, arc, st = _write(csa, files, dev, arc=buf[:n - 1], **opts)
    assert rc == csa.WRITE_ERROR and arc is None
    assert _bytes(buf[n - 1:]) == b"\xa5" * 65, "the bytes behind arc_cap"
    buf.fill_(0xA5)
    rc, arc, st = _write(csa, files, dev, arc=buf[:23], **opts)
    assert rc == csa.WRITE_ERROR and st["launches"] == 0 and st["encode_launches"] == 0
    assert _bytes(buf) == b"\xa5" * (n + 64)


# ---- 7. retry --------------------------------------------------------------------------------------------------------------

def test_scratch_too_small_is_encoded_once_more(csa, trees, monkeypatch):
    files, src, want, opts, _, _ = trees("incompressible")
    monkeypatch.setenv("CSA_DEVWRITE_SLACK", "0")
    rc, arc, st = _write(csa, files, _upload(src), **opts)
    assert rc == 0 and st["retries"] >= 1 and _bytes(arc) == want


# ---- 8. round trip on the device ---------------------------------------------------------------------------------------------

def test_round_trip_on_the_device(csa):
    import torch
    files, src, content = csa_write_cases.table("mixed_tree", _edate(csa))
    opts = {k: v for k, v in csa_cases.CSA_CASES["mixed_tree"]["opts"].items() if k != "recurse"}
    rc, arc, st = _write(csa, files, _upload(src), **opts)
    assert rc == 0
    with csa.DeviceArchive.open(arc) as a:
        total = a.plan()[1]
        dst = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
        rc, views, rst = a.extract(dst=dst)
        assert rc == 0 and rst["verify_failures"] == 0
        for name, data in content.items():
            assert _bytes(views[name]) == data, name
    rc, again, st2 = _write(csa, rst["files"], dst, **opts)
    assert rc == 0 and _bytes(again) == _bytes(arc)


# ---- 9. the reference reads it ----------------------------------------------------------------------------------------------

@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/csarc_ref not in this snapshot")
def test_the_reference_reads_it(csa, trees, tmp_path):
    files, src, _, opts, content, _ = trees("frag_edges")
    rc, arc, st = _write(csa, files, _upload(src), **opts)
    assert rc == 0
    (tmp_path / "dev.csa").write_bytes(_bytes(arc))
    t = subprocess.run([CSARC_REF, "t", "dev.csa"], cwd=tmp_path, capture_output=True)
    assert t.returncode == 0 and b"failed" not in t.stderr
    subprocess.run([CSARC_REF, "x", "-o", "r", "dev.csa"], cwd=tmp_path, check=True, capture_output=True)
    for n, d in content.items():
        assert (tmp_path / "r" / n).read_bytes() == d


# ---- the refusals that need the source's size --------------------------------------------------------------------------------

def test_tables_refused_before_any_launch(csa):
    import torch
    src = torch.full((4096,), 7, dtype=torch.uint8, device="cuda")
    arc = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    row = {"name": "a", "esize": 100, "edate": _edate(csa), "eattr": csa_write_cases.FILE_ATTR, "offset": 0}

    def rc_of(rows, s=src, a=arc):
        rc, out, st = csa.DeviceArchive.write(rows, s, arc=a)
        assert out is None or rc == 0
        if rc != 0:
            assert st["launches"] == 0 and st["encode_launches"] == 0 and st["upload_bytes"] == 0
        return rc
    assert rc_of([row]) == 0
    assert rc_of([dict(row, offset=3997)]) == -1                                     # offset + esize past src_size
    assert rc_of([dict(row, offset=3996)]) == 0
    assert rc_of([dict(row, offset=(1 << 64) - 50)]) == -1                           # ... wrapping in 64 bits
    assert rc_of([row, dict(row)]) == -1                                             # a duplicate name
    assert rc_of([dict(row, name="d/")]) == -1                                       # a directory with bytes
    assert rc_of([dict(row, esize=-1)]) == -1
    both = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    assert rc_of([row], s=both[:4096], a=both[4000:]) == -1                          # [src, ..) overlaps [arc, ..)
    assert rc_of([row], s=both[:4096], a=both[4096:]) == 0
    assert bool((arc[csa.DeviceArchive.write([row], src, arc=arc)[2]["archive_bytes"]:] == 0xA5).all())
