"""GPU tier for the early stop of the device-resident archive read (CSAMI_DeviceReadStop; DeviceArchive.extract / test with
stop_early=True): every task is decoded only up to its last selected byte, and what comes out is what CSAMI_DeviceRead delivers
for the same selection -- the comparison partner throughout, called on the same handle.  The plan (which tasks, their stops and
raw sizes) is CSAMI_PlanDeviceStops over the archive's raw index, itself pinned by the CPU tier.

Archives are written once per module by `csa.add` (and by the reference archiver where oracle/_ref travelled with the snapshot);
each is a few hundred KB."""
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

# six files of one extension and of different data kinds: ONE task of several runs (csarc.cpp:545-557)
SIX = {"s/a.bin": [["text", 71, 0, 150000]], "s/b.bin": [["exe", 72, 0, 100000]], "s/c.bin": [["delta", 73, 0, 120000]],
       "s/d.bin": [["random", 74, 0, 100000]], "s/e.bin": [["zeros", 110000]], "s/f.bin": [["entropy8", 75, 0, 100001]]}
EDGE_SIZES = [1, 15, 16, 17, 4095, 16385, 32769, 70001]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def dec(orc, zalloc):
    def dec(stream):
        rc, raw = orc.decode(stream, alloc=zalloc)
        assert rc == 0
        return raw
    return dec


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
    """{name: (path of the archive, its bytes, {relpath: content}, raw index bytes)}, written once"""
    out = {}
    cwd = os.getcwd()

    def keep(name, d, arcname, content):
        path = str(d / arcname)
        out[name] = (path, (d / arcname).read_bytes(), content, csa.read_index(path))

    try:
        for case in ("mixed_tree", "no_data"):
            d = tmp_path_factory.mktemp(case)
            content = csa_cases.make_tree(str(d), case)
            os.chdir(d)
            spec = csa_cases.CSA_CASES[case]
            assert csa.add(csa_cases.ARCNAME, spec["args"], overwrite=True, **spec["opts"])[0] == 0
            keep(case, d, csa_cases.ARCNAME, content)
        d = tmp_path_factory.mktemp("six")
        content = _write_tree(str(d), SIX)
        os.chdir(d)
        assert csa.add("out.csa", ["s"], overwrite=True, recurse=True, level=1, dict_size=256 << 10)[0] == 0
        keep("six", d, "out.csa", content)
        if HAVE_REF:
            subprocess.run([CSARC_REF, "a", "-m1", "-d256k", "-r", "-f", "ref.csa", "s"], cwd=d, check=True, capture_output=True)
            keep("six_ref", d, "ref.csa", content)
        # files cut across tasks (task_bytes), and one file in seven slices of its own
        d = tmp_path_factory.mktemp("edges")
        content = _write_tree(str(d), {f"e/f{n:05d}.bin": [["text", 50 + i, 0, n]] for i, n in enumerate(EDGE_SIZES)})
        os.chdir(d)
        assert csa.add("out.csa", ["e"], overwrite=True, recurse=True, level=1, dict_size=64 << 10, task_bytes=20000)[0] == 0
        keep("edges", d, "out.csa", content)
    finally:
        os.chdir(cwd)
    return out


def _upload(data):
    import torch
    t = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _open(csa, data):
    return csa.DeviceArchive.open(_upload(data))


def _by_position(csa, path, names):
    """the files of `names` in the order their first fragments lie in their task"""
    entries = {e["name"]: e for e in csa.list_entries(path)}
    return sorted(names, key=lambda n: entries[n]["frags"][0]["posblock"])


def _both(csa, a, names, total, **opts):
    """extract(names) and extract(names, stop_early=True) into canary-filled buffers -> ((rc, files, bytes of the whole dst, stats)) x 2"""
    import torch
    out = []
    for stop in (False, True):
        buf = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, views, st = a.extract(names, dst=buf[:total], stop_early=stop, **opts)
        assert set(views) == {f["name"] for f in st["files"]}
        out.append((rc, st["files"], buf.cpu().numpy().tobytes(), st))
    return out


def _selections(csa, name, path, content):
    if name.startswith("six"):
        order = _by_position(csa, path, list(SIX))
        return [[], [order[0]], [order[-1]], [order[2], order[1]], ["nothing"]]
    if name == "mixed_tree":
        return [[], ["d/a.txt"], ["d/b.txt"], ["d/empty"], ["d/sub"], ["d/empty", "d"]]
    if name == "edges":
        return [[], ["e/f70001.bin"], ["e/f00001.bin"], ["e/f16385.bin", "e/f00015.bin"]]
    return [[]]


# ---- 1. every selection: the same answer as the unstopped read, for what the plan says it costs ------------------------------

@pytest.mark.parametrize("name", ["six", "six_ref", "mixed_tree", "edges", "no_data"])
def test_stop_early_equals_the_full_read(csa, arcs, name):
    if name not in arcs:
        pytest.skip("oracle/_ref/csarc_ref not in this snapshot")
    path, arc, content, raw_index = arcs[name]
    stopped_somewhere = False
    with _open(csa, arc) as a:
        for names in _selections(csa, name, path, content):
            rcp, plan = csa.plan_device_stops(raw_index, len(arc), names)
            assert rcp == 0
            total = a.plan(names)[1]
            (rc0, files0, dst0, st0), (rc1, files1, dst1, st1) = _both(csa, a, names, total)
            assert rc0 == rc1 == 0 and files0 == files1 and dst0 == dst1, (name, names)
            assert st0["verify_failures"] == st1["verify_failures"] == 0
            for f in files1:
                data = content.get(f["name"], b"")
                assert dst1[f["offset"]:f["offset"] + f["size"]] == data and f["failed_frags"] == 0, f["name"]
            assert dst1[total:] == b"\xa5" * 32
            assert st1["decoded_bytes"] == sum(t["stop"] for t in plan), (name, names)
            assert st1["task_raw_bytes"] == sum(t["raw"] for t in plan)
            assert st1["scratch_bytes"] == sum((t["stop"] + 255) // 256 * 256 for t in plan)
            assert st1["stopped_tasks"] == sum(1 for t in plan if t["stop"] < t["raw"])
            assert st1["tasks"] == st0["tasks"] == len(plan) and st1["frags"] == st0["frags"] and st1["raw_bytes"] == st0["raw_bytes"]
            assert st1["launches"] == 3 * st1["waves"] and st1["waves"] == st0["waves"]
            assert st1["readback_bytes"] == st0["readback_bytes"]
            assert "decoded_bytes" not in st0                                         # the default call's dict is what it was
            # `csarc t`: the same without dst
            rct, stt = a.test(names, stop_early=True)
            assert rct == 0 and stt["verify_failures"] == 0 and stt["files"] == files1
            assert [stt[k] for k in ("decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks", "launches")] == \
                   [st1[k] for k in ("decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks", "launches")]
            stopped_somewhere |= st1["stopped_tasks"] > 0
            if name.startswith("six") and len(names) == 1 and names[0] != "nothing":
                first = names[0] == _by_position(csa, path, list(SIX))[0]
                assert (st1["decoded_bytes"] < st1["task_raw_bytes"]) == first        # the first file costs less than the task, the last all of it
                assert st1["decoded_bytes"] == (len(content[names[0]]) if first else sum(len(c) for c in content.values()))
    assert stopped_somewhere == (name != "no_data")


def test_dst_one_byte_short(csa, arcs):
    import torch
    path, arc, content, _ = arcs["six"]
    first = _by_position(csa, path, list(SIX))[0]
    with _open(csa, arc) as a:
        total = a.plan([first])[1]
        buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, views, st = a.extract([first], dst=buf[:total - 1], stop_early=True)
    assert rc == csa.WRITE_ERROR and views == {}
    assert [st[k] for k in ("launches", "decode_launches", "waves", "tasks", "readback_bytes", "decoded_bytes", "task_raw_bytes",
                            "scratch_bytes", "stopped_tasks")] == [0] * 9
    assert bool((buf == 0xA5).all())


# ---- 2. damage behind the stop -----------------------------------------------------------------------------------------------

def test_damage_behind_the_selection_is_not_decoded(csa, arcs, dec, tmp_path):
    path, arc, content, _ = arcs["six"]
    info = orc_csa.parse(arc, dec)
    assert len(info["abindex"]) == 1
    (bid, blocks), = info["abindex"].items()
    o, n = blocks[-1]
    bad = bytearray(arc)
    bad[o + n - 64:o + n] = b"\x5a" * 64                                               # the tail of the task's last archive block; the index is intact
    bad = bytes(bad)
    (tmp_path / "bad.csa").write_bytes(bad)
    order = _by_position(csa, path, list(SIX))
    first, last = order[0], order[-1]
    with _open(csa, bad) as a:
        # the preconditions: the callback path stops behind the selection and answers 0, the unstopped device read does not
        assert csa.test(str(tmp_path / "bad.csa"), [first])[0] == 0
        total = a.plan([first])[1]
        (rc0, _, _, _), (rc1, files1, dst1, st1) = _both(csa, a, [first], total)
        assert rc0 == -1
        assert rc1 == 0 and st1["verify_failures"] == 0 and files1[0]["failed_frags"] == 0
        assert dst1[:len(content[first])] == content[first] and st1["decoded_bytes"] == len(content[first])
        # the last file needs the whole task: -1 in all three
        assert csa.test(str(tmp_path / "bad.csa"), [last])[0] == -1
        assert a.extract([last])[0] == -1 and a.extract([last], stop_early=True)[0] == -1 and a.test([last], stop_early=True)[0] == -1


def _flip_in_a_stored_byte(arc, info, dec, lo, hi):
    """the archive with one byte of its single task's stream changed such that the stream still decodes and the decoded bytes differ
    inside [lo, hi) only: a byte of a bit-coder block that carries stored (incompressible) bytes, found by trying with the oracle"""
    (bid, blocks), = info["abindex"].items()
    stream = b"".join(arc[o:o + n] for o, n in blocks)
    good = dec(stream)
    bsize = int.from_bytes(stream[4:7], "big")
    p, cands = 10, []
    while p < len(stream):                                                             # the framing, csc_memio.cpp:17-79
        fb, q, n = stream[p], p + 1, bsize
        if not fb & 64:
            n, q = int.from_bytes(stream[q:q + 3], "big"), q + 3
        if not fb & 128 and n > 4096:
            cands.append(q + n // 2)
        p = q + n
    for at in cands[:12]:
        s = bytearray(stream)
        s[at] ^= 0x01
        try:
            out = dec(bytes(s))
        except AssertionError:
            continue
        diff = [i for i in range(min(len(out), len(good))) if out[i] != good[i]]
        if len(out) == len(good) and diff and lo <= diff[0] and diff[-1] < hi:
            pos, bad = at, bytearray(arc)
            for o, n in blocks:                                                        # stream position -> archive position
                if pos < n:
                    bad[o + pos] ^= 0x01
                    return bytes(bad)
                pos -= n
    return None


def test_corrupted_byte_inside_the_selected_fragment(csa, arcs, dec):
    path, arc, content, _ = arcs["six"]
    info = orc_csa.parse(arc, dec)
    f = info["index"]["s/d.bin"]["frags"][0]                                           # the incompressible file: its bytes are stored
    bad = _flip_in_a_stored_byte(arc, info, dec, f["posblock"], f["posblock"] + f["size"])
    assert bad is not None, "no stored byte found to corrupt"
    with _open(csa, bad) as a:
        total = a.plan(["s/d.bin"])[1]
        for rc, files, dst, st in _both(csa, a, ["s/d.bin"], total):
            assert rc == 0 and st["verify_failures"] == 1 and [x["failed_frags"] for x in files] == [1]
            assert dst[:100000] != content["s/d.bin"] and len(files) == 1


# ---- 3. waves ------------------------------------------------------------------------------------------------------------------

def test_waves(csa, arcs):
    path, arc, content, raw_index = arcs["mixed_tree"]
    names = ["d/a.txt", "d/sub/c.exe", "d/noext"]
    plan = csa.plan_device_stops(raw_index, len(arc), names)[1]
    with _open(csa, arc) as a:
        total = a.plan(names)[1]
        (_, _, _, _), one = _both(csa, a, names, total)
        (_, _, _, _), per_task = _both(csa, a, names, total, device_streams=1)
        (_, _, _, _), tiny = _both(csa, a, names, total, hbm_budget=1 << 20)
    assert one[0] == 0 and one[3]["waves"] == 1 and len(plan) == 3 and one[3]["stopped_tasks"] >= 1
    for rc, files, dst, st in (per_task, tiny):
        assert (rc, files, dst) == one[:3]
        assert st["waves"] == 3 and st["launches"] == 9
        assert [st[k] for k in ("decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks", "verify_failures")] == \
               [one[3][k] for k in ("decoded_bytes", "task_raw_bytes", "scratch_bytes", "stopped_tasks", "verify_failures")]
