"""CPU tier for the device-resident archive write (CSAMI_DeviceWritePlan / CSAMI_DeviceWrite, include/csa_mi355x.h): the
declarations, the exports, the refusal without a device, the host-only planner over a table built with no tree on disk against
oracle/orc_csa.py's plan and against CSAMI_PlanInfo over the same tree on disk, the refusals, and k_block_table's text
(csc_amd/csrc/csa_dev_write.h: the walk over a framed stream and the archive-block coalescer) compiled for the host with the
sanitizers and run as a program of its own (tests/model/csa_dev_write_model.cpp) on the oracle encoder's streams and on
constructed ones."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

import cases
import csa_cases
import csa_write_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc_csa  # noqa: E402

TWO = ["CSAMI_DeviceWritePlan", "CSAMI_DeviceWrite"]


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_calls_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevFile f; CSADevWriteStats s; uint32_t nt = 0, mf = 0; uint64_t raw = 0; double ms[4];\n"
                   "  f.name = \"a\"; f.esize = f.edate = f.eattr = 0; f.offset = f.size = 0; f.nfrags = f.failed_frags = 0;\n"
                   "  s.tasks = s.frags = s.waves = s.blocks = s.launches = s.encode_launches = s.readback_bytes = s.upload_bytes = 0;\n"
                   "  s.raw_bytes = s.archive_bytes = s.index_raw_size = s.index_compressed_size = 0; s.n_entries = s.retries = 0;\n"
                   "  s.kernel_ms = s.seconds_encode = s.seconds_total = 0;\n"
                   "  CSAMI_DeviceWriteKernelMs(ms);\n"
                   "  if (CSAMI_DeviceWritePlan(&f, 1, \"out.csa\", 0, &nt, &mf, &raw)) return 1;\n"
                   "  return CSAMI_DeviceWrite(0, 0, &f, 1, \"out.csa\", 0, 0, 0, &s); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_two_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in TWO if s not in have] == []


def test_ctypes_mirror_has_the_c_layout(tmp_path, csa):
    S = csa.CSADevWriteStats
    sf = [n for n, _ in S._fields_]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){ printf("%zu", sizeof(CSADevWriteStats));\n'
                   + "".join(f'  printf(" %zu", offsetof(CSADevWriteStats, {n}));\n' for n in sf) + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in sf]
    assert set(S().as_dict()) == set(sf)


def test_no_gpu_means_no_device_write(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    arr, keep = csa._write_table([{"name": "a", "esize": 4, "edate": 1, "eattr": 2, "offset": 0}])
    src, arc = (C.c_uint8 * 64)(), (C.c_uint8 * 4096)()
    st = csa.CSADevWriteStats()
    st.tasks, arr[0].nfrags = 77, 55
    rc = csa.lib().CSAMI_DeviceWrite(src, 64, arr, 1, b"out.csa", arc, 4096, None, C.byref(st))
    assert rc == csa.CSCMI_DEVICE_ERROR, "there is no CPU fallback"
    assert st.tasks == 77 and arr[0].nfrags == 55 and bytes(arc) == bytes(4096), "no argument is touched"


# ---- 2. the planner ---------------------------------------------------------------------------------------------------

def _edate(csa):
    return int(csa.lib().CSA_DecimalTime(csa_cases.MTIME))


@pytest.mark.parametrize("case", csa_cases.CPU_CASES)
def test_planner_equals_the_oracle_plan_and_the_plan_of_the_tree_on_disk(csa, case, tmp_path, monkeypatch):
    spec = csa_cases.CSA_CASES[case]
    files, _, _ = csa_write_cases.table(case, _edate(csa), with_bytes=False)
    keys = ("level", "dict_size", "split_count")
    opts = {k: v for k, v in spec["opts"].items() if k in keys}
    rc, nt, mf, raw = csa.device_write_plan(files, csa_cases.ARCNAME, **opts)
    index = {f["name"]: {"esize": f["esize"], "edate": f["edate"], "eattr": f["eattr"], "ext": b"\0\0\0\0", "frags": []} for f in files}
    tasks = orc_csa.plan_tasks(index, max(spec["opts"].get("split_count", 1), 1))
    per_file = {}
    for t in tasks:
        for name, _, _ in t["files"]:
            per_file[name] = per_file.get(name, 0) + 1
    assert (rc, nt, mf, raw) == (0, len(tasks), max(per_file.values(), default=0), sum(t["total"] for t in tasks))
    csa_cases.make_tree(str(tmp_path), case)
    monkeypatch.chdir(tmp_path)
    assert csa.plan_info(spec["args"], **spec["opts"]) == (rc, nt, mf)
    # the order of the table does not matter, and task_bytes cuts both plans alike
    assert csa.device_write_plan(files[::-1], csa_cases.ARCNAME, **opts) == (rc, nt, mf, raw)
    cut = csa.device_write_plan(files, csa_cases.ARCNAME, task_bytes=50000, **opts)
    assert cut[:3] == csa.plan_info(spec["args"], task_bytes=50000, **spec["opts"]) and cut[3] == raw


def test_a_128_fragment_split_is_refused(csa):
    one = [{"name": "huge.bin", "esize": 200 << 20, "edate": 1, "eattr": csa_write_cases.FILE_ATTR, "offset": 0}]
    rc, nt, mf, raw = csa.device_write_plan(one, split_count=128)                 # 128 slices of 1.5625 MiB + 4, and a tail
    assert rc == csa.CSA_TOO_MANY_FRAGMENTS and mf >= 128
    rc, nt, mf, raw = csa.device_write_plan(one, split_count=127)
    assert rc == 0 and mf <= csa.CSA_MAX_FRAGMENTS and raw == 200 << 20


def _plan_raw(csa, rows, n=None, null_table=False):
    """CSAMI_DeviceWritePlan over rows of (name or None, esize)"""
    keep = [C.create_string_buffer(r[0]) if r[0] is not None else None for r in rows]
    arr = (csa.CSADevFile * max(len(rows), 1))()
    for a, r, k in zip(arr, rows, keep):
        a.name = C.cast(k, C.c_void_p) if k is not None else None
        a.esize = r[1]
    nt, mf, raw = C.c_uint32(), C.c_uint32(), C.c_uint64()
    return csa.lib().CSAMI_DeviceWritePlan(None if null_table else arr, len(rows) if n is None else n, b"out.csa", None,
                                           C.byref(nt), C.byref(mf), C.byref(raw))


def test_tables_the_host_refuses(csa):
    assert _plan_raw(csa, [(b"a", 5), (b"d/", 0), (b"b", 0)]) == 0
    assert _plan_raw(csa, [], n=0, null_table=True) == 0
    assert _plan_raw(csa, [(b"a", 5)], n=1, null_table=True) == -1                 # n_files > 0 with files == NULL
    assert _plan_raw(csa, [(b"a", 5), (None, 1)]) == -1                            # a NULL name
    assert _plan_raw(csa, [(b"a", 5), (b"b", 1), (b"a", 5)]) == -1                 # a duplicate name
    assert _plan_raw(csa, [(b"a", -1)]) == -1                                      # esize < 0
    assert _plan_raw(csa, [(b"d/", 1)]) == -1                                      # a directory with bytes
    assert _plan_raw(csa, [(b"a", 1 << 59), (b"b", 1 << 59), (b"c", 1)]) == -1     # sizes whose sum leaves the checked range


# ---- 3. k_block_table's text on the CPU ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devwrite") / "csa_dev_write_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_write_model.cpp"), "-o", exe], check=True)

    def run(plant, path=None):
        return subprocess.run([exe, str(plant)] + ([path] if path else []), capture_output=True, text=True, timeout=600)
    return run


def _tables(stdout):
    out = {}
    for line in stdout.splitlines():
        if line.startswith("table "):
            head, sizes = line[6:].split(" :")
            name, rest = head.split(" status ")
            status, nblocks = rest.split(" blocks ")
            out[name] = (int(status), int(nblocks), [int(x) for x in sizes.split()])
    return out


def _coalesce(writes):
    co = orc_csa.BlockCoalescer()
    for s in writes:
        co.write(s)
    return co.finish()


def test_block_table_of_oracle_streams(model, orc, zalloc, tmp_path):
    """levels 1, 2, 3 x text, exe, entropy: the table from the stream's bytes is the table from the encoder's Write sizes"""
    from csc_amd.capi import BytesWriter
    want, blob = [], bytearray()
    for level in (1, 2, 3):
        for i, kind in enumerate(("text", "exe", "entropy8")):
            data = cases.build([[kind, 70 + i, 0, 300000]])
            w = BytesWriter()
            props = orc.props_init(len(data), level)
            rc, s = orc.encode(data, props=props, alloc=zalloc, writer=w)
            assert rc == 0
            want.append(_coalesce([10] + w.sizes))
            blob += struct.pack("<IQ", props.csc_blocksize, len(s) - 10) + s[10:]
    path = tmp_path / "streams.bin"
    path.write_bytes(struct.pack("<I", len(want)) + bytes(blob))
    out = model(0, str(path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = _tables(out.stdout)
    assert [got[str(k)] for k in range(len(want))] == [(0, len(w), w) for w in want]


CONSTRUCTED = ["empty stream", "bit-6 block", "empty payload", "exactly 1 MiB at a flush point", "1 MiB + 1 at a flush point",
               "full blocks across 1 MiB", "payload above 1 MiB", "one byte short of the last payload", "cut inside a size field"]


def test_block_table_of_constructed_streams(model):
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1] == f"ok {len(CONSTRUCTED)}"
    got = _tables(out.stdout)
    writes = {l[7:].split(" :")[0]: [int(x) for x in l.split(" :")[1].split()] for l in out.stdout.splitlines() if l.startswith("writes ")}
    assert list(got) == CONSTRUCTED
    for name in CONSTRUCTED[:7]:
        assert got[name] == (0, len(_coalesce(writes[name])), _coalesce(writes[name])), name
    for name in CONSTRUCTED[7:]:
        assert got[name][0] == 1, name                                             # kTableCut, and no load behind the end (ASan)
    MiB = 1 << 20
    assert got["exactly 1 MiB at a flush point"][2] == [MiB, 4] and got["1 MiB + 1 at a flush point"][2] == [14, MiB - 13 + 4]
    assert writes["bit-6 block"] == [10, 1, 64, 1, 3] and writes["empty payload"] == [10, 1, 3, 100, 1, 3, 1, 3, 7, 1, 3]
    assert got["payload above 1 MiB"][2] == [10 + 4 + 5 + 4, MiB + 100, 4 + 9 + 4]  # cap = max(1 MiB, size)


@pytest.mark.parametrize("plant,where", [
    (1, "exactly 1 MiB at a flush point"),       # >= for > in the flush test
    (2, "empty stream"),                          # the 10 property bytes left out
    (3, "bit-6 block"),                           # the bit-6 size taken from the size field
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, where):
    out = model(plant)
    assert out.returncode != 0
    assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
