"""CPU tier for the device archive's update in place (include/csa_mi355x.h: CSAMI_DeviceUpdateInPlace, CSAMI_DeviceMoveKernelMs): the
declarations, the exports, the ctypes mirror, the refusal without a device, and the move layer -- plan_moves and the text one thread
of k_move_extents runs (csc_amd/csrc/csa_dev_move.h) -- compiled for the host with the sanitizers and run as a program of its own
(tests/model/csa_dev_move_model.cpp) under three kinds of schedule, every case compared with the copy that reads every source before
it writes any destination."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["CSAMI_DeviceUpdateInPlace", "CSAMI_DeviceMoveKernelMs"]
CHUNK = 32768


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_call_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevFile f; CSADevWriteStats s; CSADevGatherStats g; CSADevUpdateStats u; CSADevUpdateTask t[2]; CSAOptions o;\n"
                   "  CSADevDigest d[2]; CSADevDigestStats ds; CSADevMoveStats ms; double k[3];\n"
                   "  const void *p[1] = {0};\n"
                   "  f.name = 0; CSA_OptionsInit(&o);\n"
                   "  ms.moves = ms.moved_bytes = ms.parked_moves = ms.parked_bytes = ms.held_stream_bytes = ms.launches = 0; ms.kernel_ms = 0;\n"
                   "  CSAMI_DeviceMoveKernelMs(k);\n"
                   '  return CSAMI_DeviceUpdateInPlace(0, 64, d, 2, p, 0, 0, &f, 1, "a.csa", CSAMI_UPDATE_TRUST_DIGESTS, &o, &s, &g, &u, t, 2, d, 2,\n'
                   "                                   &ds, &ms); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_calls(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert [s for s in NEW if s not in have or s not in csa.SYMBOLS] == []


def test_ctypes_mirror_has_the_c_layout(tmp_path, csa):
    T = csa.CSADevMoveStats
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   '  printf(" %zu", sizeof(CSADevMoveStats));\n'
                   + "".join(f'  printf(" %zu", offsetof(CSADevMoveStats, {n}));\n' for n, _ in T._fields_) + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(T) == 56 and got == [56] + [getattr(T, n).offset for n, _ in T._fields_]
    assert len(T().as_dict()) == len(T._fields_)
    assert not set(T().as_dict()) & (set(csa.CSADevWriteStats().as_dict()) | set(csa.CSADevUpdateStats().as_dict())
                                     | set(csa.CSADevGatherStats().as_dict()) | set(csa.CSADevDigestStats().as_dict()))


def test_no_gpu_means_no_update_in_place(csa):
    """the call has no refusal in front of the device check: without a device it is CSCMI_DEVICE_ERROR, as its siblings are, and
    nothing it was handed is touched"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    name = C.create_string_buffer(b"a")
    f = csa.CSADevFile()
    f.name, f.esize, f.offset, f.size, f.nfrags = C.cast(name, C.c_void_p), 4, 77, 78, 79
    before = bytes(f)
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    at = C.addressof(buf)
    ptrs = (C.c_void_p * 1)(at + 1024)
    st, gs, us, tasks = csa.CSADevWriteStats(), csa.CSADevGatherStats(), csa.CSADevUpdateStats(), (csa.CSADevUpdateTask * 2)()
    ds, ms = csa.CSADevDigestStats(), csa.CSADevMoveStats()
    every = (st, gs, us, tasks, ds, ms)
    for t in every:
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    o = csa.options()
    # (the handle is not looked at either: the refusal comes first)
    for handle, cap, flags in ((C.c_void_p(0x1234), 1024, csa.CSAMI_UPDATE_TRUST_DIGESTS), (None, 0, 3)):
        assert L.CSAMI_DeviceUpdateInPlace(handle, cap, at + 3200, 1, ptrs, None, None, C.byref(f), 1, b"a.csa", flags, C.byref(o), C.byref(st),
                                           C.byref(gs), C.byref(us), tasks, 2, at + 3072, 1, C.byref(ds), C.byref(ms)) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096
    for t in every:
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. the move layer on the CPU ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devmove") / "csa_dev_move_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_move_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


L3 = 3 * CHUNK + 5
SHIFTS = [1, -1, 15, -15, 16, -16, 17, -17, CHUNK - 1, -(CHUNK - 1), CHUNK, -CHUNK, CHUNK + 1, -(CHUNK + 1), L3 + 7, -(L3 + 7)]
LENS = [1, 15, 16, 17, CHUNK - 1, CHUNK + 1, L3]


def test_the_chunk_size_is_the_headers(csa):
    src = open(os.path.join(ROOT, "csc_amd", "csrc", "csa_dev_move.h")).read()
    assert f"constexpr uint32_t kMoveChunk = {CHUNK};" in src and 16384 <= CHUNK <= 65536


def test_the_move_text_under_the_sanitizers(model):
    """every case under every schedule -- stores as early as allowed, as late as possible, seeded random interleavings with 1, 2, 3
    and 7 workgroups resident -- out of a buffer exactly as large as the archive: the bytes are those of reading every source
    first; every plan keeps a chunk's destination off the sources of higher tickets; archives in id order park nothing"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    cases = [l[5:] for l in out.stdout.splitlines() if l.startswith("case ")]
    want = ([f"shift={s} len={L3}" for s in SHIFTS] + [f"len={n} shift={s}" for n in LENS for s in (1, -1, 17, -17)]
            + [f"align sa={a} da={d}" for a in range(16) for d in range(16)] + ["id order: 40 streams, one grown, one shrunk"]
            + [f"id order: random {k}" for k in range(30)] + ["swap", "interleaved extents"] + [f"random {k}" for k in range(200)])
    assert cases == want
    assert out.stdout.splitlines()[-1] == f"ok {len(want)}"


@pytest.mark.parametrize("plant,where,what", [
    # hi one ticket short: the first chunk whose destination meets a lower ticket's source -- the second of a move shifted by one byte
    (1, f"shift=1 len={L3}", "plan: a chunk's destination meets a lower ticket outside [lo, hi]"),
    # the right phase sorted ascending: the same move, whose first chunk then stores into the second's source
    (2, f"shift=1 len={L3}", "plan: a chunk's destination meets the source of a higher ticket"),
    # parking switched off: the stream that moves right is read after the left phase has stored into it
    (3, "swap", "bytes differ under early"),
    # coalescing across unequal shifts: the first list whose sources are adjacent and whose shifts are not
    (4, "swap", "plan: a chunk leaves the buffer"),
    # a chunk that stores its first unit before its last load: the first move that overlaps its own source
    (5, f"shift=1 len={L3}", "bytes differ under early"),
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, where, what):
    out = model(plant)
    assert out.returncode == 3, out.stdout[-1000:] + out.stderr[-3000:]
    assert out.stdout.splitlines()[-1] == f"FAIL {where}: {what}"
