"""CPU tier for entries gathered from strided slices of the caller's buffers (include/csa_mi355x.h: CSAMI_DeviceWriteSlices): the
declaration, the export, the ctypes mirror, the refusal without a device, tensor_slice's arithmetic on CPU tensors, and the text the
planner and k_frag_rows run (csc_amd/csrc/csa_dev_write.h: gather_whole, gather_reduce, gather_sum) compiled for the host with the
sanitizers and run as a program of its own (tests/model/csa_dev_gather_model.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "CSAMI_DeviceWriteSlices"
M64 = 1 << 64


@pytest.fixture(scope="module")
def csa(prod):
    from csc_amd import csa as m
    m.lib()
    return m


# ---- 1. declaration, export, layout, refusal --------------------------------------------------------------------------

def test_header_declares_the_call_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csa_mi355x.h"\n'
                   "int main(void){ CSADevFile f; CSADevWriteStats s; CSADevGatherStats g; CSADevSlice c; CSAOptions o;\n"
                   "  const void *p[1] = {0}; uint64_t n[1] = {0}; unsigned char arc[64];\n"
                   "  c.offset = 0; c.run = 1; c.stride = 2; c.count = 3; f.name = 0; CSA_OptionsInit(&o);\n"
                   "  g.selected_bytes = g.hull_bytes = g.periodic_pieces = g.plain_pieces = g.gathered_tasks = g.inplace_tasks = 0;\n"
                   '  return CSAMI_DeviceWriteSlices(p, n, &c, &f, 1, "a.csa", arc, sizeof(arc), &o, &s, &g) + (int)g.hull_bytes; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_call(csa):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    have = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert NEW in have and NEW in csa.SYMBOLS


def test_ctypes_mirror_has_the_c_layout(tmp_path, csa):
    name, T = "CSADevGatherStats", csa.CSADevGatherStats
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csa_mi355x.h"\nint main(void){\n'
                   + f'  printf(" %zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in T._fields_)
                   + "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_] and C.sizeof(T) == 48


def test_no_gpu_means_no_sliced_write(csa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = csa.lib()
    name = C.create_string_buffer(b"a")
    f = csa.CSADevFile()
    f.name, f.esize, f.offset, f.size, f.nfrags = C.cast(name, C.c_void_p), 4, 77, 78, 79
    before = bytes(f)
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    ptrs = (C.c_void_p * 1)(C.addressof(buf) + 1024)
    sizes = (C.c_uint64 * 1)(8)
    sl = (csa.CSADevSlice * 1)()
    sl[0].offset, sl[0].run, sl[0].stride, sl[0].count = 1, 2, 3, 2
    sliced = bytes(sl)
    st, gs = csa.CSADevWriteStats(), csa.CSADevGatherStats()
    for t in (st, gs):
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
    o = csa.options()
    assert L.CSAMI_DeviceWriteSlices(ptrs, sizes, sl, C.byref(f), 1, b"a.csa", C.addressof(buf) + 2048, 1024, C.byref(o), C.byref(st),
                                     C.byref(gs)) == csa.CSCMI_DEVICE_ERROR
    assert bytes(f) == before and bytes(buf) == b"\xa5" * 4096 and bytes(sl) == sliced
    for t in (st, gs):
        assert bytes(t) == b"\x5a" * C.sizeof(t), type(t).__name__


# ---- 2. tensor_slice on CPU tensors ---------------------------------------------------------------------------------------------

def _packed(csa, t):
    """the bytes tensor_slice's pair selects, by the definition; and the slice"""
    import torch
    base, (off, run, stride, count) = csa.tensor_slice(t)
    assert base.dtype == torch.uint8 and base.dim() == 1 and base.is_contiguous() and base.numel() == t.untyped_storage().nbytes()
    b = base.numpy().tobytes()
    assert count == 0 or off + (count - 1) * stride + run <= len(b)
    return b"".join(b[off + k * stride:off + k * stride + run] for k in range(count)), (off, run, stride, count)


def test_tensor_slice_selects_the_bytes_of_the_contiguous_copy():
    import torch
    from csc_amd import csa
    m = torch.arange(200 * 250, dtype=torch.float32).reshape(200, 250)
    x = torch.arange(4 * 6 * 8, dtype=torch.int16).reshape(4, 6, 8)
    want = {
        "a contiguous matrix is one range": (m, (0, 200000, 200000, 1)),
        "a block of columns is one run out of every row": (m[:, 10:20], (40, 40, 1000, 200)),
        "a block of rows is one range": (m[5:9], (5000, 4000, 4000, 1)),
        "one row": (m[3], (3000, 1000, 1000, 1)),
        "one column": (m[:, 7:8], (28, 4, 1000, 200)),
        "a block of one row": (m[2:3, 4:9], (2016, 20, 20, 1)),
        "every second element collapses with the rows": (m[:, ::2], (0, 4, 8, 25000)),
        "three dimensions, the middle one cut": (x[:, 1:3, :], (16, 32, 96, 4)),
        "three dimensions, the last one cut, whose rows continue across the first": (x[:, :, 2:5], (4, 6, 16, 24)),
        "a view at a storage offset": (m.view(-1)[77:][:100], (308, 400, 400, 1)),
        "nothing": (m[:0], (0, 0, 0, 0)),
    }
    for what, (t, s) in want.items():
        got, sl = _packed(csa, t)
        assert sl == s, what
        assert got == t.contiguous().view(-1).view(torch.uint8).numpy().tobytes(), what
    for what, t in {"a transpose": m.t(), "two levels of striding": x[:, 1:3, 2:4], "an expanded dimension": m[:1].expand(3, 250),
                    "a cut of the last two of three dimensions": x[:, :2, 1:]}.items():
        with pytest.raises(ValueError):
            csa.tensor_slice(t)


# ---- 3. the planner's and the kernel's text on the CPU ------------------------------------------------------------------------

BIG = [1, 2, 15, 16, 17, 16383, 16384, 16385, 1 << 31, 1 << 32, 1 << 63]
LENS = [1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384]
PATTERNS = [(1, 2), (1, 16), (3, 5), (15, 16), (16, 16), (16, 17), (17, 48), (100, 1000), (4096, 4097), (16384, 16384),
            (7, 11), (16, 33), (4097, 8197)]


def _model_cases():
    """the cases tests/model/csa_dev_gather_model.cpp runs, counted by its rules"""
    count = 0
    for run in BIG:
        for stride in BIG:
            if stride < run:
                continue
            rows = next(c for c in (3, 2, 1) if 5 + (c - 1) * (stride if c > 1 else run) + run < M64)
            for _ in (1, 16, 16384):
                for row in (0, rows - 1):                          # (one row: the same row twice, as the model walks it)
                    count += sum(row * run + r0 < run * rows for r0 in (0, run // 2, run - 1, run))
    count += 16 * 16 * len(LENS) * len(PATTERNS)
    return count + 4 * 7 * 4


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devgather") / "csa_dev_gather_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "csa_dev_gather_model.cpp"), "-o", exe], check=True)

    def run(plant):
        return subprocess.run([exe, str(plant)], capture_output=True, text=True, timeout=600)
    return run


def test_gather_reduce_and_gather_sum_under_the_sanitizers(model):
    """every (run, stride) pair around the powers the reduction turns on x three spans x every phase class against the 64-bit
    definition; 16 x 16 alignments x 13 lengths x 13 patterns of gather_sum out of sources exactly as large as their hulls;
    fragments of three pieces end to end"""
    out = model(0)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == f"ok {_model_cases()}"


@pytest.mark.parametrize("plant,how,where", [
    # the run border one byte late: the first length with a unit, under the first pattern -- its second byte is a gap byte
    (1, "FAIL", "sum sa=0 da=0 n=16 run=1 stride=2"),
    # phase dropped from a thread's first unit: the first length with a unit, under the first pattern whose phase there, 16 % 3, is not 0
    (2, "FAIL", "sum sa=0 da=0 n=16 run=3 stride=5"),
    # a unit across a run border loaded as if contiguous: the first length with a unit, under the first pattern
    (3, "FAIL", "sum sa=0 da=0 n=16 run=1 stride=2"),
    # the row not advanced on the carry: a thread's SECOND unit (more than 256 units: 16383 bytes), under the first pattern whose
    # run does not divide the workgroup's step of 4096 positions
    (4, "FAIL", "sum sa=0 da=0 n=16383 run=3 stride=5"),
    # the load window checked against the run -- its unit lies inside it, always -- and not against the hull: the first piece whose
    # last unit is misaligned and ends with the hull, two rows of 16 a stride of 17 apart, the second at address 17 of a hull of 33
    # bytes; the sanitizer sees the load
    (5, "AT", "sum sa=0 da=0 n=32 run=16 stride=17"),
])
def test_planted_mistakes_are_caught_at_named_cases(model, plant, how, where):
    out = model(plant)
    assert out.returncode != 0
    if how == "FAIL":
        assert out.stdout.strip().splitlines()[-1] == f"FAIL {where}"
    else:
        named = [l for l in out.stderr.splitlines() if l.startswith("AT ")]
        assert named[-1] == f"AT {where}" and "heap-buffer-overflow" in out.stderr and "csa_dev_read.h" in out.stderr
