"""CPU tier for the device-resident encode (CSCMI_EncodeDeviceBatch): the declarations, the export, the refusal without a
device, and the framing (csc_amd/csrc/csc_enc_frame.h: the record walk, the dst_cap rule and the copy k_frame_blocks is built
from) compiled for the host with the sanitizers and run, as a program of its own, against a replay of the checker's Write
sequence written here."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

import cases
import enc_device_cases as E
import soak_gen
from csc_amd.capi import WRITE_ERROR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. declaration and export --------------------------------------------------------------------------------------

def test_header_declares_the_call_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csc_mi355x.h"\n'
                   "int main(void){ CSCMIDevEncode j; CSCMIDevEncodeStats s; j.rc = CSCMI_NO_ENCODER;\n"
                   "  j.props.dict_size = 0; j.src = 0; j.src_size = 0; j.dst = 0; j.dst_cap = 0; j.produced = 0;\n"
                   "  s.launches = s.rounds = s.readback_bytes = 0; s.kernel_ms = 0;\n"
                   "  return CSCMI_EncodeDeviceBatch(0, &j, &s) + (j.rc == CSCMI_DEVICE_ERROR || j.rc == CSCMI_NO_DECODER ? 1 : 0) + (int)s.launches; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_call():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "CSCMI_EncodeDeviceBatch" in [l.split()[-1] for l in out.splitlines() if l.strip()]


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    from csc_amd import device
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csc_mi355x.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(CSCMIDevEncode), '
                   "offsetof(CSCMIDevEncode, src), offsetof(CSCMIDevEncode, src_size), offsetof(CSCMIDevEncode, dst), offsetof(CSCMIDevEncode, dst_cap), "
                   "offsetof(CSCMIDevEncode, produced), offsetof(CSCMIDevEncode, rc), sizeof(CSCMIDevEncodeStats), "
                   "offsetof(CSCMIDevEncodeStats, kernel_ms), CSCMI_NO_ENCODER); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, S = device.CSCMIDevEncode, device.CSCMIDevEncodeStats
    assert got == [C.sizeof(D), D.src.offset, D.src_size.offset, D.dst.offset, D.dst_cap.offset, D.produced.offset, D.rc.offset,
                   C.sizeof(S), S.kernel_ms.offset, device.CSCMI_NO_ENCODER]


def test_no_gpu_means_no_device_encode(prod):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from csc_amd import device
    fn = device.bind_encode(prod)
    assert fn(0, None, None) == 0                                           # nothing to do is not an error
    dst = (C.c_uint8 * 64)(*([0xA5] * 64))
    jobs = (device.CSCMIDevEncode * 3)()
    for k, j in enumerate(jobs):
        j.props = prod.props_init(1 << 20, 3)
        if k == 2:
            j.props.lz_mode = 0                                             # not even the props check speaks without a device
        j.src = 0x1000; j.src_size = 100; j.dst = C.addressof(dst); j.dst_cap = 64
        j.rc = 77; j.produced = 5
    stats = device.CSCMIDevEncodeStats()
    assert fn(3, jobs, C.byref(stats)) == device.CSCMI_DEVICE_ERROR, "there is no CPU fallback"
    assert [(j.rc, j.produced) for j in jobs] == [(77, 5)] * 3
    assert bytes(dst) == b"\xa5" * 64 and stats.launches == 0 and stats.rounds == 0 and stats.readback_bytes == 0


# ---- 2. the framing on the CPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame")
    exe = str(d / "enc_frame_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-strict-aliasing", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "model", "enc_frame_model.cpp"), "-o", exe], check=True)

    def run(bsize, rounds, caps):
        """rounds: [[(kind, size, payload, ...)]]; caps: [(cap, dst alignment)] -> {cap: (rc, produced, crc32)}"""
        blob = bytearray(struct.pack("<II", bsize, len(rounds)))
        for part in rounds:
            blob += struct.pack("<I", len(part))
            for b in part:
                blob += struct.pack("<II", b[0], b[1]) + b[2]
        blob += struct.pack("<I", len(caps))
        for cap, off in caps:
            blob += struct.pack("<QI", cap, off)
        (d / "in.bin").write_bytes(blob)
        out = subprocess.run([exe, str(d / "in.bin")], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        lines = out.stdout.split("\n")
        assert lines[0] == f"batch {E.frame_batch()}"
        res = {}
        for l in lines[1:]:
            if l:
                cap, rc, produced, crc = (int(x) for x in l.split())
                res[cap] = (rc, produced, crc)
        return res
    return run


def _stream(level, csc=None, raw=None, data=None):
    chk, za, _ = soak_gen.checker()
    data = cases.build(E.MIX) if data is None else data
    p = chk.props_init(1 << 20, level)
    if csc:
        p.csc_blocksize = csc
    if raw:
        p.raw_blocksize = raw
    body, sizes, marks = E.writes(chk, za, data, p)
    blks = E.blocks(body, sizes, p.csc_blocksize)
    return body, sizes, E.rounds_of(blks, marks), p.csc_blocksize


def _want(body, sizes, cap):
    rc, pre = E.replay(body, sizes, cap)
    return rc, len(pre), zlib.crc32(pre)


def test_framing_every_cap_of_a_short_stream(model):
    """three chunks with a ragged last one and the flush: four rounds that carry `produced` and `rc`; every cap, every alignment"""
    body, sizes, rounds, bsize = _stream(2, raw=8192, data=cases.build([["text", 1, 0, 20000]])[:17000])
    assert len(rounds) == 4 and all(rounds) and sum(len(r) for r in rounds) == 8 and len(body) < 12000
    caps = [(c, c % 16) for c in range(len(body) + 2)]
    got = model(bsize, rounds, caps)
    bad = [c for c, _ in caps if got[c] != _want(body, sizes, c)]
    assert not bad, (bad[:5], got[bad[0]], _want(body, sizes, bad[0]))
    assert got[len(body)][0] == 0 and got[len(body) - 1][0] == WRITE_ERROR and got[len(body) + 1] == got[len(body)]


@pytest.mark.parametrize("level,csc", [(3, 1024), (2, 4096)])
def test_framing_around_every_write_of_a_longer_stream(model, level, csc):
    """one chunk of more (csc_blocksize 1024) and fewer (4096) blocks than the walk's table holds, and the flush; caps one below,
    at and one above every Write boundary; the alignment of dst moves with the cap"""
    body, sizes, rounds, bsize = _stream(level, csc=csc)
    assert len(rounds) == 2 and len(rounds[1]) == 2
    if csc == 1024:
        assert len(rounds[0]) > E.frame_batch()
    else:
        assert 2 < len(rounds[0]) < E.frame_batch()
    assert E.kinds(rounds[0] + rounds[1], bsize) == {(1, True), (1, False), (0, True), (0, False)}
    want_caps = sorted({max(0, t + d) for t in E.totals(sizes) for d in (-1, 0, 1)} | {0})
    assert len(want_caps) >= 100
    caps = [(c, (c * 7) % 16) for c in want_caps]
    got = model(bsize, rounds, caps)
    bad = [c for c in want_caps if got[c] != _want(body, sizes, c)]
    assert not bad, (bad[:5], got[bad[0]], _want(body, sizes, bad[0]))


# three mistakes a framing can make, restated in Python; each differs from the replay at a cap that is named here, and the
# model agrees with the replay there

def _block_writes(body, sizes, bsize):
    """per block: the sizes of its header Writes ([1] or [1, 3]) and of its payload Write ([n] or [])"""
    return [([1] + ([3] if n != bsize else []), [n] if n else []) for _, n, _, _ in E.blocks(body, sizes, bsize)]


def _wrong_flag_withheld(body, sizes, bsize, cap):
    """the flag byte withheld when the size bytes behind it do not fit (delivering it is RIGHT: it was a Write of its own)"""
    total = 0
    for header, payload in _block_writes(body, sizes, bsize):
        for w in [sum(header)] + payload:
            if total + w > cap:
                return WRITE_ERROR, body[:total]
            total += w
    return 0, body[:total]


def _wrong_partial_payload(body, sizes, bsize, cap):
    """a payload that does not fit delivered as far as it fits"""
    total = 0
    for header, payload in _block_writes(body, sizes, bsize):
        for w in header:
            if total + w > cap:
                return WRITE_ERROR, body[:total]
            total += w
        for w in payload:
            if total + w > cap:
                return WRITE_ERROR, body[:cap]
            total += w
    return 0, body[:total]


def _wrong_goes_on(body, sizes, bsize, cap):
    """a later Write that fits delivered after a refusal"""
    total, out, rc = 0, bytearray(), 0
    for n, t in zip(sizes, E.totals(sizes)):
        if total + n > cap:
            rc = WRITE_ERROR
            continue
        out += body[t - n:t]
        total += n
    return rc, bytes(out)


def test_planted_mistakes_are_caught_at_named_caps(model):
    body, sizes, rounds, bsize = _stream(2, csc=4096)
    tot = [0] + E.totals(sizes)
    # a block with size bytes and a payload of some length: flag, size, payload are Writes k, k + 1, k + 2
    blks = E.blocks(body, sizes, bsize)
    k = next(b[3] for b in blks[3:] if b[1] != bsize and b[1] > 8)
    assert sizes[k:k + 3] == [1, 3, blks[[b[3] for b in blks].index(k)][1]] and k + 3 < len(sizes) and sizes[k + 3] == 1
    named = {"flag fits, size bytes do not": (tot[k] + 2, _wrong_flag_withheld, tot[k] + 1),          # the flag byte IS delivered
             "half the payload fits": (tot[k + 2] + sizes[k + 2] // 2, _wrong_partial_payload, tot[k + 2]),
             "payload refused, the next flag byte would fit": (tot[k + 2] + 1, _wrong_goes_on, tot[k + 2])}
    got = model(bsize, rounds, [(cap, 3 + 2 * i) for i, (cap, _, _) in enumerate(named.values())])
    for what, (cap, wrong, produced) in named.items():
        right = E.replay(body, sizes, cap)
        assert right[0] == WRITE_ERROR and len(right[1]) == produced, what
        assert wrong(body, sizes, bsize, cap) != right, what
        assert got[cap] == (right[0], len(right[1]), zlib.crc32(right[1])), what
        for other in (_wrong_flag_withheld, _wrong_partial_payload, _wrong_goes_on):       # (and each restatement is right elsewhere)
            assert other(body, sizes, bsize, len(body)) == (0, body)
