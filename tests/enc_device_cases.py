"""What the tests of the device-resident encode (tests/test_encode_device_host.py, tests/test_gpu_encode_device.py) share: the
checker's Write-call sequence for an input, its replay under a capacity, and its blocks.  A plain module, like `cases`.

The wanted answer of a capped run is NOT capi.encode(writer=BytesWriter(fail_after=cap)): that helper calls Encode_Flush even
after Encode failed, and a small later Write may then fit.  It is the longest run of whole Write calls whose total is <= cap."""
import os
import re

from csc_amd.capi import WRITE_ERROR, BytesWriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = [["text", 21, 0, 150000], ["pattern", "00", 40000], ["exe", 22, 0, 60000], ["zeros", 30000]]   # tests/test_gpu_decode_device.py: 280 000 bytes


def frame_batch():
    """kFrameBatch of csc_amd/csrc/csc_enc_frame.h"""
    src = open(os.path.join(ROOT, "csc_amd", "csrc", "csc_enc_frame.h")).read()
    return int(re.search(r"constexpr uint32_t kFrameBatch = (\d+);", src).group(1))


def writes(chk, za, data, props):
    """the checker's stream behind its 10 property bytes, the sizes of its Write calls, and how many of them had been made
    when each chunk was done (the Progress callback comes after every chunk; the calls behind the last mark are Encode_Flush's)"""
    w = BytesWriter()
    marks = []
    rc, s = chk.encode(data, props=props, alloc=za, writer=w, progress=lambda a, b: marks.append(len(w.sizes)))
    assert rc == 0 and sum(w.sizes) == len(s) - 10
    marks = sorted(set(m for m in marks if m))
    return s[10:], list(w.sizes), marks


def replay(body, sizes, cap):
    """(rc, prefix): the Write calls accepted while the total stays <= cap; the first refused one ends the stream"""
    total = 0
    for n in sizes:
        if total + n > cap:
            return WRITE_ERROR, body[:total]
        total += n
    return 0, body[:total]


def totals(sizes):
    out, t = [], 0
    for n in sizes:
        t += n
        out.append(t)
    return out


def blocks(body, sizes, bsize):
    """[(kind, size, payload, index of its flag-byte Write)] from the Write sequence: 1 byte, [3 bytes], [payload]"""
    out, i, p = [], 0, 0
    while i < len(sizes):
        first = i
        assert sizes[i] == 1
        fb = body[p]
        i, p, n = i + 1, p + 1, bsize
        if not fb & 64:
            assert sizes[i] == 3
            n = int.from_bytes(body[p:p + 3], "big")
            i, p = i + 1, p + 3
        if n:
            assert sizes[i] == n
            i += 1
        out.append((fb >> 7, n, body[p:p + n], first))
        p += n
    assert p == len(body)
    return out


def rounds_of(blks, marks):
    """the blocks of each chunk and, last, of the flush: what one round of encode kernels leaves in a stream's arena"""
    out, a = [], 0
    for m in marks + [None]:
        part = [b for b in blks[a:] if m is None or b[3] < m]
        out.append(part)
        a += len(part)
    return out


def kinds(blks, bsize):
    """the header kinds present: (range coder?, full?)"""
    return {(b[0], b[1] == bsize) for b in blks}
