"""CPU tier for the device-resident decode (CSCMI_DecodeDeviceBatch): the declarations, the export, the refusal without a
device, what the uniformity analysis says about the new kernel entry points, and the block reader (csc_amd/csrc/csc_dec_blocks.h,
the header the kernel's reader is built from) compiled for the host and run against a parse of the framing written here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import cases
import soak_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = [["text", 21, 0, 150000], ["pattern", "00", 40000], ["exe", 22, 0, 60000], ["zeros", 30000]]


def test_header_declares_the_call_in_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "csc_mi355x.h"\n'
                   "int main(void){ CSCMIDevDecode j; CSCMIDevDecodeOpts o; CSCMIDevDecodeStats s; j.rc = CSCMI_NO_DECODER; o.launch_bytes = 0;\n"
                   "  j.props.dict_size = 0; j.src = 0; j.src_size = 0; j.dst = 0; j.dst_cap = 0; j.produced = j.consumed = 0; s.launches = s.rounds = 0; s.kernel_ms = 0;\n"
                   "  return CSCMI_DecodeDeviceBatch(0, &j, &o, &s) + (j.rc == -92 ? 0 : 1) + (int)s.launches; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_library_exports_the_call():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "csc_amd", "libcsc_mi355x.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "CSCMI_DecodeDeviceBatch" in [l.split()[-1] for l in out.splitlines() if l.strip()]


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    from csc_amd import device
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "csc_mi355x.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(CSCMIDevDecode), '
                   "offsetof(CSCMIDevDecode, src), offsetof(CSCMIDevDecode, dst_cap), offsetof(CSCMIDevDecode, consumed), offsetof(CSCMIDevDecode, rc), "
                   "sizeof(CSCMIDevDecodeOpts), sizeof(CSCMIDevDecodeStats)); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = device.CSCMIDevDecode
    assert got == [C.sizeof(D), D.src.offset, D.dst_cap.offset, D.consumed.offset, D.rc.offset,
                   C.sizeof(device.CSCMIDevDecodeOpts), C.sizeof(device.CSCMIDevDecodeStats)]


def test_no_gpu_means_no_device_decode(prod):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from csc_amd import device
    fn = device.bind(prod)
    assert fn(0, None, None, None) == 0                                     # nothing to do is not an error
    dst = (C.c_uint8 * 64)(*([0xA5] * 64))
    jobs = (device.CSCMIDevDecode * 3)()
    for j in jobs:
        j.props = prod.props_init(1 << 20, 3)
        j.src = 0x1000; j.src_size = 100; j.dst = C.addressof(dst); j.dst_cap = 64
        j.rc = 77; j.produced = 5; j.consumed = 6
    stats = device.CSCMIDevDecodeStats()
    assert fn(3, jobs, None, C.byref(stats)) == device.CSCMI_DEVICE_ERROR, "there is no CPU fallback"
    assert [(j.rc, j.produced, j.consumed) for j in jobs] == [(77, 5, 6)] * 3
    assert bytes(dst) == b"\xa5" * 64 and stats.launches == 0 and stats.rounds == 0


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists("/opt/rocm/lib/llvm/bin/opt"),
                    reason="needs hipcc and opt")
def test_new_entry_points_keep_the_bit_chain_scalar():
    """what tests/test_uniformity.py asserts for k_decode_run, for the two device-resident forms; the fast packet loop is shared"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dec_uniformity.py")], capture_output=True, text=True, timeout=900).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"(\S+): (\d+) cycles with a divergent exit(?: \(\d+ outermost\))?, phis divergent/uniform (\d+)/(\d+), divergent terminators (\d+)", line)
        if m:
            res[m.group(1)] = dict(cycles=int(m.group(2)), dphi=int(m.group(3)), uphi=int(m.group(4)), dterm=int(m.group(5)))
    for part in ("k_decode_devEPNS", "k_decode_dev_multiEPK"):
        hits = [v for k, v in res.items() if part in k]
        assert hits, f"no function *{part}* in the analysis output: {sorted(res)}"
        k = hits[0]
        assert k["dphi"] * 3 < k["uphi"], (part, k)
        assert k["cycles"] <= 12, (part, k)
    (fast,) = [v for k, v in res.items() if "dlz_fast" in k]
    assert fast["cycles"] == 0 and fast["dterm"] == 0, fast


# ---- the block reader on the host ----------------------------------------------------------------------------------

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "csc_dec_blocks.h"
// argv: stream file (with its 10 property bytes).  Prints "kind size offset" per block visited (offsets behind the property
// bytes), then "refused <cursor>" or "end <cursor>".  The blocks are walked the way the decoder asks for them at its start --
// an RC block, then a BC block, then alternately.  argv[2]: ring slots per kind (default: rings that never fill); a call's
// blocks are taken from the rings only once the call is over.
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> s;
    int ch;
    while ((ch = fgetc(f)) != EOF) s.push_back((unsigned char)ch);
    fclose(f);
    const uint32_t bsize = ((uint32_t)s[4] << 16) + ((uint32_t)s[5] << 8) + s[6];
    const unsigned char *src = s.data() + 10;
    const uint64_t size = s.size() - 10;
    uint64_t pos = 0;
    uint32_t avail0 = 0, avail1 = 0, want = 1;
    const uint32_t qslots = argc > 2 ? (uint32_t)atoi(argv[2]) : 1u << 30;
    while (pos < size) {
        int rc = cscmi::dec_read_block([&](uint64_t o) { if (o >= size) abort(); return (uint32_t)src[o]; }, size, &pos, bsize, want, qslots,
                                       &avail0, &avail1, avail0, avail1,
                                       [&](const cscmi::DecBlock &b, uint32_t slot) { (void)slot; printf("%u %u %llu\n", b.kind, b.size, (unsigned long long)b.payload); });
        if (rc < 0) { printf("refused %llu\n", (unsigned long long)pos); return 0; }
        want ^= 1;
    }
    printf("end %llu\n", (unsigned long long)pos);
    return 0;
}
"""


def parse(stream, heads=None):
    """the framing, csc_memio.cpp:17-79: [(kind, size, payload offset)], and where the walk was refused (None: the end);
    `heads`, a list, receives the offsets of the blocks' flag bytes"""
    bsize = int.from_bytes(stream[4:7], "big")
    body, p, out = stream[10:], 0, []
    while p < len(body):
        fb, q, n = body[p], p + 1, bsize
        if not fb & 64:
            if len(body) - q < 3:
                return out, p
            n, q = int.from_bytes(body[q:q + 3], "big"), q + 3
        if n == 0 or n > bsize or len(body) - q < n:
            return out, p
        out.append((fb >> 7, n, q))
        if heads is not None:
            heads.append(p)
        p = q + n
    return out, None


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    d = tmp_path_factory.mktemp("blocks")
    (d / "h.cpp").write_text(HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csc_amd", "csrc"), str(d / "h.cpp"), "-o", str(d / "h")], check=True)

    def run(stream, qslots=None):
        (d / "s.bin").write_bytes(stream)
        lines = subprocess.run([str(d / "h"), str(d / "s.bin")] + ([str(qslots)] if qslots else []), capture_output=True, text=True, check=True).stdout.split("\n")
        blocks = [tuple(int(x) for x in l.split()) for l in lines if l and l[0].isdigit()]
        last = [l for l in lines if l and not l[0].isdigit()][0].split()
        return blocks, (int(last[1]) if last[0] == "refused" else None)
    return run


@pytest.fixture(scope="module")
def streams():
    chk, za, _ = soak_gen.checker()
    data = cases.build(MIX)
    out = []
    for level, csc, raw in ((2, 65536, 8192), (2, 4096, 8192), (3, 1024, None)):
        p = chk.props_init(1 << 20, level)
        p.csc_blocksize = csc
        if raw:
            p.raw_blocksize = raw
        rc, s = chk.encode(data, props=p, alloc=za)
        assert rc == 0
        out.append(s)
    return out


def test_block_reader_walks_the_framing(reader, streams):
    counts = []
    for s in streams:
        want, stop = parse(s)
        assert stop is None and want
        assert reader(s) == (want, None)
        counts.append((sum(1 for b in want if b[0] == 1), sum(1 for b in want if b[0] == 0)))
    assert counts == [(36, 36), (43, 36), (76, 13)], counts       # blocks with / without bit 7 (range coder / bit coder), as the reference wrote them


@pytest.mark.parametrize("what", ["zero", "over", "cut_header", "cut_payload"])
def test_block_reader_refuses_where_the_framing_is_broken(reader, streams, what):
    for s in streams:
        heads = []
        blocks, _ = parse(s, heads)
        bsize = int.from_bytes(s[4:7], "big")
        sized = [i for i, b in enumerate(blocks) if b[2] - heads[i] == 4]      # the blocks that carry a size field
        assert len(sized) >= 3
        v = sized[len(sized) // 2]
        victim, at = blocks[v], 10 + heads[v] + 1                          # `at`: its three size bytes
        bad = bytearray(s)
        if what == "zero":
            bad[at:at + 3] = (0).to_bytes(3, "big")
        elif what == "over":
            bad[at:at + 3] = (bsize + 1).to_bytes(3, "big")
        elif what == "cut_header":
            bad = bad[:at + 1]
        else:
            bad = bad[:10 + victim[2] + victim[1] - 1]
        want, stop = parse(bytes(bad))
        assert stop == heads[v] and want == blocks[:v]
        assert reader(bytes(bad)) == (want, stop)


def test_block_reader_refuses_a_full_ring(reader, streams):
    """"ring full" is a refusal: with four slots a kind, the walk stops at the fifth block of one kind that arrives while a
    block of the other kind is being looked for (the level-3 stream has runs of range-coder blocks longer than that)"""
    refused = 0
    for s in streams:
        blocks, _ = parse(s, heads := [])
        want, stop, avail, kind, i = [], None, [0, 0], 1, 0
        while i < len(blocks) and stop is None:
            taken = list(avail)
            while i < len(blocks):
                k = blocks[i][0]
                if avail[k] - taken[k] >= 4:
                    stop = heads[i]
                    break
                want.append(blocks[i]); avail[k] += 1; i += 1
                if k == kind:
                    break
            kind ^= 1
        assert reader(s, 4) == (want, stop)
        refused += stop is not None
    assert refused >= 1
