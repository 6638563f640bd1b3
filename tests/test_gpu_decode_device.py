"""GPU tier for the device-resident decode (CSCMI_DecodeDeviceBatch, csc_amd/device.py): streams in device memory decoded to
raw bytes in device memory, block reader and run delivery inside the kernel.

The wanted answer is always the checker's (soak_gen.checker(): the reference build where oracle/_ref has it, the oracle
otherwise) over capi.BytesReader(stream) and capi.BytesWriter(fail_after=cap) -- the host-stream pair the call is specified
against -- with a refused Create (None) mapped to CSCMI_NO_DECODER.  Every test passes explicit destination sizes."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import cases
import soak_gen
import synth_gen as G
from csc_amd.capi import BytesWriter, DECODE_ERROR, WRITE_ERROR
from csc_amd.device import CSCMI_NO_DECODER, decode_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = [["text", 21, 0, 150000], ["pattern", "00", 40000], ["exe", 22, 0, 60000], ["zeros", 30000]]   # tests/test_gpu_pipes.py: 280 000 bytes
_memo = {}


def _chk():
    if "chk" not in _memo:
        _memo["chk"] = soak_gen.checker()
    return _memo["chk"][:2]


def _want(stream, cap):
    chk, za = _chk()
    rc, out = chk.decode(stream, alloc=za, writer=BytesWriter(fail_after=cap))
    return (CSCMI_NO_DECODER if rc is None else rc), out


def _got(res):
    return [(rc, bytes(t.cpu().numpy().tobytes()), consumed) for rc, t, consumed in res]


def _same(got, want, what):
    assert got[0] == want[0] and got[1] == want[1], \
        f"{what}: rc {got[0]} len {len(got[1])}, checker rc {want[0]} len {len(want[1])}, first difference at " \
        f"{next((i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b), min(len(got[1]), len(want[1])))}"


def _mix_stream(level, csc_blocksize, raw_blocksize=None):
    """the 280 000-byte mix encoded by the checker: dictionary 1 MiB, the given block sizes"""
    key = ("mix", level, csc_blocksize, raw_blocksize)
    if key not in _memo:
        chk, za = _chk()
        p = chk.props_init(1 << 20, level)
        p.csc_blocksize = csc_blocksize
        if raw_blocksize:
            p.raw_blocksize = raw_blocksize
        data = cases.build(MIX)
        rc, s = chk.encode(data, props=p, alloc=za)
        assert rc == 0 and len(data) == 280000
        _memo[key] = s
    return _memo[key]


def _small():
    return _mix_stream(2, 4096, 8192)


# ---- 1. synthesized streams ---------------------------------------------------------------------------------------

def _synth_rows(orc):
    if "synth" not in _memo:
        rows = []
        for f in G.FAMILIES:
            if f in ("long_chain", "long_rle"):
                continue
            for s in G.FAMILIES[f]:
                for case in G.cases(orc.lib, f, s):
                    st = G.stream(orc.lib, case)
                    cap = len(case["out"])
                    rows.append((case, st, cap, _want(st, cap)))
        _memo["synth"] = rows
    return _memo["synth"]


@pytest.mark.parametrize("group", [256, 7])
def test_synthesized_streams(prod, orc, group):
    rows = _synth_rows(orc)
    if group != 256:
        rows = [r for r in rows if not r[0]["meta"].get("big")]
    rows = rows[1::2] + rows[0::2]                                # families and refused streams mixed within a call
    assert any(r[3][0] != 0 for r in rows) and any(r[3][0] == 0 for r in rows)
    for a in range(0, len(rows), group):
        part = rows[a:a + group]
        res, _ = decode_device(prod, [st for _, st, _, _ in part], caps=[cap for _, _, cap, _ in part])
        for (case, _, _, want), g in zip(part, _got(res)):
            _same(g, want, f"{group} a call; {G.describe(case)}")


@pytest.mark.parametrize("family", ["long_chain", "long_rle"])
def test_the_documented_refusal(prod, orc, family):
    """a packet of more than kDecUndoCap model bits (include/csc_mi355x.h, LIMIT): DECODE_ERROR, the first run's 100 bytes delivered"""
    case, = G.cases(orc.lib, family, G.FAMILIES[family][0])
    st = G.stream(orc.lib, case)
    (rc, out, _), = _got(decode_device(prod, [st], caps=[len(case["out"])])[0])
    assert rc == DECODE_ERROR and out == case["out"][:100], (rc, len(out))


# ---- 2. many blocks and many runs in one launch -------------------------------------------------------------------

@pytest.mark.parametrize("level,csc,raw", [(2, 65536, 8192), (2, 4096, 8192), (3, 1024, None)])
def test_many_blocks_and_runs_in_one_launch(prod, level, csc, raw):
    st = _mix_stream(level, csc, raw)
    want = _want(st, 280000)
    assert want == (0, cases.build(MIX))
    res, stats = decode_device(prod, [st], caps=[280000], launch_bytes=1 << 30)
    (got,) = _got(res)
    _same(got, want, "one launch")
    assert got[2] == len(st) - 10
    assert stats.launches == 1 and stats.rounds == 1
    res, stats = decode_device(prod, [st], caps=[280000], launch_bytes=8192)
    (got2,) = _got(res)
    _same(got2, want, "launch_bytes 8192")
    assert got2[2] == len(st) - 10
    # a launch returns after the run that brings its output to launch_bytes, and the last one finds the end of the stream: the
    # checker's Write sizes say how many that makes (state carried across every one of them)
    chk, za = _chk()
    w = BytesWriter()
    chk.decode(st, alloc=za, writer=w)
    acc = exits = 0
    for size in w.sizes:
        acc += size
        if acc >= 8192:
            exits, acc = exits + 1, 0
    # (the issue's bound, launches >= 30, is asserted where 30 launches can exist: the two streams with raw_blocksize 8192, 35 runs
    # each; the level-3 stream at the default raw_blocksize has fewer runs than that, and the exact count holds for all three)
    assert stats.launches == exits + 1, (stats.launches, exits)
    if raw == 8192:
        assert stats.launches >= 30, stats.launches


# ---- 3. truncation ------------------------------------------------------------------------------------------------

def test_truncated_streams(prod):
    st = _small()
    cuts = [st[:n] for n in (10, 11, 12, 14, 15, 20, len(st) // 2, len(st) - 1)]
    want = [_want(c, 280000) for c in cuts]
    assert [w[0] for w in want] == [CSCMI_NO_DECODER] * 6 + [-1, -1] and [len(w[1]) for w in want[6:]] == [114688, 278528]
    res, _ = decode_device(prod, cuts, caps=280000)
    for n, g, w in zip((len(c) for c in cuts), _got(res), want):
        _same(g, w, f"cut at {n}")


# ---- 4. destination too small -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [100000, 0, 280000, 279999])
def test_destination_too_small(prod, cap):
    import torch
    st = _small()
    want = _want(st, cap)
    if cap == 100000:
        assert want[0] == WRITE_ERROR and len(want[1]) == 98304
    buf = torch.full((64 + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    res, _ = decode_device(prod, [st], dsts=[buf[64:64 + cap]])
    (got,) = _got(res)
    _same(got, want, f"dst_cap {cap}")
    host = bytes(buf.cpu().numpy().tobytes())
    assert host[:64] == b"\xa5" * 64 and host[64 + cap:] == b"\xa5" * 64, "a guard byte was written"
    assert host[64 + len(want[1]):64 + cap] == b"\xa5" * (cap - len(want[1])), "bytes behind `produced` were written"


# ---- 5. alignment -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_off,dst_off", [(1, 1), (2, 7), (3, 1), (5, 7)])
def test_unaligned_source_and_destination(prod, src_off, dst_off):
    import torch
    st = _small()
    want = _want(st, 280000)
    src = torch.full((src_off + len(st) + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    src[src_off:src_off + len(st)] = torch.frombuffer(bytearray(st), dtype=torch.uint8).cuda()
    dst = torch.zeros(dst_off + 280000 + 64, dtype=torch.uint8, device="cuda")
    res, _ = decode_device(prod, [src[src_off:src_off + len(st)]], dsts=[dst[dst_off:dst_off + 280000]])
    (got,) = _got(res)
    _same(got, want, f"src + {src_off}, dst + {dst_off}")
    assert got[2] == len(st) - 10
    host = bytes(dst.cpu().numpy().tobytes())
    assert host[:dst_off] == bytes(dst_off) and host[dst_off + 280000:] == bytes(64)


# ---- 6. a mixed batch of more streams than CUs ----------------------------------------------------------------------

def _mixed_300():
    if "mixed" not in _memo:
        import test_gpu_forms as F
        chk, za = _chk()
        sizes = [n for n in F.BATCH_SIZES if n <= soak_gen.CHUNK]
        specs = []
        for i in range(297):
            n = sizes[i % len(sizes)]
            specs.append({"parts": [[F._kind(i), 600 + i, i * 7919, n]], "level": 1 + i % 5, "dict": max(n, 1), "props": {}})
        for i, n in enumerate(F.BATCH_SIZES[-2:]):                                # the two that cross a chunk
            specs.insert(100 * (i + 1), {"parts": [["text", 900 + i, 0, n]], "level": 2 + 3 * i, "dict": 1 << 20, "props": {}})
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_roundtrip_hazard.json")))
        specs.insert(250, {"parts": gold["spec"], "level": gold["level"], "dict": gold["dict"], "props": {}})
        assert len(specs) == 300

        def one(spec):
            data = soak_gen.build_input(spec)
            rc, s, rcd, back = soak_gen.check_one(chk, za, spec, data)
            assert rc == 0
            return s, (rcd, back)
        first = one(specs[0])
        with ThreadPoolExecutor(8) as ex:
            _memo["mixed"] = [first] + list(ex.map(one, specs[1:]))
    return _memo["mixed"]


def test_mixed_batch_of_300_streams(prod):
    rows = _mixed_300()
    streams = [s for s, _ in rows]
    caps = [len(w[1]) for _, w in rows]
    res, stats = decode_device(prod, streams, caps=caps)
    got = _got(res)
    host = soak_gen.decode_batch(prod, streams)                      # CSCDec_Decode of the product, through CSCMI_DecodeBatch
    for i, ((s, want), g, h) in enumerate(zip(rows, got, host)):
        _same(g, want, f"stream {i} ({len(s)} bytes) against the checker")
        _same(g, h, f"stream {i} ({len(s)} bytes) against the callback path")
        assert g[2] == len(s) - 10
    assert stats.launches >= 1 and stats.kernel_ms > 0


# ---- 7. nothing to do -----------------------------------------------------------------------------------------------

def test_nothing_to_do(prod):
    res, stats = decode_device(prod, [])
    assert res == [] and stats.launches == 0 and stats.rounds == 0
    st = _small()
    res, stats = decode_device(prod, [st[:10], st], caps=280000)
    got = _got(res)
    assert got[0][0] == CSCMI_NO_DECODER and got[0][1] == b""        # src_size == 0
    _same(got[1], _want(st, 280000), "the stream next to an empty one")
