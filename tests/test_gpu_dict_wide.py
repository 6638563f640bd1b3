"""GPU tier (-m gpu): the dictionary filter that walks several (two) steps of 64 positions a pass, and the 16-byte sub-block copy / LDS
stage (csc_kernels_blocks.inc, csc_kernels.hip).
  * every case of tests/dict_wide_cases.py through the stage entry point (CSCST_Filter, kind 1) against the digest and return
    value the REFERENCE recorded (tests/golden/dict_wide.json);
  * whole encodes against the oracle's stream, for what CSCST_Filter does not reach: the pipeline kernel's own copy of the filter
    and the copy / stage at odd alignments.  300 000 bytes of text under a 64 KiB dictionary (the window wraps, the shortened
    sub-block at its end occurs), fed in pieces of 1, 15, 16, 17, 8 191, 8 193, 16 389 and 40 001 bytes over and over: every later
    chunk's window position is misaligned against the chunk buffer, and sub-blocks start below window position 16 after a wrap."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dict_wide_cases as W
import filter_cases as F
import soak_gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dict_wide.json")))
PIECES = (1, 15, 16, 17, 8191, 8193, 16389, 40001)
TEXT_BYTES, DICT_BYTES = 300_000, 64 << 10


@pytest.fixture(scope="module")
def stage():
    import torch  # noqa: F401  (one HIP runtime per process, see csc_amd.load)
    from csc_amd.capi import CscLib, BytesWriter
    lib = CscLib(os.path.join(ROOT, "tests", "stage", "libcsc_stage.so"))
    L = lib.lib
    L.CSCST_Filter.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]
    L.CSCST_Filter.restype = C.c_int
    props = lib.props_init(1 << 20, 3)
    w = BytesWriter()
    h = L.CSCEnc_Create(C.byref(props), C.cast(w.ptr(), C.c_void_p), None)
    assert h
    yield lib, h
    L.CSCEnc_Destroy(h)


@pytest.fixture(scope="module")
def wide(orc):
    return W.cases(F.words(orc.lib))


@pytest.mark.parametrize("group", ["seam", "esc", "end", "reject", "text"])
def test_filter_kernel_on_the_wide_cases(stage, wide, group):
    lib, h = stage
    mine = {n: d for n, d in wide.items() if n.startswith(group + "/")}
    assert mine
    bad = []
    for name, data in mine.items():
        a = np.frombuffer(data, dtype=np.uint8).copy()
        res = C.c_uint32(0xFFFFFFFF)
        assert lib.lib.CSCST_Filter(h, 1, a.ctypes.data, len(a), 0, C.byref(res)) == 0, name
        if res.value != GOLDEN[name]["dict_ok"]:
            bad.append(f"{name}: returns {res.value}, the reference {GOLDEN[name]['dict_ok']}")
        elif F.digest(a.tobytes()) != GOLDEN[name]["sha256"]:
            bad.append(f"{name}: output differs from the reference's")
        if res.value == 0 and a.tobytes() != data:
            bad.append(f"{name}: rejected, but the buffer came back changed")
    assert not bad, f"{len(bad)} of {len(mine)} cases differ:\n" + "\n".join(bad[:20])


def _pieces(rot, total):
    """the piece sizes, starting at PIECES[rot], that add up to `total`"""
    out, k = [], rot
    while total:
        n = min(total, PIECES[k % len(PIECES)])
        out.append(n)
        total -= n
        k += 1
    return out


def _reader(data, rot):
    """a Read callback that hands out the pieces in turn (every Read becomes one chunk, csc_enc.cpp:170-171)"""
    from csc_amd.capi import BytesReader

    class PieceReader(BytesReader):
        def __init__(self):
            super().__init__(data)
            self.left = _pieces(rot, len(data))

        def _read(self, p, buf, psize):
            self.max_read = self.left.pop(0) if self.left else None
            assert self.max_read is None or self.max_read <= psize[0]
            return super()._read(p, buf, psize)

    return PieceReader()


def _text():
    from csc_amd import corpus
    return corpus.fill("text", corpus.SEED_ENWIK8, 0, TEXT_BYTES).tobytes()


@pytest.mark.parametrize("level,rot", [(3, 0), (3, 3), (3, 6), (1, 0)])
def test_ragged_encodes_match_the_oracle(prod, orc, zalloc, level, rot):
    data = _text()
    rc, got = prod.encode(data, props=prod.props_init(DICT_BYTES, level), reader=_reader(data, rot))
    rc2, want = orc.encode(data, props=orc.props_init(DICT_BYTES, level), alloc=zalloc, reader=_reader(data, rot))
    assert (rc, rc2) == (0, 0)
    assert got == want, f"level {level}, pieces from {PIECES[rot]}: stream differs ({len(got)} / {len(want)} bytes)"
    assert prod.decode(got) == (0, data)


def test_ragged_batch_of_four_matches_the_oracle(prod, orc, zalloc):
    """four such streams advanced together by CSCMI_EncodeDeviceChunkBatch, each with its own piece order"""
    import torch
    from csc_amd.capi import BytesWriter
    L = soak_gen.bind_batch(prod.lib)
    data = _text()
    rots = (0, 2, 4, 6)
    plans = [_pieces(r, len(data)) for r in rots]
    hs, ws = [], []
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    try:
        for _ in rots:
            p = prod.props_init(DICT_BYTES, 3)
            w = BytesWriter()
            h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
            assert h
            w.out += prod.write_properties(p)
            hs.append(h); ws.append(w)
        done = [0] * len(rots)
        for k in range(max(len(p) for p in plans)):
            live = [i for i in range(len(rots)) if k < len(plans[i])]
            H = (C.c_void_p * len(live))(*[hs[i] for i in live])
            P = (C.c_void_p * len(live))(*[dev.data_ptr() + done[i] for i in live])
            Z = (C.c_size_t * len(live))(*[plans[i][k] for i in live])
            assert L.CSCMI_EncodeDeviceChunkBatch(len(live), H, P, Z) == 0, f"round {k}"
            for i in live:
                done[i] += plans[i][k]
        assert done == [len(data)] * len(rots)
        assert L.CSCMI_FlushBatch(len(hs), (C.c_void_p * len(hs))(*hs)) == 0
    finally:
        for h in hs:
            L.CSCEnc_Destroy(h)
    for i, r in enumerate(rots):
        rc, want = orc.encode(data, props=orc.props_init(DICT_BYTES, 3), alloc=zalloc, reader=_reader(data, r))
        assert rc == 0 and bytes(ws[i].out) == want, f"stream {i} (pieces from {PIECES[r]}) differs"
