"""GPU tier (-m gpu): the randomized soaks as bounded, reproducible tests.  Fixed seeds and fixed case counts (no wall clock),
cases from tests/soak_gen.py (the generator tools/gpu_soak.py and tools/gpu_soak_batch.py run for longer).  Every stream is
compared byte for byte with the checker's (the reference build oracle/_ref when it is there, the oracle otherwise) and decoded
on the device; (rc, bytes) must equal the checker's decoder.  Every failure message carries the seed, the case index and the
spec.  CSCMI_SOAK_SEEDS=a,b,... adds seeds to every test here."""
import ctypes as C
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import soak_gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SINGLE_SEEDS, SINGLE_CASES, SINGLE_CAP = (20261104, 20261106, 20261109), 20, 768 << 10
BATCH_SEEDS, BATCH_ROUNDS, BATCH_BYTES = (20261201, 20261205, 20261209), 3, 6_000_000
RENORM_SEEDS, RENORM_CASES = (20261301, 20261302, 20261303), 3
STAGE_SEEDS = (20261401, 20261402, 20261403)


def single_specs(seed):
    rng = random.Random(seed)
    return [soak_gen.single_case(rng, SINGLE_CAP) for _ in range(SINGLE_CASES)]


def batch_specs(seed):
    rng = random.Random(seed)
    return [soak_gen.batch_round(rng, 900, BATCH_BYTES) for _ in range(BATCH_ROUNDS)]


def renorm_specs(seed):
    rng = random.Random(seed)
    return [soak_gen.renorm_case(rng) for _ in range(RENORM_CASES)]


@pytest.fixture(scope="module")
def chk():
    return soak_gen.checker()


@pytest.fixture(scope="module")
def stage_lib():
    import torch  # noqa: F401  (one HIP runtime per process, see csc_amd.load)
    from csc_amd.capi import CscLib
    lib = CscLib(os.path.join(ROOT, "tests", "stage", "libcsc_stage.so"))
    L = lib.lib
    L.CSCST_SetPos.argtypes = [C.c_void_p, C.c_uint32]
    L.CSCST_SetPos.restype = C.c_int
    L.CSCST_Analyze.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.CSCST_Analyze.restype = C.c_int
    L.CSCST_Filter.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]
    L.CSCST_Filter.restype = C.c_int
    return lib


@pytest.mark.parametrize("seed", soak_gen.seeds(SINGLE_SEEDS))
def test_soak_single(prod, chk, seed):
    lib, za, _ = chk
    for idx, spec in enumerate(single_specs(seed)):
        data = soak_gen.build_input(spec)
        where = soak_gen.describe(seed, idx, spec)
        rc, s = prod.encode(data, props=soak_gen.props_of(prod, spec), max_read=spec["max_read"])
        rc2, want, rcd2, back2 = soak_gen.check_one(lib, za, spec, data)
        assert (rc, s) == (rc2, want), f"stream differs (rc {rc} / {rc2}, {len(s)} / {len(want)} bytes): {where}"
        got = prod.decode(s, max_read=spec["dec_max_read"]) if rc == 0 else (rc, b"")
        assert got == (rcd2, back2), f"device decode differs (rc {got[0]} / {rcd2}): {where}"


@pytest.mark.parametrize("seed", soak_gen.seeds(BATCH_SEEDS))
def test_soak_batch(prod, chk, seed):
    lib, za, _ = chk
    for r, specs in enumerate(batch_specs(seed)):
        datas = [soak_gen.build_input(s) for s in specs]
        got, _ = soak_gen.encode_batch(prod, [soak_gen.props_of(prod, s) for s in specs], datas)
        first = soak_gen.check_one(lib, za, specs[0], datas[0])
        with ThreadPoolExecutor(8) as ex:
            want = [first] + list(ex.map(lambda i: soak_gen.check_one(lib, za, specs[i], datas[i]), range(1, len(specs))))
        bad = [i for i in range(len(specs)) if want[i][0] != 0 or got[i] != want[i][1]]
        assert not bad, f"round {r} ({len(specs)} streams): {len(bad)} streams differ; first: stream {bad[0]} " \
                        f"{soak_gen.describe(seed, r, specs[bad[0]])}"
        dec = soak_gen.decode_batch(prod, got)
        bad = [i for i in range(len(specs)) if dec[i] != (want[i][2], want[i][3])]
        assert not bad, f"round {r} ({len(specs)} streams): {len(bad)} batch decodes differ; first: stream {bad[0]} " \
                        f"{soak_gen.describe(seed, r, specs[bad[0]])}"


@pytest.mark.parametrize("seed", soak_gen.seeds(RENORM_SEEDS))
def test_soak_renormalisation(stage_lib, chk, seed):
    """streams that cross MatchFinder::normalize (csc_mf.cpp:108-114): the position started 0 .. n before 0xFFFFFFF0 on both sides
    (CSCST_SetPos in the stage build; ref_debug_set_pos / orc_debug_set_pos in the checker)"""
    lib, za, is_ref = chk
    set_pos = getattr(lib.lib, "ref_debug_set_pos" if is_ref else "orc_debug_set_pos")
    set_pos.argtypes = [C.c_void_p, C.c_uint32]
    set_pos.restype = None
    for idx, spec in enumerate(renorm_specs(seed)):
        data = soak_gen.build_input(spec)
        where = soak_gen.describe(seed, idx, spec)
        rc, s = stage_lib.encode(data, props=soak_gen.props_of(stage_lib, spec),
                                 after_create=lambda h: stage_lib.lib.CSCST_SetPos(h, spec["pos"]))
        rc2, want, rcd2, back2 = soak_gen.check_one(lib, za, spec, data, set_pos=set_pos)
        assert (rc, s) == (rc2, want), f"stream differs (rc {rc} / {rc2}, {len(s)} / {len(want)} bytes): {where}"
        assert stage_lib.decode(s) == (rcd2, back2), f"device decode differs: {where}"


# ---- the analyzer and the three forward filters on their own, random sizes and shapes ----------------------------------------

FILTER_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 511, 512, 513, 8191, 8192, 8193, 16383, 16384, 16385]


def _e8e9(rng, n):
    """dense E8 / E9 opcodes with operands whose top byte is 00 or FF (the ones Forward_E89 rewrites), some in the last 4 bytes"""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    for j in rng.integers(0, max(1, n), max(1, n // 6)):
        b[j] = 0xE8 + (j & 1)
        if j + 4 < n:
            b[j + 4] = 0xFF if rng.integers(2) else 0x00
    for j in range(max(0, n - 6), n):
        if rng.integers(2):
            b[j] = 0xE8 + (j & 1)
    return b


def _periodic(rng, n, chn):
    """stride-periodic data: chn interleaved channels, each a slow ramp with a little noise"""
    i = np.arange(n)
    base = rng.integers(0, 256, chn)
    step = rng.integers(1, 5, chn)
    v = base[i % chn] + step[i % chn] * (i // chn) + rng.integers(0, 2, n)
    return (v & 0xFF).astype(np.uint8)


def _stage_buffers(seed):
    """(label, bytes) for a seed: the fixed edge sizes, then random sizes up to raw_blocksize"""
    rng = np.random.default_rng(seed)
    sizes = FILTER_SIZES + [int(rng.integers(1, soak_gen.RAW_BLOCKSIZE + 1)) for _ in range(3)]
    out = []
    for k, n in enumerate(sizes):
        shape = ("e8e9", "periodic", "text")[(k + seed) % 3]
        if shape == "e8e9":
            b = _e8e9(rng, n)
        elif shape == "periodic":
            chn = (1, 2, 3, 4, 8)[(k + seed) % 5]
            b = _periodic(rng, n, chn)
            shape += str(chn)
        else:
            b = np.frombuffer(soak_gen.build_input({"parts": [["text", seed, int(rng.integers(0, 1 << 30)), n]]}), dtype=np.uint8).copy()
        out.append((f"{shape}/{n}", b))
    return out


@pytest.mark.parametrize("seed", soak_gen.seeds(STAGE_SEEDS))
def test_stage_filters_and_analyzer(stage_lib, orc, seed):
    """CSCST_Filter (Forward_E89, Foward_Dict, Forward_Delta with 1, 2, 3, 4 and 8 channels) and CSCST_Analyze (7 words per
    8 KiB block, ragged last block included) against the oracle's restatements, on edge and random sizes"""
    from csc_amd.capi import BytesWriter
    L, O = stage_lib.lib, orc.lib
    O.orc_analyze_block.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    O.orc_analyze_block.restype = C.c_uint32
    O.orc_dlt_bpb.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    O.orc_dlt_bpb.restype = C.c_uint32
    O.orc_forward_e89.argtypes = [C.c_void_p, C.c_uint32]
    O.orc_forward_e89.restype = None
    O.orc_forward_dict.argtypes = [C.c_void_p, C.c_uint32]
    O.orc_forward_dict.restype = C.c_uint32
    O.orc_forward_delta.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    O.orc_forward_delta.restype = None
    props = stage_lib.props_init(1 << 20, 3)
    w = BytesWriter()
    h = L.CSCEnc_Create(C.byref(props), C.cast(w.ptr(), C.c_void_p), None)
    assert h
    try:
        res = C.c_uint32(0)
        z = np.zeros(1, dtype=np.uint8)
        assert L.CSCST_Filter(h, 0, z.ctypes.data, 0, 0, C.byref(res)) == -1
        assert L.CSCST_Analyze(h, z.ctypes.data, 0, (C.c_uint32 * 7)()) == -1
        for label, src in _stage_buffers(seed):
            n = len(src)
            where = f"seed {seed} buffer {label}"
            a = src.copy(); a2 = src.copy()
            assert L.CSCST_Filter(h, 0, a.ctypes.data, n, 0, C.byref(res)) == 0
            O.orc_forward_e89(a2.ctypes.data, n)
            assert a.tobytes() == a2.tobytes(), f"Forward_E89 differs: {where}"
            b = src.copy(); b2 = src.copy()
            assert L.CSCST_Filter(h, 1, b.ctypes.data, n, 0, C.byref(res)) == 0
            r2 = O.orc_forward_dict(b2.ctypes.data, n)
            assert res.value == r2, f"Foward_Dict returns {res.value} / {r2}: {where}"
            assert b.tobytes() == b2.tobytes(), f"Foward_Dict output differs: {where}"
            for chn in (1, 2, 3, 4, 8):
                d = src.copy(); d2 = src.copy()
                assert L.CSCST_Filter(h, 2, d.ctypes.data, n, chn, C.byref(res)) == 0
                O.orc_forward_delta(d2.ctypes.data, n, chn)
                assert d.tobytes() == d2.tobytes(), f"Forward_Delta({chn}) differs: {where}"
            nblk = (n + 8191) // 8192
            out = (C.c_uint32 * (7 * nblk))()
            assert L.CSCST_Analyze(h, src.ctypes.data, n, out) == 0
            for blk in range(nblk):
                piece = src[blk * 8192:(blk + 1) * 8192].copy()
                bpb = C.c_uint32(0)
                t = O.orc_analyze_block(piece.ctypes.data, len(piece), C.byref(bpb))
                got = [out[blk * 7 + k] for k in range(7)]
                assert got[0] == t, f"block {blk} type {got[0]:#x} / {t:#x}: {where}"
                if t == 0x1E:                                   # DT_SKIP: every channel's GetDltBpb (the host may need any)
                    assert got[2:] == [O.orc_dlt_bpb(piece.ctypes.data, len(piece), c) for c in (1, 2, 3, 4, 8)], f"block {blk} dlt_bpb: {where}"
                    continue
                assert got[1] == bpb.value, f"block {blk} bpb {got[1]} / {bpb.value}: {where}"
                if 0x10 <= t < 0x15:
                    c = (1, 2, 3, 4, 8)[t - 0x10]
                    assert got[2 + t - 0x10] == O.orc_dlt_bpb(piece.ctypes.data, len(piece), c), f"block {blk} dlt_bpb({c}): {where}"
    finally:
        L.CSCEnc_Destroy(h)
