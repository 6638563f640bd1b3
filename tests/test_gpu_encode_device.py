"""GPU tier for the device-resident encode (CSCMI_EncodeDeviceBatch, csc_amd/device.py): raw bytes in device memory encoded to
streams in device memory, the coder blocks framed by k_frame_blocks.

The wanted answer is always the checker's (soak_gen.checker(): the reference build where oracle/_ref has it, the oracle
otherwise): the whole stream behind its property bytes, and for a capped run the longest run of whole Write calls of the
checker's unlimited run whose total is <= cap (enc_device_cases.replay)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import pytest

import cases
import enc_device_cases as E
import soak_gen
from csc_amd.capi import WRITE_ERROR
from csc_amd.device import CSCMI_NO_ENCODER, decode_device, encode_device

pytestmark = pytest.mark.gpu
_memo = {}
STATUS_BYTES = 16                       # FrameStatus {error, rc, produced}: include/csc_mi355x.h, csc_amd/csrc/csc_enc_frame.h


def _chk():
    if "chk" not in _memo:
        _memo["chk"] = soak_gen.checker()
    return _memo["chk"][:2]


def _props(lib, level, dict_size, **over):
    p = lib.props_init(dict_size, level)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _want(data, level, dict_size, **over):
    """(body, Write sizes, chunk marks) of the checker for this input and these props"""
    key = (data, level, dict_size, tuple(sorted(over.items())))
    if key not in _memo:
        chk, za = _chk()
        _memo[key] = E.writes(chk, za, data, _props(chk, level, dict_size, **over))
    return _memo[key]


def _bytes(t):
    return bytes(t.cpu().numpy().tobytes())


def _text(n, seed=31):
    return cases.build([["text", seed, 0, n]]) if n else b""


def _mix():
    return cases.build(E.MIX)


def _same(rc, got, want_rc, want, what):
    assert rc == want_rc and got == want, \
        f"{what}: rc {rc} len {len(got)}, checker rc {want_rc} len {len(want)}, first difference at " \
        f"{next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))}"


# ---- 3. every form ----------------------------------------------------------------------------------------------------

def _form_rows():
    import test_gpu_forms as F
    return list(F.FORMS)


@pytest.mark.parametrize("row", _form_rows())
def test_every_form(prod, row):
    import test_gpu_forms as F
    level, over = F.FORMS[row]["variants"][0]
    mix = _mix()
    inputs = [(b"", {}), (_text(1), {}), (_text(2), {}), (mix[140000:140000 + 24576], {}), (_text(24576, 32), {}),
              (_text(20000, 33), {"raw_blocksize": 8192})]                       # the last: three chunks, the third ragged
    props, wants = [], []
    for data, extra in inputs:
        o = dict(over, **extra)
        props.append(_props(prod, level, max(len(data), 1), **o))
        wants.append(_want(data, level, max(len(data), 1), **o)[0])
    res, stats = encode_device(prod, [d for d, _ in inputs], props=props)
    for (data, _), (rc, t), want, p in zip(inputs, res, wants, props):
        got = _bytes(t)
        assert got[:10] == prod.write_properties(p)
        _same(rc, got[10:], 0, want, f"{row}, {len(data)} bytes")
    assert stats.rounds == 3 + 1


# ---- 4. all four header kinds, more and fewer blocks than the walk's table ---------------------------------------------

@pytest.mark.parametrize("level,csc", [(2, 1024), (3, 1024), (2, 4096), (3, 4096)])
def test_all_four_header_kinds(prod, level, csc):
    data = _mix()
    assert len(data) == 280000
    body, sizes, marks = _want(data, level, 1 << 20, csc_blocksize=csc)
    rounds = E.rounds_of(E.blocks(body, sizes, csc), marks)
    # before anything runs on the device: the reference alone says that this case has every kind of header, and that one chunk
    # finishes more (1024) / fewer (4096) blocks than k_frame_blocks takes at a time
    assert E.kinds(rounds[0] + rounds[1], csc) == {(1, True), (0, True), (1, False), (0, False)}
    assert len(rounds) == 2 and len(rounds[1]) == 2
    if csc == 1024:
        assert len(rounds[0]) > E.frame_batch(), len(rounds[0])
    else:
        assert 2 < len(rounds[0]) < E.frame_batch(), len(rounds[0])
    res, stats = encode_device(prod, [data], props=_props(prod, level, 1 << 20, csc_blocksize=csc))
    (rc, t), = res
    _same(rc, _bytes(t)[10:], 0, body, f"level {level}, csc_blocksize {csc}")
    assert stats.rounds == 2 and stats.readback_bytes == 2 * STATUS_BYTES


# ---- 5. alignment and bounds ------------------------------------------------------------------------------------------

def _stream5():
    data = _mix()[140000:140000 + 24576]
    return data, _want(data, 2, len(data))


def test_alignment_and_bounds(prod):
    import torch
    data, (body, sizes, _) = _stream5()
    p = _props(prod, 2, len(data))
    n = len(body)
    srcs, dsts, bufs = [], [], []
    for off in range(16):
        s = torch.full((64 + len(data) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        so = 64 + off % 4
        s[so:so + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        d = torch.full((64 + 16 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
        srcs.append(s[so:so + len(data)]); dsts.append(d[64 + off:64 + off + n]); bufs.append(d)
    res, _ = encode_device(prod, srcs, props=p, dsts=dsts)
    for off, ((rc, t), d) in enumerate(zip(res, bufs)):
        host = _bytes(d)
        _same(rc, _bytes(t), 0, body, f"dst + {off}, src + {off % 4}")
        assert host[64 + off:64 + off + n] == body
        assert host[:64 + off] == b"\xa5" * (64 + off) and host[64 + off + n:] == b"\xa5" * (len(host) - 64 - off - n), f"dst + {off}: a guard byte was written"


# ---- 6. caps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["level2_24k", "csc1024"])
def test_caps(prod, which):
    import torch
    if which == "level2_24k":
        data, (body, sizes, marks) = _stream5()
        p = _props(prod, 2, len(data))
    else:
        data = _mix()[100000:160000]
        body, sizes, marks = _want(data, 3, len(data), csc_blocksize=1024)
        p = _props(prod, 3, len(data), csc_blocksize=1024)
    blks = E.blocks(body, sizes, p.csc_blocksize)
    tot = E.totals(sizes)
    picked = [blks[0], blks[len(blks) // 2], blks[-2], blks[-1]]                 # first, a middle one, the two of the flush
    assert blks[-2][3] >= marks[-1]
    ts = set()
    for b in picked:                                                            # the totals after each Write of the block
        ts.update(tot[b[3]:b[3] + 1 + (b[1] != p.csc_blocksize) + (b[1] > 0)])
    caps = sorted({max(0, t + d) for t in ts for d in (-1, 0, 1)} | {0, len(body) - 1, len(body)})
    assert len(caps) >= 20
    bufs = [torch.full((32 + len(body) + 32,), 0xA5, dtype=torch.uint8, device="cuda") for _ in caps]
    res, _ = encode_device(prod, [data] * len(caps), props=p, dsts=[b[32:32 + c] for b, c in zip(bufs, caps)])   # ONE call, one job per cap
    for cap, (rc, t), buf in zip(caps, res, bufs):
        want_rc, want = E.replay(body, sizes, cap)
        assert want_rc == (WRITE_ERROR if cap < len(body) else 0)
        _same(rc, _bytes(t), want_rc, want, f"cap {cap}")
        host = _bytes(buf)
        assert host[32:32 + len(want)] == want
        assert host[:32] == b"\xa5" * 32 and host[32 + len(want):] == b"\xa5" * (len(host) - 32 - len(want)), f"cap {cap}: bytes at or beyond `produced` were written"


# ---- 7. a mixed batch -------------------------------------------------------------------------------------------------

def _mixed_40():
    if "mixed" not in _memo:
        sizes = [0, 1, 2, 3, 255, 256, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 12000, 16384, 20000, 24576]
        kinds = ("text", "exe", "delta", "entropy8", "random", "silesia")
        custom = [(3, {"hash_width": 1, "hash_bits": 16, "good_len": 8}), (2, {"hash_width": 9, "lz_mode": 1})]
        jobs = []
        for i in range(36):
            n = sizes[i % len(sizes)]
            level, over = (1 + i % 5, {}) if i % 7 < 5 else custom[i % 2]
            jobs.append((cases.build([[kinds[i % 6], 800 + i, i * 7919, n]]) if n else b"", level, dict(over)))
        for i, n in enumerate((17000, 24576)):                                   # two that cross a chunk: 3 chunks
            jobs.insert(10 * (i + 1), (_text(n, 40 + i), 2 + i, {"raw_blocksize": 8192}))
        jobs.insert(5, (_text(5000, 50), 3, {"lz_mode": 0}))                     # CSCEnc_Create refuses these two
        jobs.insert(25, (_text(5000, 51), 2, {"csc_blocksize": 0}))
        assert len(jobs) == 40
        _memo["mixed"] = jobs
    return _memo["mixed"]


def test_mixed_batch(prod):
    jobs = _mixed_40()
    refused = [i for i, (_, _, o) in enumerate(jobs) if o.get("lz_mode") == 0 or o.get("csc_blocksize") == 0]
    assert refused == [5, 25]
    props = [_props(prod, lv, max(len(d), 1), **o) for d, lv, o in jobs]
    res, stats = encode_device(prod, [d for d, _, _ in jobs], props=props)
    got = [(rc, _bytes(t)[10:]) for rc, t in res]
    for i, ((d, lv, o), g) in enumerate(zip(jobs, got)):
        if i in refused:
            assert g == (CSCMI_NO_ENCODER, b""), (i, g[0], len(g[1]))
            continue
        want = _want(d, lv, max(len(d), 1), **o)[0]
        _same(g[0], g[1], 0, want, f"job {i} ({len(d)} bytes, level {lv}, {o}) in the batch")
    crossing = [i for i, (d, _, o) in enumerate(jobs) if o.get("raw_blocksize") and len(d) > o["raw_blocksize"]]
    assert len(crossing) == 2
    for i in range(len(jobs)):                                                   # every job the call did not refuse, alone
        if i in refused:
            continue
        (rc, t), = encode_device(prod, [jobs[i][0]], props=props[i])[0]
        assert (rc, _bytes(t)[10:]) == got[i], f"job {i} alone differs from the batch"
    chunks = max(-(-len(d) // p.raw_blocksize) for k, ((d, _, _), p) in enumerate(zip(jobs, props)) if k not in refused)
    assert chunks == 3 and stats.rounds == chunks + 1
    assert 0 < stats.readback_bytes <= STATUS_BYTES * len(jobs) * stats.rounds       # the status array and nothing else
    assert stats.launches >= stats.rounds and stats.kernel_ms > 0


# ---- 8. state reuse -----------------------------------------------------------------------------------------------------

def test_state_reuse(prod):
    a, b = _mix()[:24576], _mix()[200000:224576]
    for data in (a, b, a):                                                       # the second and third call get cached slabs
        (rc, t), = encode_device(prod, [data], level=2)[0]
        _same(rc, _bytes(t)[10:], 0, _want(data, 2, len(data))[0], "a call after another")
    # and the slabs this call left in the cache serve the callback paths
    rc, s = prod.encode(b, 2)
    _same(rc, s[10:], 0, _want(b, 2, len(b))[0], "CSCEnc_Encode after the device-resident call")
    (s2, s3), _ = soak_gen.encode_batch(prod, [prod.props_init(len(b), 2), prod.props_init(len(a), 2)], [b, a])
    assert s2[10:] == _want(b, 2, len(b))[0] and s3[10:] == _want(a, 2, len(a))[0], "CSCMI_EncodeDeviceChunkBatch + CSCMI_FlushBatch after it"
    (rc, t), = encode_device(prod, [b], level=2)[0]
    _same(rc, _bytes(t)[10:], 0, _want(b, 2, len(b))[0], "the device-resident call after the callback paths")


# ---- 9. round trip without leaving the device -----------------------------------------------------------------------------

def test_round_trip_on_the_device(prod):
    import torch
    data = _mix()
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    enc, _ = encode_device(prod, [src] * 3, props=[_props(prod, lv, 1 << 20) for lv in (2, 3, 5)])
    assert [rc for rc, _ in enc] == [0, 0, 0]
    dec, _ = decode_device(prod, [t for _, t in enc], caps=len(data))             # the tensors encode_device returned, in place
    for lv, (rc, t, consumed), (_, s) in zip((2, 3, 5), dec, enc):
        assert rc == 0 and consumed == int(s.numel()) - 10 and int(t.numel()) == len(data), (lv, rc)
        assert bool(torch.equal(t, src)), f"level {lv}: the round trip differs from the input"      # the only comparison; one flag crosses the bus


# ---- 10. threads ----------------------------------------------------------------------------------------------------------

def test_two_threads(prod):
    import torch
    sets = []
    for k in range(2):
        sets.append([(cases.build([[("text", "exe", "delta", "silesia")[i % 4], 900 + 10 * k + i, i * 1000, 3000 + 2500 * i]]), 1 + (i + k) % 5) for i in range(8)])
    wants = [[_want(d, lv, len(d))[0] for d, lv in s] for s in sets]                 # (the checker, on this thread)
    dev = torch.cuda.current_device()

    def run(s):
        torch.cuda.set_device(dev)
        res, _ = encode_device(prod, [d for d, _ in s], props=[_props(prod, lv, len(d)) for d, lv in s])
        return [(rc, _bytes(t)[10:]) for rc, t in res]
    with ThreadPoolExecutor(2) as ex:
        got = list(ex.map(run, sets))
    for k in range(2):
        for i, (g, w) in enumerate(zip(got[k], wants[k])):
            _same(g[0], g[1], 0, w, f"thread {k}, job {i}")


def test_nothing_to_do(prod):
    res, stats = encode_device(prod, [])
    assert res == [] and stats.launches == 0 and stats.rounds == 0 and stats.readback_bytes == 0
