"""GPU tier (-m gpu): the HIP path through the C ABI against (1) the vectors recorded from the
reference (tests/golden), (2) the oracle on the same seeded inputs, and (3) size-independent
properties on larger inputs (decode(encode(x)) == x, identical output for host- and device-resident
input, chunking invariance).  Bit-exact is the only tolerance: this is byte/integer work."""
import ctypes as C
import json
import os
import subprocess

import pytest

import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
STREAMS = json.load(open(os.path.join(G, "streams.json")))


def test_hip_library_is_the_one_loaded(prod):
    assert prod.lib.CSCMI_DeviceCheck() == 0
    maps = open("/proc/self/maps").read()
    assert "libcsc_mi355x.so" in maps and "libamdhip64" in maps


@pytest.mark.parametrize("key", sorted(STREAMS))
def test_stream_matches_reference_vector(prod, key):
    name, lv = key.split("/m")
    spec, dict_size, clamp, max_read = cases.STREAM_CASES[name]
    data = cases.build(spec)
    want = STREAMS[key]
    rc, s = prod.encode(data, int(lv), dict_size, clamp_dict=clamp, max_read=max_read)
    assert rc == 0
    assert len(s) == want["stream_size"], "HIP stream length differs from the reference"
    assert cases.digest(s) == want["stream_sha256"], "HIP stream bytes differ from the reference"
    if "stream_hex" in want:
        assert s.hex() == want["stream_hex"]
    assert prod.decode(s) == (0, data)


@pytest.mark.parametrize("name", sorted(json.load(open(os.path.join(G, "soak_cases.json")))))
def test_level3_ids_are_looked_after_in_short_windows(prod, name):
    """tests/golden/soak_cases.json (the reference's streams, tools/make_golden_soak_cases.py; found by tools/gpu_soak_batch.py in round 6): long runs of literals
    between two- and three-byte matches -- every DP window ends at its first node or is skipped.  The level-3 form used to drop the re-based ids of its rep
    distances on that way out; 256 positions on the candidate entry behind a live id was recycled and the stream could not be decoded."""
    import hashlib
    gold = json.load(open(os.path.join(G, "soak_cases.json")))[name]
    data = cases.build(gold["spec"])
    assert hashlib.sha256(data).hexdigest() == gold["input_sha256"]
    rc, s = prod.encode(data, props=prod.props_init(gold["dict"], gold["level"]))
    assert rc == 0 and len(s) == gold["stream_bytes"] and hashlib.sha256(s).hexdigest() == gold["stream_sha256"]
    assert prod.decode(s) == (0, data)


def test_a_stream_the_reference_does_not_turn_back_into_its_input_is_reproduced(prod):
    """tests/golden/ref_roundtrip_hazard.json (recorded from the reference, tools/make_golden_ref_roundtrip.py; found by tools/gpu_soak.py): the reference's one-byte
    rep match reads wnd_[wnd_size_], which the decoder never writes, when wnd_curpos_ == rep_dist_[0] (csc_dec.cpp:525-527); under a zeroing allocator its decoder
    turns the reference's own stream for this input into bytes that differ from the input in nine places, with return code 0.  The HIP encoder must write that
    stream and the HIP decoder (window and slack zeroed at Create) must return those bytes -- parity with the reference, not with the input."""
    import hashlib
    gold = json.load(open(os.path.join(G, "ref_roundtrip_hazard.json")))
    data = cases.build(gold["spec"])
    assert hashlib.sha256(data).hexdigest() == gold["input_sha256"]
    rc, s = prod.encode(data, props=prod.props_init(gold["dict"], gold["level"]))
    assert rc == 0 and len(s) == gold["stream_bytes"] and hashlib.sha256(s).hexdigest() == gold["stream_sha256"]
    rcd, back = prod.decode(s)
    assert rcd == gold["decoded_rc"] and hashlib.sha256(back).hexdigest() == gold["decoded_sha256"]
    assert [[i, data[i], back[i]] for i in range(len(data)) if data[i] != back[i]] == gold["decoded_differs_from_input_at"]


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5])
def test_against_oracle_on_fresh_inputs(prod, orc, zalloc, level):
    data = cases.build([["text", 100 + level, 12345, 400000], ["exe", 200 + level, 777, 250000],
                        ["delta", 300 + level, 0, 90000], ["entropy8", 9, 0, 30000], ["random", 8, 0, 20000],
                        ["text", 100 + level, 12345, 60000], ["zeros", 70000], ["random", 8, 0, 20000]])
    a = prod.encode(data, level, 4 << 20)
    b = orc.encode(data, level, 4 << 20, alloc=zalloc)
    assert a == b


def test_custom_props_bt_plus_ht6_and_wide_bucket(prod, orc, zalloc):
    """props the Init function never produces: BT and HT6 together, 16-wide bucket, greedy parser"""
    data = cases.build([["text", 31, 0, 300000], ["exe", 32, 0, 150000]])
    for tweak in ({"hash_width": 4, "hash_bits": 16}, {"hash_width": 16, "lz_mode": 2, "bt_size": 0}, {"lz_mode": 1, "bt_size": 0, "hash_width": 2}):
        p = prod.props_init(1 << 20, 5)
        for k, v in tweak.items():
            setattr(p, k, v)
        q = orc.props_init(1 << 20, 5)
        for k, v in tweak.items():
            setattr(q, k, v)
        assert prod.encode(data, props=p) == orc.encode(data, props=q, alloc=zalloc), tweak


def test_filters_off(prod, orc, zalloc):
    data = cases.build(cases.STREAM_CASES["mix_types"][0])
    for off in (("DLTFilter",), ("EXEFilter", "TXTFilter"), ("DLTFilter", "EXEFilter", "TXTFilter")):
        p = prod.props_init(1 << 20, 3)
        q = orc.props_init(1 << 20, 3)
        for k in off:
            setattr(p, k, 0)
            setattr(q, k, 0)
        assert prod.encode(data, props=p) == orc.encode(data, props=q, alloc=zalloc), off


def test_config2_geometry_roundtrip_and_parity(prod, orc, zalloc):
    """BASELINE configs[1] geometry (-m3 -d64m: 24-bit x 2 HT6, 64 MiB window) on a bounded prefix of the
    enwik9 stand-in; full 10^9 bytes do not fit a test budget, the properties below are size-independent."""
    from csc_amd import corpus
    data = corpus.fill("text", corpus.SEED_ENWIK9, 0, 6 << 20).tobytes()
    p = prod.props_init(64 << 20, 3)
    assert (p.hash_bits, p.hash_width, p.good_len, p.lz_mode) == (24, 2, 16, 3)
    rc, s = prod.encode(data, props=p)
    assert rc == 0 and prod.decode(s) == (0, data)
    assert (rc, s) == orc.encode(data, props=orc.props_init(64 << 20, 3), alloc=zalloc)


def test_config3_geometry_roundtrip_and_parity(prod, orc, zalloc):
    """BASELINE configs[2] geometry (silesia-like 211 957 760 B at -m5 -d256m: binary tree with a 24-bit head and
    78 157 824 nodes, no HT6) on a bounded prefix of the silesia stand-in"""
    data = cases.build([["silesia", 6, 0, 2 << 20], ["silesia", 6, 90 << 20, 1 << 20]])
    p = prod.props_init(min(256 << 20, 211957760), 5)
    assert (p.hash_width, p.bt_hash_bits, p.bt_size, p.bt_cyc, p.good_len, p.lz_mode) == (0, 24, 78157824, 32, 48, 3)
    rc, s = prod.encode(data, props=p)
    assert rc == 0 and prod.decode(s) == (0, data)
    assert (rc, s) == orc.encode(data, props=orc.props_init(min(256 << 20, 211957760), 5), alloc=zalloc)


def test_config5_geometry_roundtrip_and_parity(prod, orc, zalloc):
    """BASELINE configs[4] geometry (10 GB EXE|text|delta mix, -m2 -d1024m -p8: 1 GiB window, 23-bit x 8 HT6, lazy
    parser): two stretches of the mix straddling its 64 MiB segment seams, so that the analyzer switches between
    the e8e9, dictionary and delta paths inside one stream"""
    from csc_amd import corpus
    seg = 64 << 20
    data = (corpus.fill("mix5", corpus.SEED_EXE, seg - (1 << 20), 2 << 20).tobytes()
            + corpus.fill("mix5", corpus.SEED_EXE, 2 * seg - (1 << 20), 2 << 20).tobytes())
    p = prod.props_init(1 << 30, 2)
    assert (p.dict_size, p.hash_bits, p.hash_width, p.good_len, p.lz_mode) == (1 << 30, 23, 8, 24, 2)
    rc, s = prod.encode(data, props=p)
    assert rc == 0 and prod.decode(s) == (0, data)
    assert (rc, s) == orc.encode(data, props=orc.props_init(1 << 30, 2), alloc=zalloc)


@pytest.mark.timeout(600)
def test_level3_long_runs_of_windows_that_end_at_their_first_node(prod, orc, zalloc):
    """8 MiB of the enwik9 stand-in from byte 375 000 000, -m3 -d64m.  Around 6 MiB in there is a stretch where window after
    window of the advanced parser ends at its first node (one long match after the other); the rep distances' mask entries have
    to be moved on to their re-based copies across those windows or they die with the candidate entries they started from
    (csc_kernels_dp4.inc: d5_forward_ids).  Found with bench.py's -p8 tasks 3 and 5; kept as the shortest input that shows it."""
    from csc_amd import corpus
    data = corpus.fill("text", corpus.SEED_ENWIK9, 375000000, 8 << 20).tobytes()
    p = prod.props_init(64 << 20, 3)
    rc, got = prod.encode(data, props=p)
    rc2, want = orc.encode(data, props=p, alloc=zalloc)
    assert rc == 0 and rc2 == 0
    assert got == want


def test_advanced_parser_wavefront_counts(prod, orc, zalloc):
    """The advanced parser of the hash-table levels picks its form by configuration and by how many streams a launch carries: the
    level-3 geometry up to 768 streams the pipeline form (twelve wavefronts a stream, csc_kernels_dp4.inc), everything else -- level 4,
    more streams -- one wavefront a stream (round 6 retired the chain and turn-taking forms that used to serve few level-4 streams).
    Same bytes in every case: batches of 3, 200, 300 and 520 small task streams (mixed text / exe, ragged sizes, some empty)
    against the oracle, at levels 3 and 4."""
    import torch
    from csc_amd import corpus
    from csc_amd.capi import BytesWriter
    L = prod.lib
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    want = {}
    for count, level in ((3, 3), (200, 3), (300, 3), (520, 4), (300, 4), (100, 4)):
        datas = []
        for i in range(count):
            n = 0 if i % 97 == 96 else 9000 + (i * 7919) % 30000
            kind = "exe" if i % 5 == 4 else "text"
            datas.append(corpus.fill(kind, 4000 + i % 11, (i % 13) * 50000, n).tobytes())
        hs, ws, devs = [], [], []
        for d in datas:
            p = prod.props_init(max(len(d), 1), level)
            w = BytesWriter()
            h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
            assert h
            w.out += prod.write_properties(p)
            hs.append(h); ws.append(w)
            devs.append(torch.frombuffer(bytearray(d) if d else bytearray(1), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        live = [i for i, d in enumerate(datas) if d]
        H = (C.c_void_p * len(live))(*[hs[i] for i in live])
        P = (C.c_void_p * len(live))(*[devs[i].data_ptr() for i in live])
        Z = (C.c_size_t * len(live))(*[len(datas[i]) for i in live])
        assert L.CSCMI_EncodeDeviceChunkBatch(len(live), H, P, Z) == 0
        if count in (300, 520):      # every stream's EOF + last blocks in one round trip (streams that never saw a chunk included)
            L.CSCMI_FlushBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            assert L.CSCMI_FlushBatch(len(hs), (C.c_void_p * len(hs))(*hs)) == 0
        for i, h in enumerate(hs):
            if count not in (300, 520):
                assert L.CSCEnc_Encode_Flush(h) == 0
            L.CSCEnc_Destroy(h)
        for i, d in enumerate(datas):
            key = (level, d)
            if key not in want:
                want[key] = orc.encode(d, props=orc.props_init(max(len(d), 1), level), alloc=zalloc)[1]
            assert bytes(ws[i].out) == want[key], (count, level, i)


def test_advanced_parser_one_wavefront_fallbacks(prod, orc, zalloc):
    """Custom props for which the multi-wavefront DP steps aside inside the same kernel: good_len beyond the 64 lengths
    the per-lane price table holds (the one-wavefront form runs while the helper wavefronts idle), and a 9-wide bucket."""
    data = cases.build([["text", 61, 0, 250000], ["exe", 62, 0, 120000], ["text", 61, 40000, 90000]])
    for tweak in ({"good_len": 100}, {"good_len": 65}, {"good_len": 64}, {"hash_width": 9, "hash_bits": 15}, {"hash_width": 1}):
        p = prod.props_init(1 << 20, 3)
        q = orc.props_init(1 << 20, 3)
        for k, v in tweak.items():
            setattr(p, k, v)
            setattr(q, k, v)
        assert prod.encode(data, props=p) == orc.encode(data, props=q, alloc=zalloc), tweak


def test_device_resident_chunks_equal_host_path(prod):
    import torch
    from csc_amd.capi import BytesWriter
    data = cases.build([["text", 5, 0, 5 * 1048576 + 333]])
    L = prod.lib
    L.CSCMI_EncodeDeviceChunk.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    p = prod.props_init(len(data), 3)
    w = BytesWriter()
    h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
    assert h
    w.out += prod.write_properties(p)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for off in range(0, len(data), p.raw_blocksize):
        n = min(p.raw_blocksize, len(data) - off)
        assert L.CSCMI_EncodeDeviceChunk(h, C.c_void_p(dev.data_ptr() + off), n) == 0
    assert L.CSCEnc_Encode_Flush(h) == 0
    L.CSCEnc_Destroy(h)
    assert bytes(w.out) == prod.encode(data, 3, len(data))[1]


def test_callbacks_and_error_codes(prod, orc, zalloc):
    from csc_amd.capi import BytesWriter, BytesReader
    data = cases.build([["text", 3, 0, 300000]])
    seen = []
    rc, s = prod.encode(data, 2, 1 << 20, progress=lambda a, b: seen.append((a, b)))
    assert rc == 0 and seen and seen[-1][0] == len(data) and 0 < seen[-1][1] < len(s)
    # every (in, out) pair is the checker's: GetCompressedSize after each chunk (csc_enc.cpp:180-181), the decoder's after each run (csc_dec.cpp:761-762)
    want = []
    assert orc.encode(data, 2, 1 << 20, alloc=zalloc, progress=lambda a, b: want.append((a, b))) == (0, s) and seen == want
    seen_d, want_d = [], []
    assert prod.decode(s, progress=lambda a, b: seen_d.append((a, b))) == (0, data)
    assert orc.decode(s, alloc=zalloc, progress=lambda a, b: want_d.append((a, b))) == (0, data) and seen_d == want_d and len(want_d) >= 2
    assert prod.encode(data, 2, 1 << 20, writer=BytesWriter(fail_after=5000))[0] == -97       # WRITE_ERROR
    assert prod.encode(data, 2, 1 << 20, reader=BytesReader(data, max_read=100000, fail_at=200000))[0] == -98   # READ_ERROR
    r = BytesReader(data)
    prod.encode(data, 2, 1 << 20, reader=r)
    assert r.calls == [2097152, 2097152]            # exactly one Read of raw_blocksize per chunk + the EOF read


def test_write_call_pattern_matches_memio(prod, orc, zalloc):
    """2-3 Write calls per block, same sizes in the same order as MemIO::WriteBlock (csc_memio.cpp:83-108)"""
    from csc_amd.capi import BytesWriter
    data = cases.build([["text", 3, 0, 700000], ["random", 4, 0, 200000]])
    w1, w2 = BytesWriter(), BytesWriter()
    prod.encode(data, 3, 1 << 20, writer=w1)
    orc.encode(data, 3, 1 << 20, writer=w2, alloc=zalloc)
    assert w1.sizes == w2.sizes and bytes(w1.out) == bytes(w2.out)


def test_abi_from_plain_c(prod, orc, zalloc, tmp_path):
    exe = tmp_path / "abi_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_client.c"),
                    "-o", str(exe), "-L", os.path.join(ROOT, "csc_amd"), "-lcsc_mi355x",
                    "-Wl,-rpath," + os.path.join(ROOT, "csc_amd")], check=True)
    data = cases.build([["text", 3, 0, 500000], ["exe", 4, 0, 200000]])
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.csc"), "3", str(1 << 20), "100000", "0"])
    assert r.returncode == 0
    want = orc.encode(data, 3, 1 << 20, alloc=zalloc, max_read=100000, clamp_dict=False)[1]
    assert (tmp_path / "out.csc").read_bytes() == want
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out2.csc"), "3", str(1 << 20), "0", "30000"])
    assert r.returncode == 10 + 97


def test_two_handles_interleaved(prod):
    """handles are independent (csarc drives up to 8 at once): interleaving chunks of two streams changes nothing"""
    from csc_amd.capi import BytesWriter
    L = prod.lib
    L.CSCMI_EncodeHostChunk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    a = cases.build([["text", 41, 0, 3 * 1048576]])
    b = cases.build([["exe", 42, 0, 3 * 1048576]])
    outs = []
    hs = []
    for d in (a, b):
        p = prod.props_init(len(d), 3)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        w.out += prod.write_properties(p)
        hs.append((h, w, d, p))
    for off in range(0, 3 * 1048576, 2097152):
        for h, w, d, p in hs:
            n = min(2097152, len(d) - off)
            assert L.CSCMI_EncodeHostChunk(h, d[off:off + n], n) == 0
    for h, w, d, p in hs:
        assert L.CSCEnc_Encode_Flush(h) == 0
        L.CSCEnc_Destroy(h)
        outs.append(bytes(w.out))
    assert outs[0] == prod.encode(a, 3, len(a))[1] and outs[1] == prod.encode(b, 3, len(b))[1]


def test_forty_handles_from_eight_threads_share_streams(prod, orc, zalloc):
    """Handles draw their HIP stream from a pool of at most 16 per device (csc_host.cpp, pooled_stream): 40 handles alive at once, driven
    chunk by chunk from 8 threads (csarc's worker count, csarc.cpp:348-351) through the single-handle calls, share streams -- every call
    waits for its own work and may wait for a neighbour's.  Same bytes as the oracle's for every stream; decoders created meanwhile
    draw from the same pool."""
    import threading
    from csc_amd.capi import BytesWriter
    L = prod.lib
    L.CSCMI_EncodeHostChunk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    datas = [cases.build([["exe" if i % 3 == 2 else "text", 700 + i, (i % 5) * 10000, 150000 + 9000 * i]]) for i in range(40)]
    hs = []
    for i, d in enumerate(datas):
        p = prod.props_init(len(d), 1 + i % 5)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        assert h
        w.out += prod.write_properties(p)
        hs.append((h, w))
    errs = []

    def work(t):
        try:
            for i in range(t, 40, 8):
                h, w = hs[i]
                d = datas[i]
                for off in range(0, len(d), 65536 * 3):
                    n = min(65536 * 3, len(d) - off)
                    if L.CSCMI_EncodeHostChunk(h, d[off:off + n], n) != 0:
                        errs.append(("chunk", i))
                if t == 0 and i == 0:
                    rc, raw = prod.decode(orc.encode(datas[1], 3, len(datas[1]), alloc=zalloc)[1])
                    if rc != 0 or raw != datas[1]:
                        errs.append(("decode", i))
        except Exception as ex:       # noqa: BLE001 -- reported below, on the test's thread
            errs.append(("exception", repr(ex)))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in ths: th.start()
    for th in ths: th.join()
    assert not errs, errs
    for i, (h, w) in enumerate(hs):
        assert L.CSCEnc_Encode_Flush(h) == 0
        L.CSCEnc_Destroy(h)
    for i, d in enumerate(datas):
        # chunked by 192 KiB: the stream is CSCEncoder::Compress per chunk, which the oracle reproduces with max_read
        want = orc.encode(d, 1 + i % 5, len(d), alloc=zalloc, max_read=65536 * 3)[1]
        assert bytes(hs[i][1].out) == want, i


def test_batch_of_streams_equals_one_by_one(prod):
    """CSCMI_EncodeDeviceChunkBatch: 12 task streams (a -p12 split incl. a short last slice and an EXE-typed one)
    advanced chunk by chunk with one launch per step == each stream encoded alone."""
    import torch
    from csc_amd import corpus, tasks
    from csc_amd.capi import BytesWriter
    L = prod.lib
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    total = 12 * 2500000 + 777
    sl = tasks.split_single_file(total, 12)
    datas = [corpus.fill("exe" if i == 3 else "text", 900 + i, off, n).tobytes() for i, (off, n) in enumerate(sl)]
    hs, ws, devs = [], [], []
    for d in datas:
        p = prod.props_init(len(d), 3)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        assert h
        w.out += prod.write_properties(p)
        hs.append(h); ws.append(w)
        devs.append(torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    n = len(hs)
    H = (C.c_void_p * n)(*hs)
    for k in range(2):
        Z = [max(0, min(2097152, len(d) - k * 2097152)) for d in datas]
        P = (C.c_void_p * n)(*[t.data_ptr() + k * 2097152 for t in devs])
        assert L.CSCMI_EncodeDeviceChunkBatch(n, H, P, (C.c_size_t * n)(*Z)) == 0
    L.CSCMI_FlushBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    assert L.CSCMI_FlushBatch(n, H) == 0          # == n CSCEnc_Encode_Flush calls
    for h in hs:
        L.CSCEnc_Destroy(h)
    for d, w in zip(datas, ws):
        assert bytes(w.out) == prod.encode(d, 3, len(d))[1]


@pytest.mark.parametrize("level", [3, 2])
def test_batch_with_duplicate_block_checks_equals_oracle(prod, orc, zalloc, level):
    """A batch whose streams hold high-entropy, delta and mixed blocks: every such block needs LZ::IsDuplicateBlock against the
    tables "as of the pending run" (csc_encoder_main.cpp:123-126) -- which every stream's kernel does for itself while it walks its
    chunk (enc_compress_chunk / dev_is_duplicate): ONE launch per chunk for the whole batch, no verdict travels to the host.
    24 streams, different stopping points per stream, two chunks each; every stream == the oracle's."""
    import torch
    from csc_amd.capi import BytesWriter
    L = prod.lib
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    specs = []
    for i in range(24):
        k = i % 6
        if k == 0: spec = [["delta", 300 + i, 0, 700000 + 8192 * i]]
        elif k == 1: spec = [["text", 300 + i, 0, 200000], ["random", 300 + i, 0, 50000], ["text", 300 + i, 0, 200000], ["random", 300 + i, 0, 50000]]   # the second text / random part is a duplicate
        elif k == 2: spec = [["silesia", 300 + i, 0, 2097152 + 100000]]
        elif k == 3: spec = [["entropy8", 300 + i, 0, 150000], ["exe", 300 + i, 0, 300000], ["delta", 300 + i, 0, 100000 + 4096 * i]]
        elif k == 4: spec = [["text", 300 + i, 0, 900000]]
        else: spec = [["random", 300 + i, 0, 40000], ["delta", 300 + i, 0, 60000], ["random", 300 + i, 0, 40000], ["text", 300 + i, 0, 30000 + i]]
        specs.append(spec)
    datas = [cases.build(sp) for sp in specs]
    hs, ws, devs = [], [], []
    for d in datas:
        p = prod.props_init(len(d), level)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        assert h
        w.out += prod.write_properties(p)
        hs.append(h); ws.append(w)
        devs.append(torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    n = len(hs)
    H = (C.c_void_p * n)(*hs)
    for k in range(2):
        Z = [max(0, min(2097152, len(d) - k * 2097152)) for d in datas]
        P = (C.c_void_p * n)(*[t.data_ptr() + k * 2097152 for t in devs])
        assert L.CSCMI_EncodeDeviceChunkBatch(n, H, P, (C.c_size_t * n)(*Z)) == 0
    # the batch's launches are counted on its first handle: one per chunk round, whatever the blocks need
    class St(C.Structure):
        _fields_ = [("chunks", C.c_uint64), ("input_bytes", C.c_uint64), ("output_bytes", C.c_uint64), ("encode_launches", C.c_uint64)] + [("rest", C.c_uint64 * 8)]
    st = St()
    L.CSCMI_GetStats.argtypes = [C.c_void_p, C.c_void_p]
    L.CSCMI_GetStats(hs[0], C.byref(st))
    assert st.encode_launches == 2, st.encode_launches
    for h in hs:
        assert L.CSCEnc_Encode_Flush(h) == 0
        L.CSCEnc_Destroy(h)
    for i, (d, w) in enumerate(zip(datas, ws)):
        rc, want = orc.encode(d, level, len(d), alloc=zalloc)
        assert rc == 0 and bytes(w.out) == want, (i, len(w.out), len(want))


def test_host_segment_variable_is_no_longer_read(prod, orc, zalloc):
    """CSCMI_HOST_SEGMENT=1 once kept CSCEncoder::Compress's block walk on the host (run lists, a launch boundary per
    IsDuplicateBlock verdict: the arrangement of rounds 1-3).  That encoder is gone and the variable is not read: with it set the
    streams are still the oracle's, and a chunk is ONE encode launch.  `dup_blocks` is the case that tells: the analyzer types the
    four blocks of its second `random` part DT_BAD and IsDuplicateBlock turns them into normal ones (as the oracle does: its walk
    was printed once to confirm), which the host walk could only learn between two launches."""
    import subprocess
    import sys
    code = f"""
import ctypes as C, os, sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
import cases, csc_amd
from csc_amd.capi import CscLib, BytesWriter
lib = csc_amd.load()
orc = CscLib(os.path.join({ROOT!r}, "oracle", "liborc.so")); orc.lib.orc_zero_alloc.restype = C.c_void_p; za = orc.lib.orc_zero_alloc()
for name in ("mix_types", "dup_blocks", "delta_200k"):
    spec, d, clamp, _ = cases.STREAM_CASES[name]
    data = cases.build(spec)
    for lv in (2, 3, 5):
        assert lib.encode(data, lv, d, clamp_dict=clamp) == orc.encode(data, lv, d, alloc=za, clamp_dict=clamp), (name, lv)
spec, d, clamp, _ = cases.STREAM_CASES["dup_blocks"]
data = cases.build(spec)
assert len(data) == 146384
L = lib.lib
L.CSCMI_EncodeHostChunk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
L.CSCMI_GetStats.argtypes = [C.c_void_p, C.c_void_p]
p = lib.props_init(min(d, len(data)), 3)
w = BytesWriter()
h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
assert h
w.out += lib.write_properties(p)
assert L.CSCMI_EncodeHostChunk(h, data, len(data)) == 0
class St(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("input_bytes", C.c_uint64), ("output_bytes", C.c_uint64), ("encode_launches", C.c_uint64), ("rest", C.c_uint64 * 8)]
st = St()
L.CSCMI_GetStats(h, C.byref(st))
assert st.encode_launches == st.chunks == 1, (st.encode_launches, st.chunks)
assert L.CSCEnc_Encode_Flush(h) == 0
L.CSCEnc_Destroy(h)
assert bytes(w.out) == orc.encode(data, 3, d, alloc=za, clamp_dict=clamp)[1]
print("HOSTSEG_OK")
"""
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CSCMI_HOST_SEGMENT="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "HOSTSEG_OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


def test_id_guard_holds_with_a_slow_service_wavefront(orc, zalloc):
    """Round 2's review: nothing stopped an equality-mask id from outliving its entry if the service wavefront fell behind.  The
    development build (-DCSCMI_TIMERS, csc_amd/csrc/build/dev) can slow the service wavefront by ~50 k cycles per round: re-based
    masks then arrive dozens of nodes late, the spine's d5_refresh_ids has to WAIT for them (counter > 0), and the stream is
    still the oracle's."""
    import torch  # noqa: F401
    import sys
    dev = os.path.join(ROOT, "csc_amd", "csrc", "build", "dev", "libcsc_mi355x_timers.so")
    # (this is a GPU-tier test: on a GPU box a missing development build is a FAILURE -- __graft_entry__.build() makes it -- not a
    # reason to leave the guard untested)
    assert os.path.exists(dev), "development build missing: make -C csc_amd/csrc dev (part of `make all` / __graft_entry__.build())"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_dp4_guard as G
    from csc_amd import corpus
    from csc_amd.capi import CscLib
    lib = CscLib(dev)
    total_waits = 0
    for data, dsz in ((corpus.fill("text", corpus.SEED_ENWIK9, 0, 1 << 20).tobytes(), 64 << 20),
                      (cases.build(cases.STREAM_CASES["window_wrap_32k"][0]), cases.STREAM_CASES["window_wrap_32k"][1])):
        ok, waits, _ = G.run(lib, orc, zalloc, data, dsz, 1 << 63)
        assert ok
        total_waits += waits
    assert total_waits > 0


# ---- decode path (k_decode_run through CSCDec_*) ----
@pytest.mark.parametrize("name,level", [("mix_types", 3), ("text_300k", 2), ("exe_300k", 5), ("delta_200k", 1),
                                        ("window_wrap_32k", 3), ("periodic_5000x200", 4), ("empty", 3), ("one_byte", 5)])
def test_device_decoder_on_oracle_streams(prod, orc, zalloc, name, level):
    spec, dict_size, clamp, max_read = cases.STREAM_CASES[name]
    data = cases.build(spec)
    rc, s = orc.encode(data, level, dict_size, alloc=zalloc, clamp_dict=clamp, max_read=max_read)
    assert rc == 0
    assert prod.decode(s) == (0, data)
    assert prod.decode(s, alloc=zalloc) == (0, data)                    # custom ISzAlloc
    # MemIO::ReadBlock issues ONE Read per payload and rejects a short one (csc_memio.cpp:47-50): same here
    assert prod.decode(s, max_read=1000) == orc.decode(s, alloc=zalloc, max_read=1000)


@pytest.mark.parametrize("level", [1, 3, 5])
def test_device_decoder_copy_shapes_and_literal_runs(prod, orc, zalloc, level):
    """Round 5: the decoder's packets outside the careful zones run in `dlz_fast` -- copies of up to 64 bytes deferred by a packet
    (buffer instructions, lanes behind the end masked by an out-of-range offset), longer and overlapping ones through d_copy_match,
    runs of literals in a loop of their own.  Data built for exactly these shapes: matches of every length around 64 at every small
    period (overlap: distance < length), matches right behind each other, single literals between matches, long literal runs, and
    enough of it to cross several RC blocks (careful zones at their ends).  Oracle-encoded, device-decoded, byte for byte."""
    import random
    rnd = random.Random(0xC5C0D + level)
    out = bytearray(rnd.randbytes(4096))
    while len(out) < 1_500_000:
        k = rnd.randrange(7)
        if k == 0:                       # an overlapping copy: period 1..70, length around 64
            per, n = rnd.randrange(1, 71), rnd.choice([2, 3, 31, 62, 63, 64, 65, 66, 127, 128, 129, 300])
            seed = out[-per:]
            out += bytes(seed[i % per] for i in range(n))
        elif k in (1, 2):                # a far copy of a length around 64, maybe a second one right behind it
            for _ in range(rnd.randrange(1, 3)):
                n = rnd.choice([2, 3, 4, 17, 60, 63, 64, 65, 70, 143, 144, 145, 400])
                a = rnd.randrange(0, len(out) - n)
                out += out[a:a + n]
        elif k == 3:                     # one literal between two copies
            out.append(rnd.randrange(256))
        elif k == 4:                     # a run of literals (incompressible)
            out += rnd.randbytes(rnd.choice([1, 2, 5, 40, 700, 5000]))
        elif k == 5:                     # text-like: literals under few contexts
            out += bytes(rnd.choice(b"etaoin shrdlu") for _ in range(rnd.randrange(1, 200)))
        else:                            # a repeat of the last distance (rep0) after a literal
            n = rnd.randrange(2, 40)
            d = rnd.randrange(1, 2000)
            out += out[-d:-d + n] if d > n else out[-d:] * (n // d + 1)
    data = bytes(out[:1_500_000])
    rc, s = orc.encode(data, level, 1 << 20, alloc=zalloc)
    assert rc == 0
    assert prod.decode(s) == (0, data)


def test_decoder_error_paths(prod, orc, zalloc):
    from csc_amd.capi import BytesWriter
    data = cases.build(cases.STREAM_CASES["mix_types"][0])
    s = orc.encode(data, 3, 1 << 20, alloc=zalloc)[1]
    rc, out = prod.decode(s, writer=BytesWriter(fail_after=100000))
    assert rc == -97
    rc, out = prod.decode(s, writer=BytesWriter(abort_after=100000))       # CSC_WRITE_ABORT ends silently (csc_dec.cpp:768)
    assert rc == 0 and len(out) < len(data)
    assert prod.decode(s[:10] + b"\x00" * 50)[0] is None                    # garbage after the header: Create fails
    bad = bytearray(s); bad[0] = 0x7F                                       # dict_size > 1 GiB
    assert prod.decode(bytes(bad))[0] is None
    for cut in (len(s) - 3, len(s) // 2):
        assert prod.decode(s[:cut]) == orc.decode(s[:cut], alloc=zalloc)




@pytest.mark.timeout(600)
def test_device_decoder_on_corrupted_streams(prod, orc, zalloc):
    """bit flips and truncation: same return code and same bytes delivered as the oracle (= reference, see
    tests/test_oracle_vs_ref.py::test_corrupted_streams_agree); never a fault or a hang"""
    import random
    data = cases.build(cases.STREAM_CASES["mix_types"][0])
    s = orc.encode(data, 3, 1 << 20, alloc=zalloc)[1]
    rnd = random.Random(11)
    for _ in range(16):
        b = bytearray(s)
        k = rnd.randrange(40, len(b))
        b[k] ^= 1 << rnd.randrange(8)
        want = orc.decode(bytes(b), alloc=zalloc)
        got = prod.decode(bytes(b))
        assert got[0] == want[0] and got[1] == want[1], k
    for cut in (len(s) - 3, len(s) // 2, 70000):
        assert prod.decode(s[:cut]) == orc.decode(s[:cut], alloc=zalloc)


def test_golden_streams_decode_on_device(prod, orc, zalloc):
    """every reference vector small enough to carry its bytes: decode(stream_hex) == input"""
    for key, want in STREAMS.items():
        if "stream_hex" not in want:
            continue
        name = key.split("/m")[0]
        data = cases.build(cases.STREAM_CASES[name][0])
        assert prod.decode(bytes.fromhex(want["stream_hex"])) == (0, data), key


def test_batch_decode_equals_one_by_one(prod, orc, zalloc):
    """CSCMI_DecodeBatch: many handles advanced by one launch per round; per stream the same bytes, the same return
    code and the same Read sizes as CSCDec_Decode alone -- including a damaged and a truncated stream in the batch"""
    import ctypes as C
    from csc_amd.capi import BytesReader, BytesWriter, CSC_PROP_SIZE
    L = prod.lib
    L.CSCMI_DecodeBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.CSCMI_DecodeBatch.restype = C.c_int
    names = ["mix_types", "text_300k", "exe_300k", "delta_200k", "entropy8_100k", "zeros_8k", "one_byte", "empty",
             "window_wrap_32k", "dup_blocks", "random_64k", "abcdefgh_64k"]
    streams = []
    for i, n in enumerate(names):
        spec, dict_size, clamp, max_read = cases.STREAM_CASES[n]
        data = cases.build(spec)
        rc, s = orc.encode(data, (3, 2, 5, 1)[i % 4], dict_size, alloc=zalloc, clamp_dict=clamp, max_read=max_read)
        assert rc == 0
        streams.append(s)
    bad = bytearray(streams[0]); bad[len(bad) // 2] ^= 0x10
    streams.append(bytes(bad))                      # damaged
    streams.append(streams[1][:len(streams[1]) // 2])   # truncated inside the first block
    streams.append(streams[8][:len(streams[8]) - 40000])   # truncated later
    want = [orc.decode(s, alloc=zalloc) for s in streams]
    alone = []
    for s in streams:
        r = BytesReader(s[CSC_PROP_SIZE:])
        alone.append((prod.decode(s), None))
    readers, writers, hs, idx = [], [], [], []
    for i, s in enumerate(streams):
        props = prod.read_properties(s[:CSC_PROP_SIZE])
        r = BytesReader(s[CSC_PROP_SIZE:]); w = BytesWriter()
        h = L.CSCDec_Create(C.byref(props), C.cast(r.ptr(), C.c_void_p), None)
        if not h:                                   # Create already reads two blocks: a stream cut inside them never opens
            assert want[i][0] is None and alone[i][0][0] is None, i
            continue
        readers.append(r); writers.append(w); hs.append(h); idx.append(i)
    n = len(hs)
    assert n >= len(names) + 1
    H = (C.c_void_p * n)(*hs)
    W = (C.c_void_p * n)(*[C.cast(w.ptr(), C.c_void_p) for w in writers])
    R = (C.c_int * n)()
    assert L.CSCMI_DecodeBatch(n, H, W, R) == 0
    for h in hs:
        L.CSCDec_Destroy(h)
    for k, i in enumerate(idx):
        assert (R[k], bytes(writers[k].out)) == want[i] == alone[i][0], i
        # the caller saw exactly the reads a lone CSCDec_Decode makes
        r1 = BytesReader(streams[i][CSC_PROP_SIZE:])
        props = prod.read_properties(streams[i][:CSC_PROP_SIZE])
        h = L.CSCDec_Create(C.byref(props), C.cast(r1.ptr(), C.c_void_p), None)
        L.CSCDec_Decode(h, C.cast(BytesWriter().ptr(), C.c_void_p), None)
        L.CSCDec_Destroy(h)
        assert readers[k].calls == r1.calls, i
