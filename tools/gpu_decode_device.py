#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the callback decode (CSCMI_DecodeBatch: host in, host out) against the device-resident
decode (CSCMI_DecodeDeviceBatch: streams in HBM, raw bytes in HBM) on three sets of streams of the text stand-in:
    tasks954   the 954 task streams of its first 64 MiB
    8x8MiB     8 streams of 8 MiB each
    1x16MiB    one stream of 16 MiB (also through single-stream CSCDec_Decode)
Each path decodes each set three times, in alternating order; every answer is compared with the input.  Prints, per set and
path, MB/s of raw bytes per repeat, launches and rounds -- the table of profiles/decode_device.md.

    python tools/gpu_decode_device.py [--lib PATH] [--launch-bytes N] [--sets tasks954,8x8MiB,1x16MiB] [--repeats N]
                                      [--paths host,device,single] [--stop-at N]
--stop-at N decodes only the first N raw bytes of every stream on the device path (CSCMI_DecodeDeviceBatchStop; the answer is
compared with that prefix, MB/s are of the bytes delivered); --paths leaves paths out (the table of profiles/archive_device_stop.md
is --paths device --repeats 5, with and without --lib).
--lib names another build of the library (a parent commit's, for the baseline); one without CSCMI_DecodeDeviceBatch is measured on
the callback paths only.  The development build (csc_amd/csrc/build/dev/libcsc_mi355x_timers.so) prints every launch's time on
stderr: that is where the longest launch of profiles/decode_device.md comes from.

The timed region of the callback path includes CSCDec_Create / Destroy of every handle and the Python callbacks; that of the
device path includes decode_device's Python work (one 10-byte read-back per stream for the properties, the job array): both
are what a caller of that path pays, and both are partly harness."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MB = 1 << 20


def encode_batch(lib, datas, level):
    import torch
    from csc_amd.capi import BytesWriter
    L = lib.lib
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.CSCMI_FlushBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    hs, ws, devs = [], [], []
    for d in datas:
        p = lib.props_init(min(64 << 20, len(d)), level)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        assert h
        w.out += lib.write_properties(p)
        hs.append(h); ws.append(w)
        devs.append(torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    n, k, chunk = len(hs), 0, 2 * MB
    H = (C.c_void_p * n)(*hs)
    while True:
        Z = [max(0, min(chunk, len(d) - k * chunk)) for d in datas]
        if not any(Z):
            break
        P = (C.c_void_p * n)(*[t.data_ptr() + k * chunk for t in devs])
        assert L.CSCMI_EncodeDeviceChunkBatch(n, H, P, (C.c_size_t * n)(*Z)) == 0
        k += 1
    assert L.CSCMI_FlushBatch(n, H) == 0
    for h in hs:
        L.CSCEnc_Destroy(h)
    return [bytes(w.out) for w in ws]


def decode_host_batch(lib, streams):
    """CSCDec_Create per stream + ONE CSCMI_DecodeBatch: [(rc, bytes)]"""
    from csc_amd.capi import BytesReader, BytesWriter, CSC_PROP_SIZE
    L = lib.lib
    L.CSCMI_DecodeBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    rs, ws, hs = [], [], []
    for s in streams:
        props = lib.read_properties(s[:CSC_PROP_SIZE])
        r = BytesReader(s[CSC_PROP_SIZE:]); w = BytesWriter()
        h = L.CSCDec_Create(C.byref(props), C.cast(r.ptr(), C.c_void_p), None)
        assert h
        rs.append(r); ws.append(w); hs.append(h)
    n = len(hs)
    R = (C.c_int * n)()
    rc = L.CSCMI_DecodeBatch(n, (C.c_void_p * n)(*hs), (C.c_void_p * n)(*[C.cast(w.ptr(), C.c_void_p) for w in ws]), R)
    for h in hs:
        L.CSCDec_Destroy(h)
    assert rc == 0
    return [(R[i], bytes(ws[i].out)) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--launch-bytes", type=int, default=0)
    ap.add_argument("--sets", default="tasks954,8x8MiB,1x16MiB")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--paths", default="host,device,single")
    ap.add_argument("--stop-at", type=int, default=None)
    a = ap.parse_args()
    import torch
    import csc_amd
    from csc_amd import corpus
    from csc_amd.capi import CscLib
    from csc_amd.device import decode_device
    lib = CscLib(os.path.abspath(a.lib)) if a.lib else csc_amd.load()
    enc = csc_amd.load()                                     # the streams always come from this tree's encoder (the bytes are the reference's)
    has_dev = hasattr(lib.lib, "CSCMI_DecodeDeviceBatch")
    src = corpus.Source("enwik9")
    sets = {}
    if "tasks954" in a.sets:
        whole = src.read(0, 64 * MB).tobytes()
        sets["tasks954"] = [whole[o:o + n] for o, n in corpus.task_slices(64 * MB, 954)]
    if "8x8MiB" in a.sets:
        sets["8x8MiB"] = [src.read(64 * MB + i * 8 * MB, 8 * MB).tobytes() for i in range(8)]
    if "1x16MiB" in a.sets:
        sets["1x16MiB"] = [src.read(128 * MB, 16 * MB).tobytes()]
    print(f"library {lib.path}; device-resident call: {'yes' if has_dev else 'absent'}; launch_bytes {a.launch_bytes or 'default'}", flush=True)
    for name, datas in sets.items():
        streams = encode_batch(enc, datas, 3)
        raw = sum(len(d) for d in datas)
        print(f"== {name}: {len(datas)} streams, {raw} raw bytes, {sum(len(s) for s in streams)} coded", flush=True)
        rows = {"host": [], "device": [], "single": []}
        devs = [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() for s in streams] if has_dev else []
        dsts = [torch.empty(len(d), dtype=torch.uint8, device="cuda") for d in datas] if has_dev else []
        info = ""
        for rep in range(a.repeats):
            for path in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                if path not in a.paths or (path == "device" and not has_dev):
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if path == "host":
                    got = decode_host_batch(lib, streams)
                    dt = time.perf_counter() - t0
                    assert all(rc == 0 and out == d for (rc, out), d in zip(got, datas)), "callback path: wrong bytes"
                else:
                    res, st = decode_device(lib, devs, dsts=dsts, launch_bytes=a.launch_bytes, stop_at=a.stop_at)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    for (rc, t, consumed), d, s in zip(res, datas, streams):
                        want = d if a.stop_at is None else d[:a.stop_at]
                        assert rc == 0 and (consumed == len(s) - 10 or a.stop_at is not None) and bytes(t.cpu().numpy().tobytes()) == want, "device path: wrong bytes"
                    info = f"launches {st.launches} rounds {st.rounds} kernel {st.kernel_ms:.1f} ms"
                    if a.stop_at is not None:
                        info += f"; stopped at {a.stop_at}: {sum(int(t.numel()) for _, t, _ in res)} bytes delivered in {dt * 1e3:.1f} ms"
                rows[path].append((raw if path != "device" or a.stop_at is None else sum(min(a.stop_at, len(d)) for d in datas)) / 1e6 / dt)
            if len(datas) == 1 and "single" in a.paths:
                t0 = time.perf_counter()
                rc, out = lib.decode(streams[0])
                dt = time.perf_counter() - t0
                assert rc == 0 and out == datas[0]
                rows["single"].append(raw / 1e6 / dt)
        for path, label in (("host", "CSCMI_DecodeBatch (host in, host out)"), ("device", "CSCMI_DecodeDeviceBatch (HBM in, HBM out)"),
                            ("single", "CSCDec_Decode, one stream")):
            if rows[path]:
                v = rows[path]
                print(f"{name:9s} {label:42s} MB/s " + " ".join(f"{x:8.2f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:8.2f}  min..max {min(v):.2f}..{max(v):.2f}"
                      + (f"   {info}" if path == "device" else ""), flush=True)


if __name__ == "__main__":
    main()
