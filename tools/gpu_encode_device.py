#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the batch encode with host writers (CSCMI_EncodeDeviceChunkBatch + CSCMI_FlushBatch:
inputs in HBM, every coder block read back and handed to a Write callback) against the device-resident encode
(CSCMI_EncodeDeviceBatch: inputs in HBM, streams in HBM) on three sets of level-3 task streams of the text stand-in:
    large8     8 streams of 8 MiB each
    tasks127   the 127 task streams of its first 64 MiB
    tasks954   the 954 task streams of its first 64 MiB
Each path encodes each set three times, in alternating order; every stream of one path is compared with the other path's.
Prints, per set and path, MB/s of raw bytes over wall time per repeat, the median and the spread, and for the device-resident
path readback_bytes, rounds, launches, kernel_ms and the framing kernel's share of it -- the table of profiles/encode_device.md.

    python tools/gpu_encode_device.py [--lib PATH] [--sets large8,tasks127,tasks954] [--repeats 3]
--lib names the build of the library that runs the host-writer path (the PARENT commit's, for the baseline); without it that
path runs on this tree's library, which says what the drain costs but is not the acceptance comparison.

The timed region of the host-writer path includes CSCEnc_Create / Destroy of every handle and the Python Write callbacks; that
of the device-resident path includes encode_device's Python work (the job array, one allocation for all destinations, the
upload of the property bytes): both are what a caller of that path pays, and both are partly harness.  The framing share comes
from the line the library prints on stderr under CSCMI_BATCH_TRACE (HIP events around the k_frame_blocks launches)."""
import argparse
import ctypes as C
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MB = 1 << 20
LEVEL = 3


def encode_host_writers(lib, datas, devs):
    from csc_amd.capi import BytesWriter
    L = lib.lib
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.CSCMI_FlushBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    hs, ws = [], []
    for d in datas:
        p = lib.props_init(min(64 << 20, len(d)), LEVEL)
        w = BytesWriter()
        h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
        assert h
        w.out += lib.write_properties(p)
        hs.append(h); ws.append(w)
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


class Stderr:
    """what the process writes to fd 2 while the block runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sets", default="large8,tasks127,tasks954")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    os.environ["CSCMI_BATCH_TRACE"] = "1"            # (both libraries read it at their first batch call: one short line per call, both paths)
    import torch
    import csc_amd
    from csc_amd import corpus
    from csc_amd.capi import CscLib
    from csc_amd.device import encode_device
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    new = csc_amd.load()
    old = CscLib(os.path.abspath(a.lib)) if a.lib else new
    src = corpus.Source("enwik9")
    whole = src.read(0, 64 * MB).tobytes()
    sets = {}
    if "large8" in a.sets:
        sets["large8"] = [whole[i * 8 * MB:(i + 1) * 8 * MB] for i in range(8)]
    if "tasks127" in a.sets:
        sets["tasks127"] = [whole[o:o + n] for o, n in corpus.task_slices(64 * MB, 127)]
    if "tasks954" in a.sets:
        sets["tasks954"] = [whole[o:o + n] for o, n in corpus.task_slices(64 * MB, 954)]
    print(f"host-writer path: {old.path}{'' if a.lib else ' (THIS tree: not the acceptance comparison)'}; device-resident path: {new.path}", flush=True)
    verdicts = []
    for name, datas in sets.items():
        raw = sum(len(d) for d in datas)
        devs = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
        props = [new.props_init(min(64 << 20, len(d)), LEVEL) for d in datas]
        torch.cuda.synchronize()
        rows = {"host": [], "device": []}
        info, ref = "", None
        for rep in range(a.repeats):
            for path in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if path == "host":
                    with Stderr():
                        got = encode_host_writers(old, datas, devs)
                    dt = time.perf_counter() - t0
                else:
                    with Stderr() as err:
                        res, st = encode_device(new, devs, props=props)
                        torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert all(rc == 0 for rc, _ in res), "device-resident path: a stream did not fit or failed"
                    got = [bytes(t.cpu().numpy().tobytes()) for _, t in res]
                    m = re.search(r"kernels ([\d.]+) ms of which framing ([\d.]+) ms", err.text)
                    share = f"{float(m.group(2)):.3f} ms = {100 * float(m.group(2)) / max(float(m.group(1)), 1e-9):.3f} %" if m else "not printed"
                    info = f"readback {st.readback_bytes} B rounds {st.rounds} launches {st.launches} kernel {st.kernel_ms:.1f} ms framing {share}"
                if ref is None:
                    ref = got
                assert got == ref, f"{name}: the {path} path's streams differ from the other path's"
                rows[path].append(raw / 1e6 / dt)
        print(f"== {name}: {len(datas)} streams, {raw} raw bytes, {sum(len(s) for s in ref)} coded", flush=True)
        for path, label in (("host", "ChunkBatch + FlushBatch, host writers"), ("device", "CSCMI_EncodeDeviceBatch (HBM in, HBM out)")):
            v = rows[path]
            print(f"{name:9s} {label:42s} MB/s " + " ".join(f"{x:8.2f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:8.2f}  spread {max(v) - min(v):.2f}"
                  + (f"   {info}" if path == "device" else ""), flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
        spread = max(max(v) - min(v) for v in rows.values())
        ok = med["device"] >= med["host"] - spread
        verdicts.append(ok)
        print(f"{name:9s} device-resident median {med['device']:.2f} vs host-writer median {med['host']:.2f} MB/s, larger spread {spread:.2f}: "
              f"{'not slower beyond the spread' if ok else 'SLOWER beyond the spread'}", flush=True)
    print("acceptance (no set slower than the host-writer path by more than the larger spread): " + ("met" if all(verdicts) else "NOT met")
          + ("" if a.lib else " -- against this tree's own library, not the parent's"), flush=True)


if __name__ == "__main__":
    main()
