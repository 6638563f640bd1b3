#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): reading a `.csa` through the callback path from a tmpfs file (CSA_Test / CSA_Extract:
pread, CSCMI_DecodeBatch with host callbacks, adler32 on the CPU, pwrite -- untouched by the device-resident read, so it is the
parent commit's path) against the device-resident read of the same bytes uploaded once (DeviceArchive.test / .extract:
k_gather_extents, CSCMI_DecodeDeviceBatch, k_frag_pieces, k_frag_fold), on two archives written by `csa.add`:
    many_files   the 80-file tree of tests/csa_cases.py (level 1, 256 KiB dictionary)
    tree_small   the 256-file tree of `bench.py --workload tree_small` (level 3, 64 MiB dictionary)
Each path reads each archive `--repeats` times after one warm-up, the two paths alternating; every file the device path delivers
is compared with the tree's content.  Per archive and path: wall seconds per call (median, min, max) and MB/s of raw bytes over the
median; for the device path also waves, launches, decode launches, read-back bytes, and the three kernels' HIP-event time with
the bytes each moved (gather: the bytes of streams of more than one archive block plus 10 per task; pieces: raw bytes loaded,
and stored again by extract).  Writes profiles/archive_device.md.

    python tools/gpu_archive_device.py [--repeats 5] [--out profiles/archive_device.md]
    python tools/gpu_archive_device.py --stop-early [--select NAME...] [--repeats 5] [--out FILE]

--stop-early measures something else: a SELECTION read by DeviceArchive.extract with and without stop_early (CSAMI_DeviceRead against
CSAMI_DeviceReadStop, same handle, same session, alternating), on three archives: `one_ext` (24 files of 1 MiB with one extension:
one large task), `tree_small`, and `split4` (one 16 MiB file written with split_count=4).  The selection is --select, or else the
file that lies first in the archive's largest task.  Per archive: wall seconds per call of either, decoded_bytes / task_raw_bytes
and the scratch bytes; the bytes delivered are compared.  Prints the section (and writes it to --out if given); it is the first
part of profiles/archive_device_stop.md.

Needs a GPU; there is no fallback.  The upload of the archive is outside the timed region (the caller of the device path holds
it in HBM already -- that is the case the path is for); the file path's page cache is warm (tmpfs)."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
MB = 1e6


def build_archives(csa, root):
    """-> {name: (archive path, {index name: content}, add options)}"""
    import csa_cases
    from csc_amd import treegen
    out = {}
    d = os.path.join(root, "many_files")
    os.makedirs(d)
    content = csa_cases.make_tree(d, "many_files")
    out["many_files"] = (d, ["m"], content, dict(csa_cases.CSA_CASES["many_files"]["opts"]))
    d = os.path.join(root, "tree_small")
    os.makedirs(d)
    treegen.materialize(d, "tree_small")
    content = {}
    for base, _, names in os.walk(os.path.join(d, "t")):
        for n in names:
            p = os.path.join(base, n)
            content[os.path.relpath(p, d)] = open(p, "rb").read()
    out["tree_small"] = (d, ["t"], content, dict(level=3, dict_size=64 << 20, recurse=True))
    for name, (d, args, content, opts) in out.items():
        os.chdir(d)
        rc, _ = csa.add("out.csa", args, overwrite=True, **opts)
        if rc != 0:
            raise SystemExit(f"csa.add {name}: rc={rc}")
    return out


def gathered_bytes(csa, path):
    import orc_csa
    _, abindex, _ = orc_csa.unpack_index(csa.read_index(path))
    return sum(10 + (sum(n for _, n in v) - 10 if len(v) > 1 else 0) for v in abindex.values())


def spread(ts):
    return statistics.median(ts), min(ts), max(ts)


def main_stop(args):
    """--stop-early: a selection, with and without the stop"""
    import torch
    import cases
    from csc_amd import csa, treegen
    csa.lib()
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="csa_stop_", dir=shm)
    lines = ["## A selection with and without the stop", "",
             f"`tools/gpu_archive_device.py --stop-early --repeats {args.repeats}` on {torch.cuda.get_device_name(0)}: `DeviceArchive.extract(names)` "
             "(CSAMI_DeviceRead, the parent commit's text) against `extract(names, stop_early=True)` (CSAMI_DeviceReadStop) on the same handle, "
             "alternating, after one warm-up each.  Wall seconds per call: median (min .. max).", "",
             "| archive | selection | tasks | full read s | stopped read s | decoded / task raw bytes | scratch bytes: full, stopped | decode launches: full, stopped |",
             "|---|---|---|---|---|---|---|---|"]
    cwd = os.getcwd()
    try:
        trees = {}
        d = os.path.join(root, "one_ext")
        os.makedirs(os.path.join(d, "data"))
        for i in range(24):
            with open(os.path.join(d, "data", f"a{i:04d}.npy"), "wb") as f:
                f.write(cases.build([[("text", "exe", "delta")[i % 3], 300 + i, 0, 1 << 20]]))
        trees["one_ext"] = (d, ["data"], dict(level=2, dict_size=32 << 20, recurse=True))
        d = os.path.join(root, "tree_small")
        os.makedirs(d)
        treegen.materialize(d, "tree_small")
        trees["tree_small"] = (d, ["t"], dict(level=3, dict_size=64 << 20, recurse=True))
        d = os.path.join(root, "split4")
        os.makedirs(d)
        with open(os.path.join(d, "big.bin"), "wb") as f:
            f.write(cases.build([["text", 340, 0, 16 << 20]]))
        trees["split4"] = (d, ["big.bin"], dict(level=2, dict_size=32 << 20, split_count=4))
        for name, (d, argv, opts) in trees.items():
            os.chdir(d)
            rc, _ = csa.add("out.csa", argv, overwrite=True, **opts)
            if rc != 0:
                raise SystemExit(f"csa.add {name}: rc={rc}")
            data = open("out.csa", "rb").read()
            names = args.select
            if not names:                                  # the file that lies first in the largest task
                raw = {}
                entries = csa.list_entries("out.csa")
                for e in entries:
                    for f in e["frags"]:
                        raw[f["bid"]] = max(raw.get(f["bid"], 0), f["posblock"] + f["size"])
                big = max(raw, key=lambda b: raw[b])
                names = [next(e["name"] for e in entries if any(f["bid"] == big and f["posblock"] == 0 and f["size"] for f in e["frags"]))]
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            with csa.DeviceArchive.open(dev) as a:
                total = a.plan(names)[1]
                dsts = [torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda") for _ in range(2)]
                times, last = ([], []), [None, None]
                for rep in range(args.repeats + 1):
                    for k in ((0, 1) if rep % 2 == 0 else (1, 0)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rc, views, st = a.extract(names, dst=dsts[k], stop_early=bool(k))
                        dt = time.perf_counter() - t0
                        assert rc == 0 and st["verify_failures"] == 0, (name, rc)
                        last[k] = st
                        if rep:
                            times[k].append(dt)
                assert bool((dsts[0] == dsts[1]).all()), "the stopped read delivered other bytes"
                for f in last[1]["files"]:
                    rel = f["name"]
                    if os.path.isfile(rel):
                        assert dsts[1][f["offset"]:f["offset"] + f["size"]].cpu().numpy().tobytes() == open(rel, "rb").read(), rel
            full, stop = last
            raw_scratch = csa.plan_device_stops(csa.read_index("out.csa"), len(data), names)[1]
            fs = "%.4f (%.4f .. %.4f)"
            lines.append(f"| {name} ({len(data)} bytes) | {' '.join(names)} | {stop['tasks']}, {stop['stopped_tasks']} stopped | {fs % spread(times[0])} | {fs % spread(times[1])} | "
                         f"{stop['decoded_bytes']} / {stop['task_raw_bytes']} = {stop['decoded_bytes'] / max(stop['task_raw_bytes'], 1):.4f} | "
                         f"{sum((t['raw'] + 255) // 256 * 256 for t in raw_scratch)}, {stop['scratch_bytes']} | {full['decode_launches']}, {stop['decode_launches']} |")
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)
    lines.append("")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stop-early", action="store_true")
    ap.add_argument("--select", nargs="+", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device.py needs a GPU: a CPU run says nothing about these paths")
    if args.stop_early or args.select:
        return main_stop(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "archive_device.md")
    from csc_amd import csa
    csa.lib()
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="csa_dev_", dir=shm)
    lines = ["# Device-resident archive read: measured", "",
             f"`tools/gpu_archive_device.py --repeats {args.repeats}` on {torch.cuda.get_device_name(0)}; both paths run on this tree's "
             "library (the file path's code is unchanged from the parent commit).  Wall time per call, median (min .. max); MB/s = raw "
             f"bytes / median.  Files on {'tmpfs (/dev/shm)' if shm else 'the temporary directory (no tmpfs found)'}.", ""]
    cwd = os.getcwd()
    try:
        arcs = build_archives(csa, root)
        for name, (d, _, content, _) in arcs.items():
            os.chdir(d)
            data = open("out.csa", "rb").read()
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            a = csa.DeviceArchive.open(dev)
            total = a.plan()[1]
            dst = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
            xdir = os.path.join(d, "x")

            def file_test():
                rc, st = csa.test("out.csa")
                assert rc == 0 and st["verify_failures"] == 0
                return st

            def file_extract():
                shutil.rmtree(xdir, ignore_errors=True)
                rc, st = csa.extract("out.csa", to_dir=xdir)
                assert rc == 0 and st["verify_failures"] == 0
                return st

            def dev_test():
                rc, st = a.test()
                assert rc == 0 and st["verify_failures"] == 0
                st["kernel_ms3"] = a.kernel_ms()
                return st

            def dev_extract():
                rc, views, st = a.extract(dst=dst)
                assert rc == 0 and st["verify_failures"] == 0
                st["kernel_ms3"] = a.kernel_ms()
                return st

            paths = {"CSA_Test (file)": file_test, "DeviceArchive.test": dev_test, "CSA_Extract (file)": file_extract, "DeviceArchive.extract": dev_extract}
            times, last = {k: [] for k in paths}, {}
            for k, fn in paths.items():
                fn()                                                    # warm-up: code objects, caches, the decoder's resource cache
            rc, views, _ = a.extract(dst=dst)
            for rel, want in content.items():
                assert views[rel].cpu().numpy().tobytes() == want, rel
            for _ in range(args.repeats):
                for k, fn in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = fn()
                    times[k].append(time.perf_counter() - t0)
            raw = last["DeviceArchive.test"]["raw_bytes"]
            gat = gathered_bytes(csa, "out.csa")
            st = last["DeviceArchive.extract"]
            lines += [f"## {name}: {len(content)} files, {raw} raw bytes, archive {len(data)} bytes, {st['tasks']} tasks, {st['frags']} fragments", "",
                      "| path | s per call | MB/s |", "|---|---|---|"]
            for k in paths:
                med, lo, hi = spread(times[k])
                lines.append(f"| {k} | {med:.4f} ({lo:.4f} .. {hi:.4f}) | {raw / med / MB:.0f} |")
            lines += ["", f"Device path, last extract: waves {st['waves']}, launches {st['launches']}, decode launches {st['decode_launches']}, "
                          f"read-back bytes {st['readback_bytes']}.", "",
                      "| kernel | call | ms (HIP events) | bytes moved | GB/s |", "|---|---|---|---|---|"]
            for call, moved in (("DeviceArchive.test", raw), ("DeviceArchive.extract", 2 * raw)):
                g, p, f = last[call]["kernel_ms3"]
                lines.append(f"| k_gather_extents | {call} | {g:.4f} | {2 * gat} | {2 * gat / (g * 1e-3) / 1e9 if g else 0:.1f} |")
                lines.append(f"| k_frag_pieces | {call} | {p:.4f} | {moved} | {moved / (p * 1e-3) / 1e9 if p else 0:.1f} |")
                lines.append(f"| k_frag_fold | {call} | {f:.4f} | - | - |")
            lines.append("")
            a.close()
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)
    lines += ["## What these numbers are, and what was not measured", "",
              "- Kernel times are one launch per kernel per wave at these archive sizes: a few hundred KB to a few MB a launch is a "
              "measurement of launch overhead as much as of bandwidth, so the GB/s above are NOT the kernels' share of the 6.3 TB/s "
              "a streaming kernel can reach on this device.  An archive of several GB was not measured.  k_gather_extents moved the property bytes only: no task stream of these archives exceeds one archive block, so nothing was gathered and its bandwidth was not measured.",
              "- Not measured: the parent commit's library as a separate build (the file path's code is the same text), rocprofv3 "
              "kernel traces, PMC counters, more than one wave at a realistic budget, archives written with `-t4`.",
              "- Not built: overlap of a wave's gather with the previous wave's decode, "
              "decoding straight into dst where a task is one whole file.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
