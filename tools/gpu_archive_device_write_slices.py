#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): entries gathered from strided slices (DeviceArchive.write_slices) against the only way
to archive the same bytes without it -- `t[:, c0:c1].contiguous()` followed by write_tensors.  One row-major matrix of --rows x
--row-bytes (default 16384 x 16384: 256 MiB, 16 MiB of text, exe and delta data repeated) lies in device memory; a block of columns
of each of --widths bytes (default 8 -- the slow path, run < 16 --, 64, 1024, 2048), beginning at byte column 4099, and a block of
1/8 of its whole rows are archived as one entry, level 1, 1 MiB dictionary, task_bytes 1 MiB.  Alternating, `--repeats` times after
one warm-up, per case:
    gather    write_slices of the matrix under rows_slice
    copy      the .contiguous() copy alone, ended by a synchronise
    write     write_tensors of that copy
Per case: wall seconds (median, min .. max) of each, slot [0] of the write's kernel times -- k_frag_rows for the gather, or
k_frag_pieces where no piece crosses a run border -- and the selected bytes over it, the pieces by kind, the tasks by kind.  The two
archives of a case are compared byte for byte once.  Writes profiles/archive_device_write_slices.md.

    python tools/gpu_archive_device_write_slices.py [--repeats 3] [--rows 16384] [--row-bytes 16384] [--widths 8,64,1024,2048]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OPTS = dict(level=1, dict_size=1 << 20, task_bytes=1 << 20)
FILE_ATTR = ord("u") + (0o100644 << 8)
C0 = 4099


def med(ts):
    return f"{statistics.median(ts):.4f} ({min(ts):.4f} .. {max(ts):.4f})"


def measure(repeats, rows, row_bytes, widths):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_write_slices.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    size = rows * row_bytes
    unit = min(size, 16 << 20)
    part = unit // 3
    seed = b"".join(corpus.fill(k, 200 + i, 0, n).tobytes() for i, (k, n) in enumerate([("text", part), ("exe", part), ("delta", unit - 2 * part)]))
    base = torch.frombuffer(bytearray(seed), dtype=torch.uint8).cuda().repeat((size + unit - 1) // unit)[:size].contiguous()
    m = base.view(rows, row_bytes)
    row = {"name": "w", "edate": edate, "eattr": FILE_ATTR}
    cases = {f"columns, {w} bytes": (slice(None), slice(C0, C0 + w), csa.rows_slice(row_bytes, 0, rows, C0, C0 + w)) for w in widths}
    r0 = rows * 3 // 8
    cases["whole rows, 1/8 of them"] = (slice(r0, r0 + rows // 8), slice(None), csa.rows_slice(row_bytes, r0, r0 + rows // 8))
    out = {"device": torch.cuda.get_device_name(0), "size": size, "rows": rows, "row_bytes": row_bytes, "cases": {}}
    for name, (rs, cs, s) in cases.items():
        res = {"slice": s, "gather": [], "copy": [], "write": [], "gather_ms": [], "write_ms": [], "st": None, "st_w": None}
        for rep in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc, arc, st = csa.DeviceArchive.write_slices([dict(row, tensor=base, slice=s)], **OPTS)
            t1 = time.perf_counter()
            gms = csa.device_write_kernel_ms()
            assert rc == 0
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            packed = m[rs, cs].contiguous().view(-1)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            rc, arc_w, st_w = csa.DeviceArchive.write_tensors([dict(row, tensor=packed)], **OPTS)
            t4 = time.perf_counter()
            wms = csa.device_write_kernel_ms()
            assert rc == 0
            if rep == 0:                                                    # warm-up, and the one comparison
                assert arc.numel() == arc_w.numel() and bool((arc == arc_w).all()), name
                continue
            res["gather"].append(t1 - t0); res["copy"].append(t3 - t2); res["write"].append(t4 - t3)
            res["gather_ms"].append(gms[0]); res["write_ms"].append(wms[0])
            res["st"] = {k: v for k, v in st.items() if k != "files"}
            res["st_w"] = {k: v for k, v in st_w.items() if k != "files"}
            del arc, arc_w, packed
            print(f"{name}: repeat {rep}: gather {t1 - t0:.3f} s, copy {t3 - t2:.4f} s, write {t4 - t3:.3f} s", file=sys.stderr, flush=True)
        out["cases"][name] = res
    return out


def report(r, args):
    lines = ["# Device archive write, entries gathered from strided slices: measured", "",
             f"`tools/gpu_archive_device_write_slices.py --repeats {args.repeats} --rows {r['rows']} --row-bytes {r['row_bytes']} --widths {args.widths}` on "
             f"{r['device']}: a matrix of {r['size']} bytes in device memory; each case is one entry, level {OPTS['level']}, {OPTS['dict_size'] >> 20} MiB "
             f"dictionary, task_bytes {OPTS['task_bytes']}.  The three calls of a case alternate; wall seconds and HIP-event milliseconds are medians "
             "(min .. max) of the repeats after one warm-up.  The gathered archive and the copy-then-write archive of every case were compared byte "
             "for byte.", "",
             "| case | slice (offset, run, stride, count) | selected bytes | tasks (gathered / in place) | periodic pieces | plain pieces | "
             "gather: s per call | its slot [0] ms | selected bytes / slot [0], GB/s | copy: s | write_tensors: s per call | its slot [0] ms | "
             "copy + write: s |", "|" + "---|" * 13]
    for name, x in r["cases"].items():
        st = x["st"]
        g = statistics.median(x["gather_ms"])
        both = [a + b for a, b in zip(x["copy"], x["write"])]
        lines.append(f"| {name} | {tuple(x['slice'])} | {st['selected_bytes']} | {st['tasks']} ({st['gathered_tasks']} / {st['inplace_tasks']}) | "
                     f"{st['periodic_pieces']} | {st['plain_pieces']} | {med(x['gather'])} | {med(x['gather_ms'])} | {st['selected_bytes'] / g / 1e6:.1f} | "
                     f"{med(x['copy'])} | {med(x['write'])} | {med(x['write_ms'])} | {med(both)} |")
    lines += ["", "## What these numbers are", "",
              "- Slot [0] is the gather-and-sum pass of the call: k_frag_rows where a piece crosses a run border (periodic pieces > 0), k_frag_pieces "
              "otherwise -- for the whole rows every task is encoded where it lies and the pass only sums.  For write_tensors it is "
              "k_frag_pieces over the copy.  The GB/s are selected (stored) bytes over that time; the bytes LOADED are more where a 32-byte "
              "window reaches into a gap.",
              "- The wall time of a write is the encoder's: it moves with the selected bytes, hardly with this layer's kernels.  What the gather "
              "saves is the copy and the memory of the copy, what it costs is the difference of the two slot [0] columns.",
              "- The 8-byte columns are the slow path: run < 16, every 16-byte unit assembled byte by byte.  No rate is promised for it.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--row-bytes", type=int, default=16384)
    ap.add_argument("--widths", default="8,64,1024,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_write_slices.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.rows, args.row_bytes, [int(w) for w in args.widths.split(",")]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
