#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): a read into, and a comparison against, a strided slice of the caller's buffer
(DeviceArchive.extract_into_slices, compare_slices) against the two-step paths that do the same without them.  Per run length of
--runs bytes (default 4 -- the slow path, run < 16 --, 64, 1024, 65536) a buffer in device memory holds --total bytes (default 8 MiB
of text, exe and delta data) as rows of `run` bytes 4 * run apart, beginning at byte 4099; the rows are archived once as one entry
(write_slices, level 1, 1 MiB dictionary, task_bytes 1 MiB).  Then, alternating, `--repeats` times after one warm-up, per case:
    spread        extract_into_slices into the rows of a second buffer
    read + copy   extract_into a packed scratch tensor, then view.copy_(packed), ended by a synchronise
    rows          compare_slices against the rows of the first buffer
    copy + cmp    view.contiguous(), ended by a synchronise, then compare against the copy
Per case: wall seconds (median, min .. max) of each, slot [1] of the read's kernel times -- k_frag_spread / k_frag_compare_rows where a
piece crosses a run border, k_frag_pieces / k_frag_compare otherwise -- and the selected bytes over it, and the pieces by kind.  The
warm-up checks that both reads give the rows and that both comparisons find them equal.  Writes profiles/archive_device_spread.md.

    python tools/gpu_archive_device_spread.py [--repeats 5] [--total 8388608] [--runs 4,64,1024,65536]

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


def measure(repeats, total, runs):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_spread.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    part = total // 3
    seed = b"".join(corpus.fill(k, 300 + i, 0, n).tobytes() for i, (k, n) in enumerate([("text", part), ("exe", part), ("delta", total - 2 * part)]))
    packed0 = torch.frombuffer(bytearray(seed), dtype=torch.uint8).cuda()
    row = {"name": "w", "edate": edate, "eattr": FILE_ATTR}
    out = {"device": torch.cuda.get_device_name(0), "total": total, "cases": {}}

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    for run in runs:
        count, stride = total // run, 4 * run

        def rows_of(buf):
            return buf[C0:C0 + count * stride].view(count, stride)[:, :run]
        src = torch.zeros(C0 + count * stride, dtype=torch.uint8, device="cuda")
        rows_of(src).copy_(packed0[:count * run].view(count, run))
        dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
        base, s = csa.tensor_slice(rows_of(src))
        rc, arc, _ = csa.DeviceArchive.write_slices([dict(row, tensor=base, slice=s)], **OPTS)
        assert rc == 0
        res = {"slice": s, "spread": [], "read": [], "copy": [], "rows": [], "ccopy": [], "cmp": [],
               "spread_ms": [], "read_ms": [], "rows_ms": [], "cmp_ms": [], "st": None, "st_c": None}
        with csa.DeviceArchive.open(arc) as a:
            for rep in range(repeats + 1):
                t0 = sync()
                rc1, st = a.extract_into_slices({"w": rows_of(dst)})
                t1 = time.perf_counter()
                ms1 = a.kernel_ms()
                scratch = torch.empty(count * run, dtype=torch.uint8, device="cuda")
                t2 = sync()
                rc2, _ = a.extract_into({"w": scratch})
                t3 = time.perf_counter()
                ms2 = a.kernel_ms()
                rows_of(dst2).copy_(scratch.view(count, run))
                t4 = sync()
                rc3, d3, st_c = a.compare_slices({"w": rows_of(src)})
                t5 = time.perf_counter()
                ms3 = a.kernel_ms()
                t6 = sync()
                copy = rows_of(src).contiguous().view(-1)
                t7 = sync()
                rc4, d4, _ = a.compare({"w": copy})
                t8 = time.perf_counter()
                ms4 = a.kernel_ms()
                assert rc1 == rc2 == rc3 == rc4 == 0 and d3["w"]["status"] == d4["w"]["status"] == 0
                if rep == 0:                                                # warm-up, and the one look at the bytes
                    assert torch.equal(dst, src) and torch.equal(dst2, src), run
                    continue
                res["spread"].append(t1 - t0); res["read"].append(t3 - t2); res["copy"].append(t4 - t3)
                res["rows"].append(t5 - t4); res["ccopy"].append(t7 - t6); res["cmp"].append(t8 - t7)
                res["spread_ms"].append(ms1[1]); res["read_ms"].append(ms2[1]); res["rows_ms"].append(ms3[1]); res["cmp_ms"].append(ms4[1])
                res["st"] = {k: v for k, v in st.items() if k != "files"}
                res["st_c"] = {k: v for k, v in st_c.items() if k != "files"}
                del scratch, copy
                print(f"run {run}: repeat {rep}: spread {t1 - t0:.4f} s, read + copy {t4 - t2:.4f} s, rows {t5 - t4:.4f} s, "
                      f"copy + compare {t8 - t6:.4f} s", file=sys.stderr, flush=True)
        out["cases"][run] = res
        del src, dst, dst2, arc
    return out


def report(r, args):
    lines = ["# Device archive read into, and compare against, strided slices: measured", "",
             f"`tools/gpu_archive_device_spread.py --repeats {args.repeats} --total {r['total']} --runs {args.runs}` on {r['device']}: per case "
             f"{r['total']} bytes as rows of `run` bytes 4 * run apart in a buffer in device memory, archived once as one entry, level "
             f"{OPTS['level']}, {OPTS['dict_size'] >> 20} MiB dictionary, task_bytes {OPTS['task_bytes']}.  The calls of a case alternate; wall seconds "
             "and HIP-event milliseconds are medians (min .. max) of the repeats after one warm-up, which checked the bytes of both reads and the "
             "verdict of both comparisons.", "",
             "## Reading", "",
             "| run | slice (offset, run, stride, count) | periodic pieces | plain pieces | extract_into_slices: s | its slot [1] ms | selected bytes / slot [1], "
             "GB/s | extract_into: s | its slot [1] ms | view.copy_(packed): s | read + copy: s |", "|" + "---|" * 11]
    for run, x in r["cases"].items():
        st = x["st"]
        both = [a + b for a, b in zip(x["read"], x["copy"])]
        lines.append(f"| {run} | {tuple(x['slice'])} | {st['periodic_pieces']} | {st['plain_pieces']} | {med(x['spread'])} | {med(x['spread_ms'])} | "
                     f"{st['selected_bytes'] / statistics.median(x['spread_ms']) / 1e6:.1f} | {med(x['read'])} | {med(x['read_ms'])} | {med(x['copy'])} | {med(both)} |")
    lines += ["", "## Comparing", "",
              "| run | periodic pieces | plain pieces | compare_slices: s | its slot [1] ms | selected bytes / slot [1], GB/s | view.contiguous(): s | compare: s | "
              "its slot [1] ms | copy + compare: s |", "|" + "---|" * 10]
    for run, x in r["cases"].items():
        st = x["st_c"]
        both = [a + b for a, b in zip(x["ccopy"], x["cmp"])]
        lines.append(f"| {run} | {st['periodic_pieces']} | {st['plain_pieces']} | {med(x['rows'])} | {med(x['rows_ms'])} | "
                     f"{st['selected_bytes'] / statistics.median(x['rows_ms']) / 1e6:.1f} | {med(x['ccopy'])} | {med(x['cmp'])} | {med(x['cmp_ms'])} | {med(both)} |")
    lines += ["", "## What these numbers are", "",
              "- Slot [1] is the middle kernel of the read's three: k_frag_spread (k_frag_compare_rows) where a piece crosses a run border "
              "(periodic pieces > 0), k_frag_pieces (k_frag_compare) otherwise.  The GB/s are selected bytes over that time: each is loaded "
              "once and stored once (read), or loaded twice (compare); a comparison's 32-byte window may load gap bytes besides.",
              "- The wall time of a read is the decoder's: it moves with the selected bytes, hardly with this layer's kernels.",
              "- The 4-byte rows are the slow path: run < 16, every 16-byte unit goes byte by byte.  No rate is promised for it.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--total", type=int, default=8 << 20)
    ap.add_argument("--runs", default="4,64,1024,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_spread.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.total, [int(w) for w in args.runs.split(",")]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
