#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): byte ranges and strided slices of an entry (DeviceArchive.extract_slices) against the read
of the whole entry, on the same archive.  One "matrix" entry of --rows x --row-bytes (default 4096 x 8192: 32 MiB of text, exe and
delta data) and three small entries are written with write_tensors(task_bytes=2 MiB), level 1, 1 MiB dictionary, so the matrix is
cut across at least 16 tasks.  Then, alternating, `--repeats` times after one warm-up, each with and without stop_early:
    whole     the entry as one byte range
    rows      a block of 1/8 of its rows, from the middle: one byte range
    columns   a block of 1/8 of its columns: one run out of every row
and extract_into of the same entry, whose middle kernel is k_frag_pieces<true>.  Per call: wall seconds (median, min .. max), the
tasks it decoded, decoded_bytes and scratch_bytes beside what the host planner (plan_device_slices) says over the archive's index,
the pieces by kind, and the HIP-event time of the middle kernel.  What each slice delivered is compared with extract's bytes once.
Writes profiles/archive_device_slices.md.

    python tools/gpu_archive_device_slices.py [--repeats 5] [--rows 4096] [--row-bytes 8192] [--out profiles/archive_device_slices.md]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OPTS = dict(level=1, dict_size=1 << 20, task_bytes=2 << 20)
FILE_ATTR = ord("u") + (0o100644 << 8)
MATRIX = "w/matrix.bin"


def med(ts):
    return f"{statistics.median(ts):.4f} ({min(ts):.4f} .. {max(ts):.4f})"


def measure(repeats, rows, row_bytes):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_slices.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    size = rows * row_bytes
    part = size // 4
    content = {MATRIX: b"".join(corpus.fill(k, 200 + i, 0, n).tobytes() for i, (k, n) in enumerate(
                   [("text", part), ("exe", part), ("delta", part), ("text", size - 3 * part)])),
               "w/a.txt": corpus.fill("text", 301, 0, 70001).tobytes(), "w/b.exe": corpus.fill("exe", 302, 0, 16385).tobytes(),
               "w/c.dat": corpus.fill("delta", 303, 0, 17).tobytes()}
    entries = [{"name": n, "tensor": torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda(), "edate": edate, "eattr": FILE_ATTR}
               for n, d in content.items()]
    rc, arc, wst = csa.DeviceArchive.write_tensors(entries, **OPTS)
    assert rc == 0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.csa")
        with open(path, "wb") as f:
            f.write(arc.cpu().numpy().tobytes())
        raw_index = csa.read_index(path)
    a = csa.DeviceArchive.open(arc)
    rc, views, st = a.extract([MATRIX])
    assert rc == 0 and st["verify_failures"] == 0
    truth = views[MATRIX].clone()
    assert st["tasks"] >= 16, st["tasks"]
    r0 = rows * 3 // 8
    slices = {"whole": (0, size), "rows": csa.rows_slice(row_bytes, r0, r0 + rows // 8), "columns": csa.rows_slice(row_bytes, 0, rows, 0, row_bytes // 8)}
    dsts = {k: torch.empty(s[1] * (s[3] if len(s) == 4 else 1), dtype=torch.uint8, device="cuda") for k, s in slices.items()}
    whole_dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    out = {"device": torch.cuda.get_device_name(0), "size": size, "rows": rows, "row_bytes": row_bytes, "archive_bytes": int(arc.numel()),
           "archive_tasks": wst["tasks"], "slices": slices, "plan": {}, "calls": {}}
    for k, s in slices.items():
        rc, plan, touched = csa.plan_device_slices(raw_index, int(arc.numel()), {MATRIX: s}, [MATRIX])
        assert rc == 0
        out["plan"][k] = {"tasks": len(plan), "touched": touched, "stops": sum(t["stop"] for t in plan), "raws": sum(t["raw"] for t in plan),
                          "scratch": sum((t["stop"] + 255) // 256 * 256 for t in plan)}

    def sliced(k, stop):
        def fn():
            rc, got, st = a.extract_slices({MATRIX: slices[k]}, {MATRIX: dsts[k]}, [MATRIX], stop_early=stop)
            assert rc == 0 and st["verify_failures"] == 0
            return st, a.kernel_ms()
        return fn

    def into(stop):
        def fn():
            rc, st = a.extract_into({MATRIX: whole_dst}, [MATRIX], stop_early=stop)
            assert rc == 0 and st["verify_failures"] == 0
            return st, a.kernel_ms()
        return fn

    group = {}
    for stop in (True, False):
        for k in slices:
            group[(k, stop)] = sliced(k, stop)
        group[("extract_into", stop)] = into(stop)
    for fn in group.values():
        fn()                                                                # warm-up
    res = {k: {"wall": [], "ms": [], "st": None} for k in group}
    for _ in range(repeats):
        for k, fn in group.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st, ms = fn()
            res[k]["wall"].append(time.perf_counter() - t0)
            res[k]["ms"].append(list(ms))
            res[k]["st"] = {x: y for x, y in st.items() if x != "files"}
    out["calls"] = res
    # what was delivered, against extract's bytes
    m = truth.view(rows, row_bytes)
    assert bool((dsts["whole"] == truth).all()) and bool((whole_dst == truth).all())
    assert bool((dsts["rows"] == m[r0:r0 + rows // 8].reshape(-1)).all())
    assert bool((dsts["columns"] == m[:, :row_bytes // 8].reshape(-1)).all())
    a.close()
    return out


def report(r, repeats):
    c, size = r["calls"], r["size"]
    lines = ["# Device archive, byte ranges and strided slices of an entry: measured", "",
             f"`tools/gpu_archive_device_slices.py --repeats {repeats} --rows {r['rows']} --row-bytes {r['row_bytes']}` on {r['device']}: one entry of "
             f"{size} bytes ({r['rows']} rows of {r['row_bytes']}) and three small ones, level {OPTS['level']}, {OPTS['dict_size'] >> 20} MiB dictionary, "
             f"task_bytes {OPTS['task_bytes']}: {r['archive_tasks']} tasks, {r['archive_bytes']} archive bytes.  The calls alternate; wall time per call "
             "and HIP-event milliseconds are medians (min .. max) of the repeats after one warm-up.  What every slice delivered was compared "
             "with extract's bytes of the whole entry.", "",
             "| read | slice (offset, run, stride, count) | selected bytes |", "|---|---|---|"]
    for k, s in r["slices"].items():
        s4 = (s[0], s[1], s[1], 1) if len(s) == 2 else s
        lines.append(f"| {k} | {s4} | {s4[1] * s4[3]} |")
    for stop in (True, False):
        lines += ["", f"## stop_early = {stop}", "",
                  "| read | s per call | tasks (plan) | decoded bytes (plan: sum of stops) | scratch bytes (plan) | touched bytes | plain pieces | periodic pieces | "
                  "middle kernel | its ms | fold ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for k in list(r["slices"]) + ["extract_into"]:
            x = c[(k, stop)]
            st, ms = x["st"], list(zip(*x["ms"]))
            p = r["plan"].get(k)
            if p:
                dec = f"{st['decoded_bytes']} ({p['stops']})" if stop else f"- (raw sizes: {p['raws']})"
                scr = f"{st['scratch_bytes']} ({p['scratch']})" if stop else "-"
                lines.append(f"| {k} | {med(x['wall'])} | {st['tasks']} ({p['tasks']}) | {dec} | {scr} | {st['touched_bytes']} | {st['plain_pieces']} | "
                             f"{st['periodic_pieces']} | k_frag_slices | {med(ms[1])} | {med(ms[2])} |")
            else:
                dec = str(st["decoded_bytes"]) if stop else "-"
                scr = str(st["scratch_bytes"]) if stop else "-"
                lines.append(f"| {k} (whole entry) | {med(x['wall'])} | {st['tasks']} | {dec} | {scr} | {st['raw_bytes']} | - | - | "
                             f"k_frag_pieces<true> | {med(ms[1])} | {med(ms[2])} |")
    ratios = [x[1] / y[1] for x, y in zip(c[("whole", True)]["ms"], c[("extract_into", True)]["ms"])]
    lines += ["", "k_frag_slices / k_frag_pieces<true> on the whole entry (whole / extract_into, stop_early), per repeat: "
              + ", ".join(f"{x:.3f}" for x in ratios) + f"; median {statistics.median(ratios):.3f}, spread {min(ratios):.3f} .. {max(ratios):.3f}.",
              "", "## What these numbers are", "",
              "- The exact claims are the byte counts: tasks, decoded bytes and scratch bytes equal the host planner's, which the tests assert.",
              "- One launch per kernel per wave: a launch over a few MB measures launch overhead as much as bandwidth, so the milliseconds of the "
              "middle kernel are NOT its share of what a streaming kernel reaches on this device, and a ratio of two such times is mostly a "
              "ratio of two launch overheads.",
              "- The wall time of a read is the decoder's: it falls with the decoded bytes, not with this layer's kernels.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--row-bytes", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_slices.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.rows, args.row_bytes), args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
