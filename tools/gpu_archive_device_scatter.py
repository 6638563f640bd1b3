#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the device archive over the caller's own buffers against the contiguous calls, on the
same data.  N entries (default 24, about 21 MiB, six extensions so six task streams; level 1, 1 MiB dictionary) are uploaded twice:
once back to back into one tensor, once into N separately allocated tensors at byte offsets 0, 1, 3, 8, 15 in rotation.  Then, the
calls of each group alternating, `--repeats` times after one warm-up:
    write     DeviceArchive.write (one tensor)            | DeviceArchive.write_tensors (N tensors); the archives must be equal
    read      DeviceArchive.extract (one dst)             | DeviceArchive.extract_into (a second set of N tensors)
    verify    DeviceArchive.test                          | DeviceArchive.compare with the originals | ... with a mutated set
Per call: wall seconds (median, min .. max), the stats that matter, and the HIP-event time of this layer's kernels with the bytes
the middle one moved -- k_frag_pieces<true> loads and stores every fragment byte, k_frag_compare loads it twice, k_frag_pieces<false>
(test) loads it once.  The ratio k_frag_compare / k_frag_pieces<true> is taken per repeat, from calls that ran back to back.
Writes profiles/archive_device_scatter.md.

    python tools/gpu_archive_device_scatter.py [--repeats 5] [--entries 24] [--out profiles/archive_device_scatter.md]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OFFSETS = [0, 1, 3, 8, 15]
SIZES = [(2 << 20) + 1, (512 << 10) + 3, 70001, (1 << 20) - 5]
KINDS = [("text", "txt"), ("exe", "exe"), ("delta", "dat"), ("text", "log"), ("silesia", "bin"), ("text", "md")]
OPTS = dict(level=1, dict_size=1 << 20)
FILE_ATTR = ord("u") + (0o100644 << 8)


def med(ts):
    return f"{statistics.median(ts):.4f} ({min(ts):.4f} .. {max(ts):.4f})"


def measure(repeats, n_entries):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_scatter.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    content = {}
    for i in range(n_entries):
        kind, ext = KINDS[i % len(KINDS)]
        content[f"s/e{i:03d}.{ext}"] = corpus.fill(kind, 100 + i, 0, SIZES[i % len(SIZES)]).tobytes()

    def alone(data, off):
        buf = torch.empty(off + len(data) + 1, dtype=torch.uint8, device="cuda")
        buf[off:off + len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        return buf[off:off + len(data)]
    # one tensor, and N tensors
    table, src = [], bytearray()
    for name, data in content.items():
        off = (len(src) + 15) // 16 * 16
        src.extend(bytes(off - len(src)) + data)
        table.append({"name": name, "esize": len(data), "edate": edate, "eattr": FILE_ATTR, "offset": off})
    dev = torch.frombuffer(src, dtype=torch.uint8).cuda()
    entries = [{"name": n, "tensor": alone(d, OFFSETS[i % 5]), "edate": edate, "eattr": FILE_ATTR} for i, (n, d) in enumerate(content.items())]
    mutated = {}
    for i, (n, d) in enumerate(content.items()):
        b = bytearray(d)
        b[(len(d) * (i + 1)) // (n_entries + 1)] ^= 0x10
        mutated[n] = alone(bytes(b), OFFSETS[(i + 2) % 5])
    originals = {e["name"]: e["tensor"] for e in entries}
    second = {n: alone(bytes(len(d)), OFFSETS[(i + 3) % 5]) for i, (n, d) in enumerate(content.items())}
    rc, nt, _, raw = csa.device_write_plan(table, "out.csa", **OPTS)
    assert rc == 0
    cap = 24 + raw + raw // 8 + (64 << 10) * (nt + 1) + (1 << 20)
    arcs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def write():
        rc, view, st = csa.DeviceArchive.write(table, dev, "out.csa", arc=arcs[0], **OPTS)
        assert rc == 0
        return view, st, csa.device_write_kernel_ms()

    def write_tensors():
        rc, view, st = csa.DeviceArchive.write_tensors(entries, "out.csa", arc=arcs[1], **OPTS)
        assert rc == 0
        return view, st, csa.device_write_kernel_ms()

    out = {"device": torch.cuda.get_device_name(0), "raw": raw, "n": n_entries, "calls": {}}

    def run(group):
        for fn in group.values():
            fn()                                                            # warm-up
        res = {k: {"wall": [], "ms": [], "st": None} for k in group}
        for _ in range(repeats):
            for k, fn in group.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, st, ms = fn()
                res[k]["wall"].append(time.perf_counter() - t0)
                res[k]["ms"].append(list(ms))
                res[k]["st"] = {a: b for a, b in st.items() if a != "files"}
        out["calls"].update(res)
        return res

    run({"write": write, "write_tensors": write_tensors})
    assert bool((write()[0] == write_tensors()[0]).all()), "the two writes' archives differ"
    a = csa.DeviceArchive.open(arcs[1][:write_tensors()[1]["archive_bytes"]])
    dst = torch.empty(a.plan()[1], dtype=torch.uint8, device="cuda")

    def extract():
        rc, views, st = a.extract(dst=dst)
        assert rc == 0 and st["verify_failures"] == 0
        return views, st, a.kernel_ms()

    def extract_into():
        rc, st = a.extract_into(second)
        assert rc == 0 and st["verify_failures"] == 0
        return None, st, a.kernel_ms()

    def test():
        rc, st = a.test()
        assert rc == 0 and st["verify_failures"] == 0
        return None, st, a.kernel_ms()

    def compare_with(srcs, differ):
        def fn():
            rc, diffs, st = a.compare(srcs)
            assert rc == 0 and st["verify_failures"] == 0
            assert all((d["status"] == csa.CSA_DIFF_BYTES) == differ for d in diffs.values())
            return diffs, st, a.kernel_ms()
        return fn

    run({"extract": extract, "extract_into": extract_into, "test": test, "compare (equal)": compare_with(originals, False),
         "compare (every entry differs)": compare_with(mutated, True)})
    views = extract()[0]
    for n, d in content.items():
        assert bool((views[n] == second[n]).all()) and bool((second[n] == originals[n]).all()), n
    a.close()
    return out


def report(r, repeats):
    raw, c = r["raw"], r["calls"]
    lines = ["# Device archive over the caller's buffers: measured", "",
             f"`tools/gpu_archive_device_scatter.py --repeats {repeats} --entries {r['n']}` on {r['device']}: {r['n']} entries, {raw} raw bytes, "
             f"level {OPTS['level']}, {OPTS['dict_size'] >> 20} MiB dictionary.  The calls of a group alternate; wall time per call and "
             "HIP-event milliseconds are medians (min .. max).  The two writes' archives were compared byte for byte, and what "
             "extract_into delivered with what extract delivered and with the originals.", "",
             "## Write", "", "| call | s per call | tasks | waves | launches | bytes up | bytes down | k_frag_pieces ms | k_frag_fold ms | k_block_table ms | k_gather_extents ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for k in ("write", "write_tensors"):
        st, ms = c[k]["st"], list(zip(*c[k]["ms"]))
        lines.append(f"| {k} | {med(c[k]['wall'])} | {st['tasks']} | {st['waves']} | {st['launches']} | {st['upload_bytes']} | {st['readback_bytes']} | "
                     + " | ".join(med(m) for m in ms) + " |")
    lines += ["", "## Read, verify, compare", "",
              "| call | s per call | tasks | frags | waves | launches | bytes down | k_gather_extents ms | middle kernel | its ms | bytes it moved | GB/s | fold ms |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    middle = {"extract": ("k_frag_pieces<true>", 2), "extract_into": ("k_frag_pieces<true>", 2), "test": ("k_frag_pieces<false>", 1),
              "compare (equal)": ("k_frag_compare", 2), "compare (every entry differs)": ("k_frag_compare", 2)}
    for k, (kern, factor) in middle.items():
        st, ms = c[k]["st"], list(zip(*c[k]["ms"]))
        m1 = statistics.median(ms[1])
        lines.append(f"| {k} | {med(c[k]['wall'])} | {st['tasks']} | {st['frags']} | {st['waves']} | {st['launches']} | {st['readback_bytes']} | {med(ms[0])} | "
                     f"{kern} | {med(ms[1])} | {factor * raw} | {factor * raw / (m1 * 1e-3) / 1e9:.1f} | {med(ms[2])} |")
    for name, num, den in (("k_frag_compare / k_frag_pieces<true> (compare, equal / extract_into)", "compare (equal)", "extract_into"),
                           ("k_frag_pieces<true> scattered / contiguous (extract_into / extract)", "extract_into", "extract")):
        ratios = [x[1] / y[1] for x, y in zip(c[num]["ms"], c[den]["ms"])]
        lines += ["", f"{name}, per repeat: " + ", ".join(f"{x:.3f}" for x in ratios) + f"; median {statistics.median(ratios):.3f}, "
                  f"spread {min(ratios):.3f} .. {max(ratios):.3f}."]
    lines += ["", "## What these numbers are", "",
              "- One launch per kernel per wave at these sizes: a few MB a launch measures launch overhead as much as bandwidth, so the GB/s "
              "above are NOT the kernels' share of what a streaming kernel reaches on this device, and the ratio of two such times is mostly the "
              "ratio of two launch overheads.",
              "- The wall times of the writes are the encoder's; of the reads, the decoder's.  This layer's kernels are the milliseconds in "
              "the right-hand columns.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entries", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_scatter.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.entries), args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
