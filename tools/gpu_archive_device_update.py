#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the device archive update (DeviceArchive.update) against the fresh write of the same
entries (DeviceArchive.write_tensors) of the same build, in the same process.  A seeded table of --entries tensors (default 320) of
--entry-bytes each (default 1 MiB: 320 MiB of text, exe and delta data), one extension, task_bytes = --entry-bytes, so that every
entry is its own task, encoded where it lies.  A base archive is written per level; then, per row, one byte is flipped in every
16th, every 2nd or every entry -- the changed fraction of the TASKS is 0, 1/16, 1/2 or 1 -- and, alternating, `--repeats` times
after one warm-up of each:
    update    DeviceArchive.update over the base (verify, or trust_sums)
    fresh     DeviceArchive.write_tensors of the new entries
Levels 2 and 3, both modes.  Per row: wall seconds per call (median, min .. max) of both, and the update's statistics.  The two
archives of a row are compared byte for byte at the warm-up.  A row's "update against fresh" says "within the spread" when the
[min, max] ranges of the two overlap.  Writes profiles/archive_device_update.md.

    python tools/gpu_archive_device_update.py [--repeats 3] [--entries 320] [--entry-bytes 1048576] [--levels 2,3]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILE_ATTR = ord("u") + (0o100644 << 8)
FRACTIONS = [("0", 0), ("1/16", 16), ("1/2", 2), ("1", 1)]      # (label, every n-th entry changed; 0: none)


def med(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def measure(repeats, n, size, levels):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_update.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    unit = 16 << 20
    part = unit // 3
    seed = b"".join(corpus.fill(k, 500 + i, 0, m).tobytes() for i, (k, m) in enumerate([("text", part), ("exe", part), ("delta", unit - 2 * part)]))
    pool = torch.frombuffer(bytearray(seed), dtype=torch.uint8).cuda()
    old = [pool[(i * 52429) % (unit - size):][:size].clone() for i in range(n)]
    flipped = []
    for t in old:
        c = t.clone()
        c[size // 2] ^= 0x5A
        flipped.append(c)
    names = [f"layers/{i:04d}.bin" for i in range(n)]

    def entries(tensors):
        return [{"name": nm, "edate": edate, "eattr": FILE_ATTR, "tensor": t} for nm, t in zip(names, tensors)]
    out = {"device": torch.cuda.get_device_name(0), "entries": n, "entry_bytes": size, "rows": []}
    for level in levels:
        opts = dict(level=level, dict_size=1 << 20, task_bytes=size)
        rc, base, bst = csa.DeviceArchive.write_tensors(entries(old), **opts)
        assert rc == 0
        base = base.clone()
        for label, every in FRACTIONS:
            new = [flipped[i] if every and i % every == 0 else old[i] for i in range(n)]
            for trust in (False, True):
                row = {"level": level, "fraction": label, "mode": "trust_sums" if trust else "verify", "update": [], "fresh": [], "st": None,
                       "fst": None}
                with csa.DeviceArchive.open(base) as a:
                    for rep in range(repeats + 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rc, arc, st = a.update(entries(new), trust_sums=trust, **opts)
                        t1 = time.perf_counter()
                        assert rc == 0
                        rc, arc_f, fst = csa.DeviceArchive.write_tensors(entries(new), **opts)
                        t2 = time.perf_counter()
                        assert rc == 0
                        if rep == 0:                                        # warm-up, and the one comparison
                            assert arc.numel() == arc_f.numel() and bool((arc == arc_f).all()), (level, label, trust)
                            continue
                        row["update"].append(t1 - t0); row["fresh"].append(t2 - t1)
                        row["st"] = {k: v for k, v in st.items() if k not in ("files", "tasks")}
                        row["st"]["tasks"] = len(st["tasks"])
                        row["fst"] = {k: v for k, v in fst.items() if k != "files"}
                        del arc, arc_f
                        print(f"level {level}, changed {label}, {row['mode']}: repeat {rep}: update {t1 - t0:.3f} s, fresh {t2 - t1:.3f} s",
                              file=sys.stderr, flush=True)
                out["rows"].append(row)
    return out


def verdict(u, f):
    if min(u) > max(f):
        return "slower"
    if max(u) < min(f):
        return "faster"
    return "within the spread"


def report(r, args):
    total = r["entries"] * r["entry_bytes"]
    lines = ["# Device archive update against the fresh write: measured", "",
             f"`tools/gpu_archive_device_update.py --repeats {args.repeats} --entries {r['entries']} --entry-bytes {r['entry_bytes']} --levels {args.levels}` "
             f"on {r['device']}: {r['entries']} entries of {r['entry_bytes']} bytes ({total} bytes) in tensors of their own, 1 MiB dictionary, "
             f"task_bytes {r['entry_bytes']} -- every entry is its own task, encoded where it lies.  The base archive was written by write_tensors "
             "at the row's level; a changed entry has one byte flipped.  update and the fresh write_tensors of the same entries alternate in one "
             "process; wall seconds per call are medians (min .. max) of the repeats after one warm-up of each, at which the two archives were "
             "compared byte for byte.  No ratio was promised in advance: the last column is what the run says, \"within the spread\" where the "
             "[min, max] ranges of the two calls overlap.", "",
             "| level | changed tasks | mode | tasks | reused / encoded | update: s per call | fresh write: s per call | update against fresh | "
             "median ratio fresh / update | seconds_check | check kernel ms | checked bytes | decoded bytes | check waves | update seconds_encode | "
             "fresh seconds_encode |", "|" + "---|" * 16]
    for x in r["rows"]:
        st, fst = x["st"], x["fst"]
        ratio = statistics.median(x["fresh"]) / statistics.median(x["update"])
        lines.append(f"| {x['level']} | {x['fraction']} | {x['mode']} | {st['tasks']} | {st['reused_tasks']} / {st['encoded_tasks']} | {med(x['update'])} | "
                     f"{med(x['fresh'])} | {verdict(x['update'], x['fresh'])} | {ratio:.2f} | {st['seconds_check']:.3f} | {st['check_kernel_ms']:.2f} | "
                     f"{st['checked_bytes']} | {st['decoded_bytes']} | {st['check_waves']} | {st['seconds_encode']:.3f} | {fst['seconds_encode']:.3f} |")
    lines += ["", "## What these numbers are", "",
              "- The statistics columns are those of the last repeat.  seconds_check is the wall time of the check phase (candidates on the host, the "
              "property bytes, the decode in verify, the compare or sum pass and the fold); seconds_encode is the time inside "
              "CSCMI_EncodeDeviceBatch, the index stream included.",
              "- verify decodes every candidate's base stream and compares it with the caller's bytes, so its check costs a decode of everything "
              "that is a candidate whatever fraction then turns out changed; trust_sums reads the caller's bytes once and decodes nothing.",
              "- With every task changed the update is the fresh write plus a check that reuses nothing: that row is the price of asking.",
              "- Encoding is latency-bound per stream: the time inside CSCMI_EncodeDeviceBatch is set by the wave's slowest stream, not by the "
              "number of streams, as long as the device is not full -- compare \"update seconds_encode\" across the changed fractions.  So copying "
              "the streams of most tasks saves little wall time while a few tasks of the same size are still encoded; it saves their scratch, their "
              "encoder state and the device for other work.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--entries", type=int, default=320)
    ap.add_argument("--entry-bytes", type=int, default=1 << 20)
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_update.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.entries, args.entry_bytes, [int(v) for v in args.levels.split(",")]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
