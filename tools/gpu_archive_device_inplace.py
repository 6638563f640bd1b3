#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the device archive update in place (DeviceArchive.update_in_place) against the out-of-place
update (DeviceArchive.update) of the same base and entries, of the same build, in the same process.  The set-up is
tools/gpu_archive_device_update.py's: a seeded table of --entries tensors (default 320) of --entry-bytes each (default 1 MiB), one
extension, task_bytes = --entry-bytes, so that every entry is its own task.  A base archive and its digest table are written per
level; both calls run with trust_digests.  Three cases:
    nothing      no entry changed: nothing moves
    worse        the entry of task 0 replaced by bytes that do not compress: every stream behind it moves right
    better       the entry of task 0 replaced by zeros: every stream behind it moves left
Per case, alternating, `--repeats` times after one warm-up of each (at which the two archives are compared byte for byte): wall
seconds per call; moved_bytes; k_move_extents' HIP-event milliseconds and GB/s; the out-of-place call's k_gather_extents
milliseconds and GB/s over the bytes it places (the same streams, non-overlapping: the comparison figure); and peak device memory of
a call -- torch.cuda.max_memory_allocated over the call, and the device's own count (torch.cuda.mem_get_info, i.e. hipMemGetInfo,
before the call and sampled during it), whose excess over torch's reserved memory is the library's scratch.
Writes profiles/archive_device_inplace.md.

    python tools/gpu_archive_device_inplace.py [--repeats 3] [--entries 320] [--entry-bytes 1048576] [--levels 2,3]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILE_ATTR = ord("u") + (0o100644 << 8)
CHANGED = 3


def med(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


class Peak:
    """device memory over a call: torch's allocator's peak, and the device's own count sampled from a thread"""

    def __enter__(self):
        import torch
        self.torch = torch
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.alloc0, self.res0 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        self.free0 = self.low = torch.cuda.mem_get_info()[0]
        self.res_hi = self.res0
        self.stop = False

        def poll():
            while not self.stop:
                self.low = min(self.low, torch.cuda.mem_get_info()[0])
                self.res_hi = max(self.res_hi, torch.cuda.memory_reserved())
                time.sleep(0.0005)
        self.th = threading.Thread(target=poll, daemon=True)
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.th.join()
        self.torch_peak = self.torch.cuda.max_memory_allocated() - self.alloc0
        self.device_peak = self.free0 - self.low
        self.library_peak = max(self.device_peak - (self.res_hi - self.res0), 0)


def first_entry(csa, names, edate):
    """which entry is task 0: the plan's order of equal tasks depends on the names and the count alone, so it is asked of a small
    table of the same names -- nine updates, each with the entries changed whose index has one bit set"""
    import torch
    n, size = len(names), 70000
    opts = dict(level=1, dict_size=1 << 16, task_bytes=size)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    old = [torch.randint(0, 8, (size,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    new = [t ^ 1 for t in old]

    def entries(tensors):
        return [{"name": nm, "edate": edate, "eattr": FILE_ATTR, "tensor": t} for nm, t in zip(names, tensors)]
    rc, base, _ = csa.DeviceArchive.write_tensors(entries(old), **opts)
    assert rc == 0
    k = 0
    with csa.DeviceArchive.open(base.clone()) as a:
        for bit in range(max(n - 1, 1).bit_length()):
            rc, _, st = a.update(entries([new[i] if i >> bit & 1 else old[i] for i in range(n)]), trust_sums=True, **opts)
            assert rc == 0
            if st["tasks"][0]["status"] == CHANGED:
                k |= 1 << bit
    return k


def measure(repeats, n, size, levels):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_inplace.py needs a GPU: a CPU run says nothing about these paths")
    from csc_amd import corpus, csa
    csa.lib()
    edate = int(csa.lib().CSA_DecimalTime(1700000000))
    unit = 16 << 20
    part = unit // 3
    seed = b"".join(corpus.fill(k, 500 + i, 0, m).tobytes() for i, (k, m) in enumerate([("text", part), ("exe", part), ("delta", unit - 2 * part)]))
    pool = torch.frombuffer(bytearray(seed), dtype=torch.uint8).cuda()
    old = [pool[(i * 52429) % (unit - size):][:size].clone() for i in range(n)]
    names = [f"layers/{i:04d}.bin" for i in range(n)]
    k0 = first_entry(csa, names, edate)
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    variants = {"nothing": old[k0], "worse": torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda", generator=g),
                "better": torch.zeros(size, dtype=torch.uint8, device="cuda")}

    def entries(tensors):
        return [{"name": nm, "edate": edate, "eattr": FILE_ATTR, "tensor": t} for nm, t in zip(names, tensors)]
    out = {"device": torch.cuda.get_device_name(0), "entries": n, "entry_bytes": size, "first": k0, "rows": []}
    for level in levels:
        opts = dict(level=level, dict_size=1 << 20, task_bytes=size)
        rc, base, bst = csa.DeviceArchive.write_tensors(entries(old), digests=True, **opts)
        assert rc == 0
        base, table = base.clone(), bst["digests"]
        room = torch.empty(base.numel() + size + (1 << 20), dtype=torch.uint8, device="cuda")
        for case, t0 in variants.items():
            new = entries([t0 if i == k0 else old[i] for i in range(n)])
            row = {"level": level, "case": case, "inplace": [], "update": [], "move_ms": [], "gather_ms": [], "st": None, "ost": None}
            for rep in range(repeats + 1):
                with csa.DeviceArchive.open(base) as a:
                    with Peak() as po:
                        t = time.perf_counter()
                        rc, arc, ost = a.update(new, trust_digests=True, base_digests=table, **opts)
                        t_upd = time.perf_counter() - t
                    assert rc == 0
                    row["task"] = next((i for i, t in enumerate(ost["tasks"]) if t["status"] == CHANGED), None)
                    gather_ms = csa.device_write_kernel_ms()[3]
                room[:base.numel()].copy_(base)
                with csa.DeviceArchive.open(room[:base.numel()]) as a:
                    with Peak() as pi:
                        t = time.perf_counter()
                        rc, view, st = a.update_in_place(new, buf=room, trust_digests=True, base_digests=table, **opts)
                        t_in = time.perf_counter() - t
                    assert rc == 0
                    ms = csa.device_move_kernel_ms()
                    if rep == 0:                                            # warm-up, and the one comparison
                        assert view.numel() == arc.numel() and bool((view == arc).all()), (level, case)
                        del arc
                        continue
                del arc
                row["inplace"].append(t_in); row["update"].append(t_upd)
                row["move_ms"].append(ms[1] + ms[2]); row["gather_ms"].append(gather_ms)
                row["st"] = {k: v for k, v in st.items() if k not in ("files", "tasks", "digests")}
                row["ost"] = {k: v for k, v in ost.items() if k not in ("files", "tasks", "digests")}
                row["peak_in"] = (pi.torch_peak, pi.library_peak, pi.device_peak)
                row["peak_out"] = (po.torch_peak, po.library_peak, po.device_peak)
                print(f"level {level}, {case}: repeat {rep}: in place {t_in:.3f} s, out of place {t_upd:.3f} s, moves {ms[1] + ms[2]:.3f} ms",
                      file=sys.stderr, flush=True)
            out["rows"].append(row)
    return out


def gbs(nbytes, ms):
    return f"{nbytes / (ms * 1e6):.1f}" if ms > 0 and nbytes else ""


def report(r, args):
    total = r["entries"] * r["entry_bytes"]
    mib = lambda b: f"{b / (1 << 20):.1f}"
    lines = ["# Device archive update in place against the out-of-place update: measured", "",
             f"`tools/gpu_archive_device_inplace.py --repeats {args.repeats} --entries {r['entries']} --entry-bytes {r['entry_bytes']} --levels {args.levels}` "
             f"on {r['device']}: {r['entries']} entries of {r['entry_bytes']} bytes ({total} bytes) in tensors of their own, 1 MiB dictionary, "
             f"task_bytes {r['entry_bytes']} -- every entry is its own task; task 0 is entry {r['first']}.  The base archive and its digest table "
             "were written by write_tensors(digests=True) at the row's level; both calls run with trust_digests.  The out-of-place update (into an "
             "archive tensor it allocates) and the update in place (the base copied back into one buffer first, outside the timing) alternate in one "
             "process; wall seconds per call are medians (min .. max) of the repeats after one warm-up of each, at which the two archives were "
             "compared byte for byte.  No throughput was promised for k_move_extents: nobody had measured it.  Its comparison figure is the "
             "out-of-place call's k_gather_extents placement of the same run, which copies the same streams between two buffers that do not overlap.", "",
             "| level | case | changed task | in place: s per call | out of place: s per call | moves | moved bytes | parked | k_move_extents ms | GB/s | "
             "out of place: k_gather_extents ms | placed bytes | GB/s | held stream bytes | in place: peak MiB torch / library / device | "
             "out of place: peak MiB torch / library / device |", "|" + "---|" * 16]
    for x in r["rows"]:
        st, ost = x["st"], x["ost"]
        mm, gm = statistics.median(x["move_ms"]), statistics.median(x["gather_ms"])
        placed = ost["archive_bytes"]
        lines.append(f"| {x['level']} | {x['case']} | {'' if x['task'] is None else x['task']} | {med(x['inplace'])} | {med(x['update'])} | {st['moves']} | {st['moved_bytes']} | {st['parked_moves']} | "
                     f"{mm:.3f} | {gbs(st['moved_bytes'], mm)} | {gm:.3f} | {placed} | {gbs(placed, gm)} | {st['held_stream_bytes']} | "
                     f"{' / '.join(mib(b) for b in x['peak_in'])} | {' / '.join(mib(b) for b in x['peak_out'])} |")
    lines += ["", "## What these numbers are", "",
              "- GB/s counts every byte once (a copy loads it and stores it).  k_move_extents' milliseconds are the HIP-event time of its one "
              "launch (the left or the right phase; no move of these cases is parked), the hipMemsetAsync of its state block included.",
              "- Peak memory: torch's column is torch.cuda.max_memory_allocated over the call minus what was allocated before it -- for the "
              "out-of-place call that is the new archive tensor; the device column is hipMemGetInfo's free bytes before the call minus the lowest "
              "value a sampling thread saw during it; the library column is the device column minus the growth of torch's reserved memory, i.e. "
              "the scratch the library allocates itself (encoder state, streams, tables).  The sampling thread can miss a short peak.",
              "- Registers of the build: k_move_extents: 63 VGPRs, 0 AGPRs, 36 SGPRs, 0 bytes of scratch, 8 bytes of LDS a workgroup (the ticket and "
              "the go word), occupancy 8 waves a SIMD.",
              "- A workgroup loads its whole 32 KiB chunk, publishes one flag and polls one or two flags of lower tickets, which were published "
              "without waiting for anyone: there is no chain from chunk to chunk.", verdict(r), ""]
    return "\n".join(lines)


def verdict(r):
    """the mover's rate against k_gather_extents' of the same row, over the rows that moved anything"""
    ratios = []
    for x in r["rows"]:
        mm, gm = statistics.median(x["move_ms"]), statistics.median(x["gather_ms"])
        if mm > 0 and gm > 0 and x["st"]["moved_bytes"]:
            ratios.append((x["st"]["moved_bytes"] / mm) / (x["ost"]["archive_bytes"] / gm))
    if not ratios:
        return "- No row of this run moved a byte."
    text = f"- In this run the mover runs at {100 * min(ratios):.0f} % to {100 * max(ratios):.0f} % of k_gather_extents' rate over the same streams"
    if min(ratios) >= 0.5:
        return text + ": not below half of it.  It issues the same loads and stores; what it adds is the ticket draw, two barriers and the flag round trip a workgroup."
    return text + (": BELOW half of it in at least one row.  Which of the chain, the polls or the loads sets that has not been separated here: "
                   "rerun with the poll loop compiled out (no overlap: shift larger than the move) against this run to split the polls from the loads.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--entries", type=int, default=320)
    ap.add_argument("--entry-bytes", type=int, default=1 << 20)
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_inplace.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.entries, args.entry_bytes, [int(v) for v in args.levels.split(",")]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
