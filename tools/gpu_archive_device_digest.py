#!/usr/bin/env python3
"""Measurement (not a test, not bench.py): the device archive update that trusts the fragment digests (DeviceArchive.update with
base_digests and trust_digests) against trust_sums, verify and the fresh write of the same entries (DeviceArchive.write_tensors) of
the same build, in the same process, on the workload of tools/gpu_archive_device_update.py: a seeded table of --entries tensors
(default 320) of --entry-bytes each (default 1 MiB), one extension, task_bytes = --entry-bytes, so that every entry is its own task.
A base archive and its digest table are written per level; then, per row, one byte is flipped in every 16th entry or in none, and,
alternating, `--repeats` times after one warm-up of each: the update in one of the three modes, and the fresh write.  The archives
of a row are compared byte for byte at the warm-up.
Then the kernels alone, by HIP events: k_digest_leaves over all the entries (DeviceArchive.digest_slices) beside k_frag_pieces<false>
over the same bytes (the sum-only pass of the fresh write: it loads the same bytes and hashes nothing), and k_digest_roots over one
fragment of --root-bytes (default 64 MiB), where the root is one serial chain.  Writes profiles/archive_device_digest.md.

    python tools/gpu_archive_device_digest.py [--repeats 3] [--entries 320] [--entry-bytes 1048576] [--levels 2,3]

Needs a GPU; there is no fallback.  Run it under a time limit of its own."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILE_ATTR = ord("u") + (0o100644 << 8)
FRACTIONS = [("0", 0), ("1/16", 16)]                           # (label, every n-th entry changed; 0: none)
MODES = [("verify", {}), ("trust_sums", {"trust_sums": True}), ("trust_digests", {"trust_digests": True})]
# of the build this tool was last run against (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)
RESOURCES = ("k_digest_leaves: 61 VGPRs, 0 AGPRs, 37 SGPRs, 0 bytes of scratch, 4096 bytes of LDS a workgroup (the compiler keeps the message "
             "block of the byte-wise load there), occupancy 8 waves a SIMD; k_digest_roots: 54 VGPRs, 28 SGPRs, 0 bytes of scratch, no LDS")


def med(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def measure(repeats, n, size, levels, root_bytes):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_archive_device_digest.py needs a GPU: a CPU run says nothing about these paths")
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
    out = {"device": torch.cuda.get_device_name(0), "entries": n, "entry_bytes": size, "rows": [], "root_bytes": root_bytes}
    for level in levels:
        opts = dict(level=level, dict_size=1 << 20, task_bytes=size)
        rc, base, bst = csa.DeviceArchive.write_tensors(entries(old), digests=True, **opts)
        assert rc == 0
        base, table = base.clone(), bst["digests"]
        for label, every in FRACTIONS:
            new = [flipped[i] if every and i % every == 0 else old[i] for i in range(n)]
            row = {"level": level, "fraction": label, "fresh": [], "modes": {m: {"t": [], "st": None} for m, _ in MODES}}
            with csa.DeviceArchive.open(base) as a:
                for rep in range(repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rc, arc_f, fst = csa.DeviceArchive.write_tensors(entries(new), **opts)
                    t1 = time.perf_counter()
                    assert rc == 0
                    if rep:
                        row["fresh"].append(t1 - t0)
                    for mode, kw in MODES:
                        t0 = time.perf_counter()
                        rc, arc, st = a.update(entries(new), base_digests=table if mode == "trust_digests" else None, **kw, **opts)
                        t1 = time.perf_counter()
                        assert rc == 0
                        if rep == 0:                                        # warm-up, and the one comparison
                            assert arc.numel() == arc_f.numel() and bool((arc == arc_f).all()), (level, label, mode)
                        else:
                            row["modes"][mode]["t"].append(t1 - t0)
                            row["modes"][mode]["st"] = {k: v for k, v in st.items() if k not in ("files", "tasks", "digests")}
                        del arc
                        print(f"level {level}, changed {label}, {mode}: repeat {rep}: update {t1 - t0:.3f} s", file=sys.stderr, flush=True)
                    del arc_f
            out["rows"].append(row)
    # the kernels alone
    opts = dict(level=2, dict_size=1 << 20, task_bytes=size)
    leaf, root, sums = [], [], []
    for rep in range(repeats + 1):
        rc, t, ds = csa.DeviceArchive.digest_slices(entries(old), **opts)
        assert rc == 0
        ms = csa.device_digest_kernel_ms()
        rc, arc, st = csa.DeviceArchive.write_tensors(entries(old), **opts)
        assert rc == 0
        if rep:
            leaf.append(ms[0]); root.append(ms[1]); sums.append(csa.device_write_kernel_ms()[0])
        del arc
    out["leaf_ms"], out["roots_ms"], out["sum_ms"], out["leaves"] = leaf, root, sums, ds["digest_leaves"]
    big = pool[:1].new_empty(root_bytes)
    big.copy_(pool.repeat(-(-root_bytes // unit))[:root_bytes])
    one = [{"name": "one.bin", "edate": edate, "eattr": FILE_ATTR, "tensor": big}]
    r1, l1 = [], []
    for rep in range(repeats + 1):
        rc, t, ds = csa.DeviceArchive.digest_slices(one, level=2)
        assert rc == 0 and ds["digest_frags"] == 1
        if rep:
            ms = csa.device_digest_kernel_ms()
            l1.append(ms[0]); r1.append(ms[1])
    out["one_root_ms"], out["one_leaf_ms"], out["one_leaves"] = r1, l1, ds["digest_leaves"]
    return out


def verdict(u, f):
    if min(u) > max(f):
        return "slower"
    if max(u) < min(f):
        return "faster"
    return "within the spread"


def report(r, args):
    total = r["entries"] * r["entry_bytes"]
    first = next(x for x in r["rows"] if x["fraction"] == "0")
    td, vf = first["modes"]["trust_digests"]["t"], first["modes"]["verify"]["t"]
    head = {"faster": "With nothing changed trust_digests BEATS verify of the same run",
            "slower": "With nothing changed trust_digests DOES NOT beat verify of the same run: it is slower",
            "within the spread": "With nothing changed trust_digests DOES NOT beat verify of the same run: the two are within the spread"}[verdict(td, vf)]
    lines = ["# Device archive update that trusts the fragment digests: measured", "",
             f"**{head}** (level {first['level']}: {med(td)} s against {med(vf)} s per call).", "",
             f"`tools/gpu_archive_device_digest.py --repeats {args.repeats} --entries {r['entries']} --entry-bytes {r['entry_bytes']} --levels {args.levels}` "
             f"on {r['device']}: {r['entries']} entries of {r['entry_bytes']} bytes ({total} bytes) in tensors of their own, 1 MiB dictionary, "
             f"task_bytes {r['entry_bytes']} -- every entry is its own task and one fragment of {-(-r['entry_bytes'] // 16384)} leaves.  The base "
             "archive and its digest table were written by write_tensors(digests=True) at the row's level; a changed entry has one byte flipped.  "
             "The fresh write and the three updates alternate in one process; wall seconds per call are medians (min .. max) of the repeats after "
             "one warm-up of each, at which every update's archive was compared byte for byte with the fresh write's.  No figure was set in advance.", "",
             "| level | changed tasks | mode | reused / encoded | update: s per call | fresh write: s per call | against fresh | against verify | "
             "seconds_check | check kernel ms | digest kernel ms | digested bytes | mismatches | decoded bytes |", "|" + "---|" * 14]
    for x in r["rows"]:
        for mode, _ in MODES:
            m = x["modes"][mode]
            st = m["st"]
            lines.append(f"| {x['level']} | {x['fraction']} | {mode} | {st['reused_tasks']} / {st['encoded_tasks']} | {med(m['t'])} | {med(x['fresh'])} | "
                         f"{verdict(m['t'], x['fresh'])} | {'' if mode == 'verify' else verdict(m['t'], x['modes']['verify']['t'])} | "
                         f"{st['seconds_check']:.3f} | {st['check_kernel_ms']:.2f} | {st.get('digest_kernel_ms', 0):.2f} | {st.get('digested_bytes', 0)} | "
                         f"{st.get('mismatches', 0)} | {st['decoded_bytes']} |")
    gbs = lambda ms: total / (statistics.median(ms) * 1e-3) / 1e9
    lines += ["", "## The kernels alone (HIP events)", "",
              "| kernel | over | ms (median, min .. max) | GB/s |", "|---|---|---|---|",
              f"| k_digest_leaves, one lane per leaf | {r['leaves']} leaves, {total} bytes | {med(r['leaf_ms'])} | {gbs(r['leaf_ms']):.1f} |",
              f"| k_frag_pieces<false>, one workgroup per piece (the sum-only pass of the fresh write) | the same bytes | {med(r['sum_ms'])} | {gbs(r['sum_ms']):.1f} |",
              f"| k_digest_roots, one lane per fragment | {r['entries']} fragments of {-(-r['entry_bytes'] // 16384)} leaves | {med(r['roots_ms'])} | |",
              f"| k_digest_roots, ONE fragment of {r['root_bytes']} bytes | {r['one_leaves']} leaf digests, one serial chain of {r['one_leaves'] // 2} compressions | "
              f"{med(r['one_root_ms'])} | |",
              f"| k_digest_leaves for that fragment | {r['one_leaves']} leaves | {med(r['one_leaf_ms'])} | {r['root_bytes'] / (statistics.median(r['one_leaf_ms']) * 1e-3) / 1e9:.1f} |",
              "", "## What these numbers are", "",
              "- trust_digests digests the candidates' fragments where they lie (one leaf launch and one root launch a call), compares them on the "
              "device with the base table, and then runs trust_sums's check waves for the property bytes and for the new index's checksums; nothing "
              "is decoded.  So it costs trust_sums plus the digest pass.",
              "- The leaf pass is the PLAIN form: a lane loads its own 64-byte blocks, 16 KiB from its neighbours'.  The form that stages a "
              "wavefront's leaves transposed through LDS has NOT been built, so there is no measurement of it against the plain form here.  "
              "What this run does say: the pass is bound by one lane's serial chain of 256 compressions, not by its loads -- the one fragment's "
              "leaves (64 wavefronts at 64 MiB) take about as long as the table's (320 wavefronts at 320 MiB) -- so coalescing the loads can gain "
              "at most the difference between the two rows.",
              f"- Registers of the build: {RESOURCES}.",
              "- The sum-only pass is the yardstick because it reads the same bytes and does no hashing.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--entries", type=int, default=320)
    ap.add_argument("--entry-bytes", type=int, default=1 << 20)
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--root-bytes", type=int, default=64 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_device_digest.md"))
    args = ap.parse_args()
    text = report(measure(args.repeats, args.entries, args.entry_bytes, [int(v) for v in args.levels.split(",")], args.root_bytes), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
