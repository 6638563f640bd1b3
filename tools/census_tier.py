#!/usr/bin/env python3
"""Write profiles/encoder_census.md: which events of the encoder census (oracle/orc_api.h, enum OrcEvent) the GPU tier's encoder
inputs reach, per dispatch row, counted by the oracle on the CPU; and what the census cases (tests/golden/census_cases.json) add.

The tier's inputs, as the tests build them: tests/test_gpu_forms.py (the single streams, the 24-size batches, every eighth stream
of the threshold batches), the three test_soak_single seeds of tests/test_gpu_soak.py, every tenth stream of its first batch seed,
and the non-heavy cases.STREAM_CASES at five levels.  A cell is the number of STREAMS of that row that hit the event at least
once."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases                       # noqa: E402
import census_cases as cc          # noqa: E402
import soak_gen                    # noqa: E402
import test_gpu_forms as F         # noqa: E402
import test_gpu_soak as S          # noqa: E402
from csc_amd.capi import CscLib    # noqa: E402


def tier_specs():
    out = []
    for row in F.FORMS:
        out.append(F._spec(row, 0, 1 << 20, F.SINGLE_PARTS))
        for i, n in enumerate(F.BATCH_SIZES):
            out.append(F._spec(row, i, 1 << 20 if n > soak_gen.CHUNK else max(n, 1), [[F._kind(i), 600 + i, i * 7919, n]]))
    for row, count in F.THRESHOLD_CASES:
        out += F._small_streams(row, count, count)[::8]
    for seed in S.SINGLE_SEEDS:
        out += S.single_specs(seed)
    for rnd in S.batch_specs(S.BATCH_SEEDS[0]):
        out += rnd[::10]
    for name, (parts, dsz, clamp, max_read) in cases.STREAM_CASES.items():
        if name in cases.HEAVY:
            continue
        n = len(cases.build(parts))
        for level in cases.LEVELS:
            spec = {"parts": parts, "level": level, "dict": min(dsz, n) if clamp else dsz, "props": {}, "max_read": max_read}
            spec["row"] = soak_gen.spec_row(spec)
            out.append(spec)
    return out


def table(title, rows_hit, totals):
    lines = [f"### {title}", "", "| event | " + " | ".join(cc.ROWS) + " |", "|---|" + "---:|" * len(cc.ROWS),
             "| *streams* | " + " | ".join(str(totals[r]) for r in cc.ROWS) + " |"]
    for ev in cc.EVENTS:
        cells = [(str(rows_hit[r][ev]) if r in cc.APPLIES[ev] else "-") for r in cc.ROWS]
        lines.append(f"| `{ev}` | " + " | ".join(cells) + " |")
    return lines + [""]


def main():
    orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
    orc.lib.orc_zero_alloc.restype = C.c_void_p
    za = orc.lib.orc_zero_alloc()
    specs = tier_specs()
    with ThreadPoolExecutor(16) as ex:
        evs = list(ex.map(lambda s: cc.census(orc, za, s)[2], specs))
    hit = {r: {ev: 0 for ev in cc.EVENTS} for r in cc.ROWS}
    totals = {r: 0 for r in cc.ROWS}
    for s, ev in zip(specs, evs):
        totals[s["row"]] += 1
        for e in cc.EVENTS:
            hit[s["row"]][e] += ev[e] > 0
    golden = cc.load()
    new = {r: {ev: 0 for ev in cc.EVENTS} for r in cc.ROWS}
    for c in golden["cases"]:
        got = cc.census(orc, za, c["spec"])[2]
        for e in cc.EVENTS:
            new[c["row"]][e] += got[e] > 0
    out = ["# Encoder census: what the GPU tier reaches, and what the census cases add", "",
           "Written by `tools/census_tier.py` from the counters in `oracle/orc_encoder.c` (`orc_census_attach`).  Events are named",
           "branches of the reference (`oracle/orc_api.h`, `enum OrcEvent`); a cell counts the streams of a dispatch row that hit the",
           "event at least once; `-` marks a row in which the event's branch does not exist (`tests/census_cases.py`, `APPLIES`).", "",
           f"## The tier before the census cases ({len(specs)} streams)", "",
           "`tests/test_gpu_forms.py` (threshold batches sampled 1 in 8), the three `test_soak_single` seeds, the first batch seed",
           "sampled 1 in 10, the non-heavy `cases.STREAM_CASES` at five levels.  None of them sets `csc_blocksize`.", ""]
    out += table("streams that hit the event, per row", hit, totals)
    zero = [(ev, r) for ev in cc.EVENTS for r in cc.APPLIES[ev] if hit[r][ev] == 0 and ev not in cc.DEAD]
    out += ["Cells the tier never reached (dead events aside): " + ", ".join(f"`{ev}`/{r}" for ev, r in zero) + ".", ""]
    out += ["## The census cases", "",
            f"{len(golden['cases'])} cases, {sum(c['size'] for c in golden['cases'])} input bytes in all.  Each row's cases run in three kernel",
            "forms in `tests/test_gpu_census.py` -- alone (the row's single-stream kernel), together (its batch kernel) and, where the row",
            "has a threshold, with fillers one stream above it (its over-threshold kernel) -- so a cell below is covered in every form",
            "of its row:", "",
            "| row | single | multi | over |", "|---|---|---|---|"]
    for r, f in F.FORMS.items():
        out.append(f"| {r} | `{f['single']}` | `{f['multi']}` | " + (f"`{f['over']}`" if f["threshold"] else "(no threshold)") + " |")
    out.append("")
    out += table("census cases that hit the event, per row", new, {r: len(cc.cases_of(r)) for r in cc.ROWS})
    out += ["## OPEN cells", ""]
    out += [f"- `{ev}` / {row}: {why}" for (ev, row), why in cc.OPEN.items()] or ["None: every cell where an event's branch exists has a case."]
    out += ["", "Argued dead in the reference (the arguments stand beside the events in `oracle/orc_encoder.c`); no input of the search,",
            "the tier or the cases hit them:", ""]
    out += [f"- `{ev}`: {why}" for ev, why in cc.DEAD.items()]
    fl = golden["floor"]
    out += ["", "## Block sizes", "",
            f"Measured with the {fl['checker']} build on {', '.join(fl['inputs'])} at levels {fl['levels']}, `csc_blocksize` {fl['tried'][0]} .. 64 and "
            f"{', '.join(str(b) for b in fl['tried'] if b > 64)}: below **{fl['floor']}** the decoder answers DECODE_ERROR to every stream of its own encoder.",
            "At and above it two hazards remain, tied to the stream and not to one block size: a `Coder::Flush` whose two BC bytes end",
            f"exactly on a block seam writes an empty BC block, which the block reader refuses (rc -1; seen at {fl['empty_bc_block']}), and",
            f"some streams end in DECODE_ERROR (seen at {fl['decode_error']}, the mixed input only).  The encoder side is exact at every size:",
            "`tests/test_gpu_census.py` compares the streams down to `csc_blocksize` 1.", "",
            "The search also met a fault of the reference itself: with `bt_size` below about 8 KiB a long match lets `SlidePos`' skip rule",
            "(csc_mf.cpp:145) run `bt_pos_` past the ring, :161 subtracts `bt_size_` once, and the insert writes outside `bt_nodes_`",
            "(glibc aborted the search with a corrupted heap at `bt_size` 300).  The search keeps `bt_size` at 9000 and above.", ""]
    with open(os.path.join(ROOT, "profiles", "encoder_census.md"), "w") as f:
        f.write("\n".join(out))
    print("\n".join(out[:12]))
    print("never reached by the tier:", zero)


if __name__ == "__main__":
    main()
