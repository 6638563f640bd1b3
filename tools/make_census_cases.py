#!/usr/bin/env python3
"""Search small inputs that reach every event of the encoder census (oracle/orc_api.h, enum OrcEvent; tests/census_cases.py) in
every dispatch row where its branch exists, and freeze them: tests/golden/census_cases.json <- the oracle's counters.

Deterministic (fixed seeds, fixed order) and CPU-only.  Per row it runs the oracle, census attached, over
  * the row's props variants of tests/test_gpu_forms.py and small custom geometries that keep the row (narrow hash tables, a short
    tree ring, few or many descent steps, short good_len), dict 32 KiB so that the window wraps within an input.  bt_size stays
    above 8 KiB + 128: SlidePos' skip rule advances bt_pos_ by up to a sub-block's 8 KiB without wrapping it and csc_mf.cpp:161
    subtracts bt_size_ once, so with a smaller ring the reference itself writes outside bt_nodes_,
  * small corpus stretches and splices in soak_gen form, and constructed ["pattern", hex, repeat] parts (runs, short periods,
    far short repeats for the kBound rejects, a ladder of growing prefixes for the candidate list),
  * csc_blocksize 65536 and a few tiny ones (the coder events),
then covers the (event, row) cells greedily, rarest event first, smallest input first.  A case is at most 128 KiB, a row's cases
1 MiB together.  It also measures, with the checker (the reference build where present), the block sizes from which the decoder
reads the encoder's own streams, and records the block-size family's counts.  What it could not reach it prints: those cells
belong in census_cases.OPEN with a reason."""
import ctypes as C
import itertools
import json
import os
import random
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases                       # noqa: E402
import census_cases as cc          # noqa: E402
import soak_gen                    # noqa: E402
from csc_amd.capi import CscLib    # noqa: E402

SEED = 20250
KINDS = ["text", "exe", "delta", "random", "entropy8", "silesia"]


def geometries(row):
    """(level, overrides) candidates that select `row`"""
    g = list(cc.ROW_VARIANTS[row])
    if row == "level3":
        g += [(3, {"hash_width": w, "hash_bits": hb, "good_len": gl}) for w in (1, 2) for hb in (6, 12) for gl in (2, 4, 16)]
    elif row == "level4":
        g += [(4, {"hash_bits": 8}), (4, {"hash_bits": 12, "good_len": 17}), (3, {"good_len": 17, "hash_bits": 8}), (3, {"good_len": 200}),
              (3, {"hash_width": 9, "hash_bits": 8, "good_len": 4}), (3, {"hash_width": 3, "hash_bits": 6})]
    elif row == "level5":
        g += [(5, {"bt_size": bs, "bt_cyc": cy, "good_len": gl, "bt_hash_bits": hb})
              for bs in (9000, 20000) for cy in (1, 4, 32) for gl in (8, 48) for hb in (4, 10)]
    elif row == "level12":
        g += [(lv, {"hash_width": w, "hash_bits": hb, "good_len": gl, "lz_mode": m})
              for lv, w, hb, gl, m in [(2, 8, 6, 24, 2), (2, 8, 12, 4, 2), (1, 1, 8, 8, 2), (2, 2, 10, 200, 1), (2, 5, 6, 8, 1), (1, 3, 12, 32, 2)]]
    elif row == "lazy_w9":
        g += [(2, {"hash_width": 9, "hash_bits": hb, "good_len": gl, "lz_mode": m}) for hb, gl, m in [(6, 24, 2), (12, 4, 2), (8, 200, 1), (10, 8, 1)]]
    elif row == "adv_generic":
        g += [(5, {"hash_width": 4, "hash_bits": hb, "bt_size": bs, "bt_cyc": cy, "good_len": gl, "bt_hash_bits": bh})
              for hb, bs, cy, gl, bh in [(8, 9000, 4, 48, 4), (12, 12000, 1, 8, 10), (8, 20000, 32, 48, 4), (12, 12000, 40, 16, 4)]]
        g += [(5, {"bt_cyc": 33, "bt_size": bs, "bt_hash_bits": bh, "good_len": gl}) for bs, bh, gl in [(9000, 4, 48), (12000, 10, 8), (20000, 4, 200)]]
        g += [(3, {"hash_width": w, "hash_bits": hb, "good_len": gl}) for w, hb, gl in [(10, 6, 16), (32, 8, 200), (16, 12, 4)]]
    elif row == "lazy_generic":
        g += [(5, {"lz_mode": m, "bt_size": bs, "bt_cyc": cy, "good_len": gl, "bt_hash_bits": bh})
              for m, bs, cy, gl, bh in [(2, 9000, 4, 48, 4), (2, 12000, 1, 8, 10), (1, 20000, 32, 48, 4), (2, 12000, 32, 200, 4)]]
        g += [(5, {"lz_mode": 2, "hash_width": 4, "hash_bits": 8, "bt_size": 9000, "bt_cyc": 4, "bt_hash_bits": 6})]
        g += [(2, {"hash_width": w, "hash_bits": hb, "good_len": gl, "lz_mode": m}) for w, hb, gl, m in [(10, 6, 24, 2), (32, 8, 200, 2), (16, 12, 4, 1)]]
    return g


def ladder(rng, steps, base_len):
    """growing prefixes of one string, longest first, each behind a separator no other place repeats: at the last copy every older
    bucket / tree entry matches longer than the newer ones, so the candidate list grows by one entry a step"""
    s = bytes(rng.randrange(256) for _ in range(base_len + steps + 4))
    parts = []
    for k in range(steps, -1, -1):
        parts.append(["pattern", (s[:base_len + k] + bytes(rng.randrange(256) for _ in range(5))).hex(), 1])
    parts.append(["pattern", s.hex(), 1])
    return parts


def inputs(rng):
    """[(name, parts)] small first"""
    out = []
    for n in (600, 3000, 9000, 20000, 40000, 70000, 131072):
        for kind in KINDS:
            out.append((f"{kind}{n}", [[kind, 900 + len(out), rng.randrange(0, 5_000_000), n]]))
    # splices: literal-rich stretches cut into text
    for n in (20000, 40000, 70000):
        for k2 in ("delta", "entropy8", "random"):
            a = n // 3
            out.append((f"text+{k2}{n}", [["text", 950, 1000, a], [k2, 951, 0, a], ["text", 950, 1000 + a, n - 2 * a]]))
    # runs and short periods: long matches (the 143 chain, the skip rule, good_len splices, rep matches)
    for hx, rep in [("00", 600), ("61", 5000), ("6162", 400), ("616263", 20000), ("6162636465666768", 6000), ("00", 40000)]:
        out.append((f"pat{hx}x{rep}", [["pattern", hx, rep]]))
    # one stretch again and again at a distance beyond kBound[2..4]: short matches far away, long ones wrapped by a 32 KiB window
    for kind, n, times in [("text", 1100, 30), ("delta", 2100, 20), ("random", 300, 100), ("random", 17000, 3), ("text", 17000, 4),
                           ("entropy8", 5000, 8)]:
        out.append((f"{kind}{n}x{times}", [[kind, 960, 777, n]] * times))
    # far short repeats: random bytes with 2-, 3-, 4- and 5-byte words of an old stretch spliced in
    for gap in (80, 1100, 17000):
        for w in (2, 3, 4, 5):
            words = bytes(rng.randrange(256) for _ in range(64 * w))
            parts = [["pattern", words.hex(), 1], ["random", 970 + w, gap, gap]]
            for i in range(40):
                parts += [["pattern", words[(i % 64) * w:(i % 64) * w + w].hex(), 1], ["random", 971, i * 40, 7 + i % 5]]
            out.append((f"far{w}gap{gap}", parts))
    for steps, base in [(34, 7), (40, 9), (60, 8)]:
        out.append((f"ladder{steps}_{base}", ladder(rng, steps, base)))
        out.append((f"ladder{steps}_{base}+text", ladder(rng, steps, base) + [["text", 980, 0, 3000]]))
    # the block-size family's input and the texts of its encode-only members
    out.append(("family", cc.FAMILY_PARTS))
    return out


def main():
    orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
    orc.lib.orc_zero_alloc.restype = C.c_void_p
    za = orc.lib.orc_zero_alloc()
    chk, _, is_ref = soak_gen.checker()
    assert cc.oracle_names(orc) == cc.EVENTS, "tests/census_cases.py and oracle/orc_api.h name different events"
    rng = random.Random(SEED)
    ins = inputs(rng)
    built = {name: cases.build(parts) for name, parts in ins}
    assert all(len(b) <= cc.MAX_CASE for b in built.values())

    result = {"cases": []}
    unreached = []
    for row in cc.ROWS:
        cands = []
        for (g, (level, over)), (name, parts) in itertools.product(enumerate(geometries(row)), ins):
            n = len(built[name])
            for dsz in ((32768,) if n <= 40000 else (32768, 1 << 20)):
                for bsz in (None, 2, 7, 16, 17, 255, 4096):
                    if bsz is not None and (g > 0 or dsz != 32768 or (n > 40000 and bsz < 255)):       # (the coder does not see the geometry)
                        continue
                    props = dict(over) if bsz is None else dict(over, csc_blocksize=bsz)
                    spec = {"parts": parts, "level": level, "dict": dsz, "props": props}
                    if soak_gen.spec_row(spec) != row:
                        continue
                    spec["row"] = row
                    cands.append((name, spec))

        def run(c):
            rc, _, ev = cc.census(orc, za, c[1], built[c[0]])
            assert rc == 0
            return ev
        with ThreadPoolExecutor(16) as ex:
            evs = list(ex.map(run, cands))
        want = [ev for ev in cc.EVENTS if row in cc.APPLIES[ev] and ev not in cc.DEAD]
        hits = {ev: [i for i in range(len(cands)) if evs[i][ev] > 0] for ev in want}
        for ev in cc.DEAD:
            assert not any(e[ev] for e in evs), f"{ev} is argued dead but was hit"
        chosen, covered = [], set()
        for ev in sorted(want, key=lambda e: (len(hits[e]), cc.EVENTS.index(e))):          # rarest first
            if ev in covered:
                continue
            if not hits[ev]:
                unreached.append((ev, row))
                continue
            i = min(hits[ev], key=lambda i: (len(built[cands[i][0]]), i))                   # smallest input (then search order)
            chosen.append(i)
            covered |= {e for e in want if evs[i][e] > 0}
        total = sum(len(built[cands[i][0]]) for i in chosen)
        assert total <= cc.MAX_ROW, (row, total)
        claimed = set()
        for k, i in enumerate(sorted(chosen, key=lambda i: (len(built[cands[i][0]]), i))):
            name, spec = cands[i]
            mine = {e: evs[i][e] for e in want if evs[i][e] > 0 and e not in claimed}
            claimed |= set(mine)
            _, _, rcd, back = soak_gen.check_one(chk, za, spec, built[name])
            result["cases"].append({"name": f"{row}-{k:02d}-{name}", "row": row, "spec": spec, "size": len(built[name]), "events": mine,
                                    "decodes": rcd == 0 and back == built[name]})
        print(f"{row}: {len(cands)} candidates, {len(chosen)} cases, {total} bytes, {len(want) - len(covered)} cells unreached", flush=True)

    # ---- the floor: csc_blocksize from which the checker's decoder reads the checker's own streams
    probe = {"text3000": [["text", 813, 0, 3000]], "text20000": [["text", 814, 0, 20000]], "random65536": [["random", 11, 0, 65536]],
             "family": cc.FAMILY_PARTS}
    bad = {}
    tried = list(range(1, 65)) + [100, 255, 256, 257, 1000, 4096]
    for b in tried:
        for name, parts in probe.items():
            for level in (2, 3, 5):
                spec = {"parts": parts, "level": level, "dict": 32768, "props": {"csc_blocksize": b}}
                data = cases.build(parts)
                rc, s, rcd, back = soak_gen.check_one(chk, za, spec, data)
                _, s2, ev = cc.census(orc, za, spec, data)
                assert rc == 0 and s == s2
                if rcd != 0 or back != data:
                    bad.setdefault(b, []).append({"input": name, "level": level, "rc": rcd, "whole": back == data, "flush_bc_empty": ev["flush_bc_empty"]})
                else:
                    assert ev["flush_bc_empty"] == 0
    always = [b for b in tried if len(bad.get(b, [])) == len(probe) * 3]
    floor = max(always) + 1 if always else 1
    # above the floor two hazards remain, neither tied to one block size: streams whose Flush left an empty BC block (the decoder's block
    # reader refuses a zero size: rc -1, output cut short), and streams the decoder answers DECODE_ERROR to, some of them after it has
    # written every byte (cause not looked for: the decoder on streams it rejects is another matter)
    above = [(b, x) for b, xs in bad.items() if b >= floor for x in xs]
    assert all((x["flush_bc_empty"] > 0 and x["rc"] == -1) or x["rc"] == cc_decode_error() for b, x in above)
    assert all(x["rc"] == cc_decode_error() for b in always for x in bad[b])
    result["floor"] = {"floor": floor, "checker": "reference" if is_ref else "oracle", "tried": tried, "inputs": sorted(probe),
                       "levels": [2, 3, 5], "below": "DECODE_ERROR (-96) on every stream",
                       "empty_bc_block": sorted({b for b, x in above if x["rc"] == -1}),
                       "decode_error": sorted({b for b, x in above if x["rc"] != -1})}
    # ---- the family: counts per row and member, and whether the checker's decoder reads the stream
    fam = {}
    for row in cc.ROWS:
        fam[row] = {}
        for member, spec in cc.family_members(row):
            data = soak_gen.build_input(spec)
            rc, s, rcd, back = soak_gen.check_one(chk, za, spec, data)
            _, s2, ev = cc.census(orc, za, spec, data)
            assert rc == 0 and s == s2
            fam[row][member] = {"decodes": rcd == 0 and back == data, "events": {e: ev[e] for e in cc.CODER if ev[e]}}
        missing = [e for e in cc.FAMILY_MUST_HIT if not any(fam[row][f"bsize{b}"]["events"].get(e) for b in cc.FAMILY_BSIZES)]
        assert not missing, f"family {row}: {missing} not hit"
    result["family"] = fam
    with open(cc.GOLDEN, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("floor", result["floor"])
    print("unreached (for census_cases.OPEN):")
    for ev, row in unreached:
        print(f"    ({ev!r}, {row!r})")


def cc_decode_error():
    from csc_amd.capi import DECODE_ERROR
    return DECODE_ERROR


if __name__ == "__main__":
    main()
