"""Seeded small inputs for the chunk walk (CSCEncoder::Compress) and the duplicate check (LZ::IsDuplicateBlock /
MatchFinder::TestFind), shared by tools/make_golden_walk_edges.py (which records the REFERENCE's streams in
tests/golden/walk_edges.json), tests/test_walk_edges.py (oracle, CPU) and tests/test_gpu_walk.py (the HIP kernels).  A plain
module like filter_cases.py, not a conftest.

A case is a Case: name (family/...), data, a soak_gen-style spec (level, dict, props overrides: raw_blocksize, the filter
switches, table geometry), `cells` -- the cells of COVERAGE it is there for -- and `claims`, the trace facts it states
(tests/test_walk_edges.py holds every claim against the oracle's trace, oracle/orc_api.h orc_trace_*).

Blocks are built from csc_amd.corpus stretches and literal patterns and typed with orc_analyze_block while they are built:
a block that does not get the verdict it was built for stops the generator.  Two facts the duplicate cases lean on: an
offset is probed (and, in a no-LZ run, inserted) exactly when HASH2 % 16 == 0, which for the reference's HASH2 is "the low
nibble of the byte is 0"; and the window side of every compare starts at wnd_curpos, the start of the PENDING run, minus the
distance.  A `quiet` block is a DT_ENTROPY block over seven symbols with a non-zero low nibble: it has no probed offset
but the ones planted into it.

The plain-Python restatements at the end (walk, test_find_verdict) take the trace's per-block and per-candidate figures and
give the run list and the verdict; each takes ONE planted mistake by name."""
import ctypes as C
import hashlib
import random
from collections import namedtuple

import numpy as np

from csc_amd import corpus

BLK = 8192
DT_NORMAL, DT_ENGTXT, DT_EXE, DT_FAST, DT_NO_LZ, DT_ENTROPY, DT_BAD, DT_DLT, DT_SKIP = 1, 2, 3, 4, 5, 7, 8, 0x10, 0x1E
DLT_CHN = (1, 2, 3, 4, 8)
TYPE_NAMES = {DT_NORMAL: "normal", DT_ENGTXT: "engtxt", DT_EXE: "exe", DT_FAST: "fast", DT_ENTROPY: "entropy", DT_BAD: "bad",
              DT_SKIP: "skip", **{DT_DLT + k: f"dlt{DLT_CHN[k]}" for k in range(5)}}
QUIET = bytes([0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77])    # no probed offset among these
PROBE = 0x10                                                 # low nibble 0: probed, and inserted by a no-LZ run
TAILS = (1, 2, 18, 19, 511, 512)

Case = namedtuple("Case", "name data spec cells claims")

# trace row fields (oracle/orc_api.h)
B_CHUNK, B_BLOCK, B_OFF, B_SIZE, B_AN, B_BPB, B_DLT5, B_DLT_USED, B_SKIP, B_SWITCH, B_BPB95, B_FINAL, B_DUP = 0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16
C_CHUNK, C_BLOCK, C_I, C_TABLE, C_DIST, C_VLD, C_CMP, C_LIMIT, C_ROOM, C_EQ, C_HIT = range(11)


# ---- the oracle's probes ---------------------------------------------------------------------------------------------------

class Orc:
    """orc_analyze_block / orc_dlt_bpb / orc_trace_* of oracle/liborc.so (a ctypes CDLL)"""

    def __init__(self, lib):
        self.lib = lib
        lib.orc_analyze_block.argtypes, lib.orc_analyze_block.restype = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)], C.c_uint32
        lib.orc_dlt_bpb.argtypes, lib.orc_dlt_bpb.restype = [C.c_void_p, C.c_uint32, C.c_uint32], C.c_uint32
        lib.orc_trace_new.argtypes, lib.orc_trace_new.restype = [], C.c_void_p
        lib.orc_trace_attach.argtypes, lib.orc_trace_attach.restype = [C.c_void_p, C.c_void_p], None
        lib.orc_trace_rows.argtypes, lib.orc_trace_rows.restype = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)], C.POINTER(C.c_uint32)
        lib.orc_trace_free.argtypes, lib.orc_trace_free.restype = [C.c_void_p], None

    def analyze(self, blk):
        a = np.frombuffer(bytes(blk), np.uint8).copy()
        bpb = C.c_uint32(0)
        t = self.lib.orc_analyze_block(a.ctypes.data, len(a), C.byref(bpb))
        return int(t), int(bpb.value)

    def dlt_bpb(self, blk, chn):
        a = np.frombuffer(bytes(blk), np.uint8).copy()
        return int(self.lib.orc_dlt_bpb(a.ctypes.data, len(a), chn))


Trace = namedtuple("Trace", "blocks cands runs")


def traced_encode(orc_lib, za, case):
    """(rc, stream, Trace) of the oracle over a case; rows as lists of int tuples"""
    import soak_gen
    o = Orc(orc_lib.lib)
    t = o.lib.orc_trace_new()
    try:
        rc, s = orc_lib.encode(case.data, props=soak_gen.props_of(orc_lib, case.spec), alloc=za,
                               after_create=lambda h: o.lib.orc_trace_attach(h, t))
        out = []
        for kind, width in ((0, 17), (1, 11), (2, 5)):
            n = C.c_size_t(0)
            p = o.lib.orc_trace_rows(t, kind, C.byref(n))
            a = np.ctypeslib.as_array(p, shape=(n.value * width,)).reshape(-1, width) if n.value else np.zeros((0, width), np.uint32)
            out.append([tuple(int(v) for v in row) for row in a])
    finally:
        o.lib.orc_trace_free(t)
    return rc, s, Trace(*out)


# ---- blocks ----------------------------------------------------------------------------------------------------------------

def _np_rng(seed):
    return np.random.RandomState(seed)


def _triangle(rng, m, start, direction):
    """a wave between 10 and 245 in steps of 0..4: equal neighbours one time in five, eight positions on 16 away -- what
    Analyzer::get_channel_idx asks of a channel -- and a flat histogram over 236 values, none of them 0"""
    steps = rng.randint(0, 5, m)
    out = np.zeros(m, np.uint8)
    v, d = start, direction
    for i in range(m):
        v += d * int(steps[i])
        if v > 245:
            v, d = 245 - (v - 245), -1
        elif v < 10:
            v, d = 10 + (10 - v), 1
        out[i] = v
    return out


class Blocks:
    """typed building blocks; every whole 8 KiB block is held against orc_analyze_block as it is made (shorter pieces are
    tails, typed by the case's own claims)"""

    def __init__(self, orc):
        self.o = orc
        self._n = {}

    def _typed(self, b, want):
        if len(b) == BLK:
            got = self.o.analyze(b[:BLK])[0]
            assert got == want, (TYPE_NAMES.get(got, got), TYPE_NAMES[want], len(b))
        return bytes(b)

    def _next(self, key):
        self._n[key] = self._n.get(key, 0) + 1
        return self._n[key]

    def normal(self, n=BLK):
        """32 symbols at random: entropy 500 a byte, no channel"""
        k = self._next("normal")
        return self._typed((_np_rng(1000 + k).randint(0, 32, n) + 0x40).astype(np.uint8).tobytes(), DT_NORMAL)

    def corpus(self, kind, want, n=BLK):
        """the next stretch of a corpus kind that the analyzer gives the wanted verdict"""
        for _ in range(64):
            k = self._next(kind)
            b = corpus.fill(kind, 77, k * 40960, n).tobytes()
            if len(b) != BLK or self.o.analyze(b)[0] == want:
                return b
        raise AssertionError(kind)

    def engtxt(self, n=BLK):
        return self.corpus("text", DT_ENGTXT, n)

    def exe(self, n=BLK):
        return self.corpus("exe", DT_EXE, n)

    def entropy(self, n=BLK):
        return self.corpus("entropy8", DT_ENTROPY, n)

    def bad(self, n=BLK):
        return self.corpus("random", DT_BAD, n)

    def fast(self, n=BLK):
        """a histogram over 230 symbols in shuffled order, 70 of them 31 times and the rest 37 or 38 times in 8 192 bytes (the
        analyzer's logarithm table is stepped: counts of 16..31 and of 32..47 each weigh the same): 780 * size < entropy
        <= 795 * size, diffNum >= 200, no channel"""
        k = self._next("fast")
        rng = _np_rng(2000 + k)
        syms = rng.permutation(256)[:230].astype(np.uint8)
        counts = [31] * 70 + [37] * 160
        for j in range(BLK - sum(counts)):
            counts[70 + j] += 1
        b = np.repeat(syms, counts)
        rng.shuffle(b)
        b = np.resize(b, n)
        return self._typed(b.tobytes(), DT_FAST)

    def dlt(self, k, n=BLK):
        """DLT_CHN[k] interleaved triangle waves (see _triangle), each channel at its own phase"""
        chn = DLT_CHN[k]
        s = self._next(("dlt", k))
        rng = _np_rng(3000 + 10 * s + k)
        out = np.zeros(n + chn, np.uint8)
        for c in range(chn):
            out[c::chn] = _triangle(rng, len(out[c::chn]), 20 + (c * 83 + 11 * s) % 200, 1 if c % 2 == 0 else -1)
        return self._typed(out[:n].tobytes(), DT_DLT + k)

    def quiet(self, n=BLK, probes=()):
        """a DT_ENTROPY block without a probed offset, `probes`: {offset: bytes} planted into it"""
        k = self._next("quiet")
        b = bytearray(QUIET[i] for i in _np_rng(4000 + k).randint(0, len(QUIET), n))
        for off, s in dict(probes).items():
            b[off:off + len(s)] = s
        assert len(b) == n
        return self._typed(b, DT_ENTROPY)

    def of(self, name, n=BLK):
        if name.startswith("dlt"):
            return self.dlt(DLT_CHN.index(int(name[3:])), n)
        return getattr(self, name)(n)


def key19(k, tail=b""):
    """19 bytes that start with the probed symbol: the k-th key, quiet symbols after the first byte"""
    r = _np_rng(5000 + k)
    return bytes([PROBE]) + bytes(QUIET[i] for i in r.randint(0, len(QUIET), 18)) + tail


def _other(sym):
    return QUIET[(QUIET.index(sym) + 1) % len(QUIET)]


# ---- the cases -------------------------------------------------------------------------------------------------------------

MAIN_TYPES = ("normal", "engtxt", "exe", "entropy", "bad", "fast", "dlt2")
TYPE_OF = {"normal": DT_NORMAL, "engtxt": DT_ENGTXT, "exe": DT_EXE, "entropy": DT_ENTROPY, "bad": DT_BAD, "fast": DT_FAST,
           **{f"dlt{DLT_CHN[k]}": DT_DLT + k for k in range(5)}}


def _spec(level=2, dict_=1 << 20, **props):
    return {"level": level, "dict": dict_, "props": props}


def _euler(names):
    """a closed walk over every ordered pair of `names`, self pairs included (Hierholzer on the complete digraph)"""
    adj = {a: list(names) for a in names}
    stack, out = [names[0]], []
    while stack:
        v = stack[-1]
        if adj[v]:
            stack.append(adj[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def types_cases(B):
    out = []
    walk = _euler(MAIN_TYPES)
    assert len(walk) == 50 and {(walk[i], walk[i + 1]) for i in range(49)} == {(a, b) for a in MAIN_TYPES for b in MAIN_TYPES}
    for part, seq in (("a", walk[:26]), ("b", walk[25:])):
        cells = [f"types/pair/{seq[i]}>{seq[i + 1]}" for i in range(len(seq) - 1)] + [f"types/verdict/{n}" for n in set(seq)]
        claims = [("block", 0, i, {B_AN: TYPE_OF[n]}) for i, n in enumerate(seq)]
        out.append(Case(f"types/pairs/{part}", b"".join(B.of(n) for n in seq), _spec(2), cells, claims))
    seq = ["dlt1", "dlt2", "dlt3", "dlt4", "dlt8", "normal", "dlt8", "dlt1"]
    out.append(Case("types/dlt_channels", b"".join(B.of(n) for n in seq), _spec(3),
                    [f"types/verdict/dlt{c}" for c in DLT_CHN],
                    [("block", 0, i, {B_AN: TYPE_OF[n], B_FINAL: TYPE_OF[n]}) for i, n in enumerate(seq)]
                    + [("nruns", 0, 8)]))
    seq = ["fast", "normal", "normal", "fast", "fast", "normal"]
    out.append(Case("types/fast_next_to_normal", b"".join(B.of(n) for n in seq), _spec(2), ["types/fast_splits_a_normal_run"],
                    [("runs", 0, [(DT_FAST, 0, BLK, 0), (DT_NORMAL, BLK, 2 * BLK, 0), (DT_FAST, 3 * BLK, 2 * BLK, 0),
                                  (DT_NORMAL, 5 * BLK, BLK, 1)])]))
    seq = ["dlt2", "engtxt", "engtxt", "exe", "bad", "dlt1", "exe", "engtxt"]
    sw_data = b"".join(B.of(n) for n in seq)
    for off in ("D", "T", "E", "DT", "DE", "TE", "DTE"):
        props = {"DLTFilter": int("D" not in off), "TXTFilter": int("T" not in off), "EXEFilter": int("E" not in off)}
        gone = {TYPE_OF[n] for n in seq if (n.startswith("dlt") and "D" in off) or (n == "engtxt" and "T" in off) or (n == "exe" and "E" in off)}
        claims = []
        for i, n in enumerate(seq):
            t = TYPE_OF[n]
            if off == "DTE":
                claims.append(("block", 0, i, {B_AN: DT_NORMAL, B_FINAL: DT_NORMAL}))
            else:
                claims.append(("block", 0, i, {B_AN: t, B_SWITCH: DT_NORMAL if t in gone else t}))
        out.append(Case(f"types/switch_off/{off}", sw_data, _spec(2, **props), [f"types/switch_off/{off}"], claims))
    return out


def skip_cases(B):
    out = []
    for n in MAIN_TYPES:
        for t in TAILS:
            head = B.of(n)
            tail = B.of(n, t + 64)[64:] if n != "dlt2" else B.dlt(1, BLK + t)[BLK:]
            cells = [f"skip/{n}/{t}"]
            if t < 512:
                claims = [("block", 0, 1, {B_AN: DT_SKIP, B_SIZE: t}), ("inherits", 0, 1)]
            else:
                claims = [("block", 0, 1, {B_SIZE: t}), ("analyzed", 0, 1)]
            out.append(Case(f"skip/{n}/tail{t}", head + tail, _spec(2), cells, claims))
    for t in (1, 511):                                      # a chunk that is one short block only
        out.append(Case(f"skip/alone/{t}", B.dlt(1, t), _spec(2), [f"skip/alone/{t}"],
                        [("block", 0, 0, {B_AN: DT_SKIP, B_SKIP: DT_NORMAL, B_BPB: 0, B_FINAL: DT_NORMAL}),
                         ("runs", 0, [(DT_NORMAL, 0, t, 1)])]))
    for n in ("dlt2", "bad", "entropy"):                    # the tail is the whole second chunk: last_type and bpb start over
        for t in TAILS[:5]:
            data = B.of(n) + (B.dlt(1, BLK + t)[BLK:] if n == "dlt2" else B.of(n, t + 64)[64:])
            out.append(Case(f"skip/second_chunk/{n}/tail{t}", data, _spec(2, raw_blocksize=BLK), [f"skip/second_chunk/{n}/{t}"],
                            [("block", 1, 0, {B_AN: DT_SKIP, B_SKIP: DT_NORMAL, B_BPB: 0, B_FINAL: DT_NORMAL}),
                             ("runs", 1, [(DT_NORMAL, 0, t, 1)])]))
    for t in (1, 19, 511):                                  # ... and behind a delta block INSIDE a second chunk
        data = B.bad() + B.bad() + B.dlt(1, BLK + t)
        out.append(Case(f"skip/in_second_chunk/dlt2/tail{t}", data, _spec(2, raw_blocksize=2 * BLK), [f"skip/in_second_chunk/dlt2/{t}"],
                        [("block", 1, 1, {B_AN: DT_SKIP, B_SKIP: DT_DLT + 1}), ("inherits", 1, 1)]))
    return out


def _rough_wave(seed, mean, hi):
    """one delta channel whose residuals are nearly as costly as its bytes: a wave between 10 and `hi` in geometric steps of
    the given mean (a long tail of rare residuals, which the analyzer's stepped logarithm prices high)"""
    rng = _np_rng(seed)
    steps = rng.geometric(1.0 / (mean + 1), BLK) - 1
    out = np.zeros(BLK, np.uint8)
    v, d = 128, 1
    for i in range(BLK):
        v += d * int(steps[i])
        while v > hi or v < 10:
            if v > hi:
                v, d = 2 * hi - v, -1
            if v < 10:
                v, d = 20 - v, 1
        out[i] = v
    return out.tobytes()


def bpb95_search(o, seeds=range(6000, 9000)):
    """the family the three picks below come from: (seed, mean, hi) -> a block; kept are the first DT_DLT block whose
    GetDltBpb is the largest whole number under bpb * 0.95, one exactly on it (bpb a multiple of 20: the product is exact in
    doubles) and one that is the smallest whole number over it.  Run by hand when the picks have to be found again."""
    found = {}
    for seed in seeds:
        r = random.Random(seed)
        mean, hi = r.choice((40, 41, 42, 43, 44, 45)), r.choice((225, 230, 235, 240, 245))
        blk = _rough_wave(seed, mean, hi)
        t, bpb = o.analyze(blk)
        if t != DT_DLT:
            continue
        gap = o.dlt_bpb(blk, 1) - bpb * 0.95
        side = "on" if gap == 0.0 else "under" if -1.0 < gap < 0 else "over" if 0 < gap < 1.0 else None
        if side:
            found.setdefault(side, (seed, mean, hi))
        if len(found) == 3:
            break
    return found


BPB95_PICKS = {"under": (6034, 40, 230), "on": (6603, 40, 240), "over": (6000, 41, 235)}


def bpb95_cases(B):
    """delta blocks whose GetDltBpb sits just under, exactly on and just over bpb * 0.95 (bpb95_search)"""
    out = []
    for side in ("under", "on", "over"):
        blk = _rough_wave(*BPB95_PICKS[side])
        t, bpb = B.o.analyze(blk)
        assert t == DT_DLT, side
        want = DT_DLT if side == "under" else DT_NORMAL
        out.append(Case(f"bpb95/{side}", B.normal() + blk + B.normal(), _spec(2), [f"bpb95/{side}"],
                        [("block", 0, 1, {B_AN: DT_DLT, B_SWITCH: DT_DLT, B_BPB95: want}), ("bpb95", 0, 1, side)]))
    return out


def runs_cases(B):
    out = []
    raw = 3 * BLK
    for n in ("normal", "bad"):                             # a run of exactly raw_blocksize, then one block more: two runs, two chunks
        data = b"".join(B.of(n) for _ in range(4))
        out.append(Case(f"runs/exactly_raw_plus_one/{n}", data, _spec(2, raw_blocksize=raw),
                        [f"runs/exactly_raw/{n}", f"runs/same_type_across_chunks/{n}"],
                        [("runs", 0, [(TYPE_OF[n], 0, raw, 1)]), ("runs", 1, [(TYPE_OF[n], 0, BLK, 1)])]))
    data = B.normal() + B.normal()[:1024]                   # raw_blocksize no multiple of 8 192: chunks of 4 608, one block each
    out.append(Case("runs/raw_4608", data, _spec(2, raw_blocksize=4096 + 512), ["runs/raw_not_a_multiple"],
                    [("runs", 0, [(DT_NORMAL, 0, 4608, 1)]), ("runs", 1, [(DT_NORMAL, 0, 4608, 1)]), ("nchunks", 2)]))
    out.append(Case("runs/raw_12800", B.entropy(12800) + B.normal(12800), _spec(2, raw_blocksize=12800), ["runs/raw_not_a_multiple"],
                    [("runs", 0, [(DT_ENTROPY, 0, 12800, 1)]), ("runs", 1, [(DT_NORMAL, 0, 12800, 1)])]))
    for where, seq in (("first", ["bad", "normal", "normal"]), ("last", ["normal", "normal", "bad"])):
        data = b"".join(B.of(n) for n in seq + seq)
        first = [(DT_BAD, 0, BLK, 0), (DT_NORMAL, BLK, 2 * BLK, 1)] if where == "first" else [(DT_NORMAL, 0, 2 * BLK, 0), (DT_BAD, 2 * BLK, BLK, 1)]
        out.append(Case(f"runs/type_change_at_{where}_block", data, _spec(2, raw_blocksize=raw), [f"runs/type_change/{where}"],
                        [("runs", 0, first), ("runs", 1, first)]))
    return out


def _dup_case(B, name, blocks, cells, claims, spec=None):
    return Case("dup/" + name, b"".join(blocks), spec or _spec(2), cells, claims)


def dup_cases(B):
    """No-LZ blocks placed so that TestFind sits on its edges.  The usual layout: a quiet SOURCE block with one planted key (a
    no-LZ run: its probed offsets are inserted), a normal block that ends that run, a `bad` block that ends the normal one, and
    the quiet TEST block with the key at one offset: when the test block is typed, the source and the normal run have been
    compressed and the `bad` block is the pending run, so wnd_curpos is that block's start."""
    out = []

    def layout(src_off, test_off, eq=19, tail_equal=False, test_size=BLK):
        """[source, normal, bad, test]; the key at src_off / test_off, `eq` equal bytes then a difference"""
        k = key19(len(out) + 1, bytes(QUIET[:5]))           # 24 bytes
        src = B.quiet(probes={src_off: k})
        kt = bytearray(k)
        if eq < len(kt):
            kt[eq] = _other(kt[eq])
        kt = bytes(kt)[:max(0, test_size - test_off)]
        test = B.quiet(test_size, probes={test_off: kt})
        return [src, B.normal(), B.bad(), test]

    def hit_claims(i, eq, hit, blk=3):
        c = [("cand", 0, blk, {C_I: i, C_HIT: hit, **({C_EQ: eq} if eq < 24 else {})}), ("block", 0, blk, {B_AN: DT_ENTROPY, B_DUP: hit, B_FINAL: DT_NORMAL if hit else DT_ENTROPY})]
        return c

    # 18 equal bytes then a difference, and 19
    out.append(_dup_case(B, "equal18", layout(100, 200, 18), ["dup/equal/18"], hit_claims(200, 18, 0)))
    out.append(_dup_case(B, "equal19", layout(100, 200, 19), ["dup/equal/19"], hit_claims(200, 19, 1)))
    # the copy at size - 19 and size - 18 of the block: limit is what stops the compare
    out.append(_dup_case(B, "at_size-19", layout(100, BLK - 19, 24), ["dup/limit/19"], hit_claims(BLK - 19, 19, 1) + [("cand", 0, 3, {C_LIMIT: 19})]))
    out.append(_dup_case(B, "at_size-18", layout(100, BLK - 18, 24), ["dup/limit/18"], hit_claims(BLK - 18, 18, 0) + [("cand", 0, 3, {C_LIMIT: 18})]))
    # the only probed offset in lane 0, lane 63, the second and the last round of 64
    for nm, off in (("lane0", 0), ("lane63", 63), ("round2", 64 + 37), ("last_round", BLK - 64 + 5)):
        out.append(_dup_case(B, f"only_probe/{nm}", layout(300, off, 24), [f"dup/only_probe/{nm}"],
                             hit_claims(off, 24, 1) + [("ncands", 0, 3, 1)]))
    # a block with no probed offset at all
    out.append(_dup_case(B, "no_probe", [B.quiet(probes={10: key19(99)}), B.normal(), B.bad(), B.quiet()], ["dup/no_probe"],
                         [("ncands", 0, 3, 0), ("block", 0, 3, {B_DUP: 0, B_FINAL: DT_ENTROPY})]))
    return out


def window_cases(B):
    """the duplicate check against a 32 KiB window (vld_rge 24 572): distances at vld_rge, climit from the window's end, the
    wrap of cmp_pos, sources one and two laps back.  Layout: blocks of 8 192; the test block is typed while block `pend` is the
    pending run, so wnd_curpos = pend * 8 192 mod 32 768 and dist = pend * 8 192 - (the source's offset in the stream)."""
    out = []
    W = 32768
    vld = W - BLK - 4
    spec = _spec(2, 32768, dict_size=W, hash_bits=20)

    def build(n_blocks, src_blk, src_off, pend, key_id, eq=24, key=None):
        """blocks: the source (quiet) at src_blk, `bad` at pend, the quiet test block at pend + 1, quiet blocks elsewhere: one
        DT_ENTROPY run up to pend, compressed (the source's key inserted, and nothing else) when the `bad` block is typed.  A
        key that does not fit into the source block goes on in the next one."""
        k = key if key is not None else key19(key_id, bytes(QUIET[:5]))
        kt = bytearray(k)
        if eq < len(kt):
            kt[eq] = _other(kt[eq])
        blocks = []
        for i in range(n_blocks):
            if i == src_blk:
                blocks.append(B.quiet(probes={src_off: k[:BLK - src_off]}))
            elif i == src_blk + 1 and src_off + len(k) > BLK:
                blocks.append(B.quiet(probes={0: k[BLK - src_off:]}))
            elif i == pend:
                blocks.append(B.bad())
            elif i == pend + 1:
                blocks.append(B.quiet(probes={1000: bytes(kt)}))
            else:
                blocks.append(B.quiet())
        return blocks

    # dist = vld_rge - 1, vld_rge, vld_rge + 1: pending run at 32 768, source at 8 196 -+ 1
    for nm, off, hit in (("vld-1", 5, 1), ("vld", 4, 0), ("vld+1", 3, 0)):
        dist = 4 * BLK - (BLK + off)
        claims = [("cand", 0, 5, {C_I: 1000, C_DIST: dist, C_VLD: vld, C_HIT: hit}), ("block", 0, 5, {B_DUP: hit})]
        out.append(Case(f"dup/dist/{nm}", b"".join(build(6, 1, off, 4, 200)), spec, [f"dup/dist/{nm}"], claims))
    # the source ends 18 / 19 bytes before wnd_size: climit comes from the window (source in block 3, pending run at 49 152)
    # (the key ends in zeros from its 19th byte on, what the window's slack holds: a compare that runs past wnd_size sees 24 equal bytes)
    for room, hit in ((19, 1), (18, 0)):
        claims = [("cand", 0, 7, {C_I: 1000, C_ROOM: room, C_CMP: W - room, C_HIT: hit, C_EQ: 24}), ("block", 0, 7, {B_DUP: hit})]
        out.append(Case(f"dup/window_end/{room}", b"".join(build(8, 3, BLK - room, 6, 0, key=key19(210)[:18] + bytes(6))), spec,
                        [f"dup/window_end/{room}"], claims))
    # wnd_curpos == dist (cmp_pos 0) and wnd_curpos == dist - 1 (cmp_pos wnd_size - 1): source at window position 0 / wnd_size - 1
    claims = [("cand", 0, 7, {C_I: 1000, C_CMP: 0, C_DIST: 2 * BLK, C_HIT: 1}), ("block", 0, 7, {B_DUP: 1})]
    out.append(Case("dup/wpos_eq_dist", b"".join(build(8, 4, 0, 6, 220)), spec, ["dup/wpos/eq_dist"], claims))
    k = bytes([PROBE, 0, 0, 0, 0, 0]) + bytes(QUIET[:5]) * 4   # what position wnd_size - 1 is hashed over: the byte and the slack's zeros
    claims = [("cand", 0, 7, {C_I: 1000, C_CMP: W - 1, C_DIST: 2 * BLK + 1, C_ROOM: 1, C_HIT: 0}), ("block", 0, 7, {B_DUP: 0})]
    out.append(Case("dup/wpos_eq_dist-1", b"".join(build(8, 3, BLK - 1, 6, 221, eq=12, key=k)), spec, ["dup/wpos/eq_dist-1"], claims))
    # the source one lap and two laps of the window back (dist < vld_rge: the table entry has been overwritten by nothing since)
    for laps, src_blk, pend in ((1, 5, 7), (2, 9, 11)):
        claims = [("cand", 0, pend + 1, {C_I: 1000, C_DIST: (pend - src_blk) * BLK - 500, C_HIT: 1}), ("block", 0, pend + 1, {B_DUP: 1})]
        out.append(Case(f"dup/laps/{laps}", b"".join(build(pend + 2, src_blk, 500, pend, 230 + laps)), spec, [f"dup/laps/{laps}"], claims))
    return out


def _hash6(b, bits):
    v = int.from_bytes(b[:4], "little")
    v2 = int.from_bytes(b[4:6], "little")
    return (((v ^ (v2 << 13)) & 0xFFFFFFFF) * 2654435761 & 0xFFFFFFFF) >> (32 - bits)


def _collider(key, same_bits, differ_bits=None):
    """six bytes, the first probed, with HASH6 of `same_bits` equal to the key's and (when given) that of `differ_bits` different"""
    alpha = QUIET + bytes([0x20, 0x30, 0x40, 0x50, 0x60, 0x70, PROBE])
    want = _hash6(key, same_bits)
    n = len(alpha)
    for first in (PROBE, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70):
        for x in range(n ** 5):
            b = bytes([first] + [alpha[(x // n ** j) % n] for j in range(5)])
            if b != key[:6] and _hash6(b, same_bits) == want and (differ_bits is None or _hash6(b, differ_bits) != _hash6(key, differ_bits)):
                return b
    raise AssertionError("no collider")


def table_cases(B):
    """the cases that hang on ONE table: slot 0 taken by a later position of the same hash, an empty slot against zero bytes,
    the pending run, a hit through the BT head alone and through HT6 alone, vetoed blocks between no-LZ neighbours"""
    out = []
    k = key19(300, bytes(QUIET[:5]))

    def blocks(mid, test_key=k):
        """source and `mid` are one DT_ENTROPY run, compressed when the `bad` block is typed; the test block sees `bad` pending"""
        return [B.quiet(probes={100: k}), mid, B.bad(), B.quiet(probes={1000: test_key})]

    # HT6 of 13 bits, bucket of 4: a later position with the same 13-bit hash takes slot 0; the source moves to slot 1, never probed
    spec = _spec(2, 1 << 20, hash_bits=13, hash_width=4)
    col = _collider(k, 13)
    out.append(Case("dup/slot0_taken", b"".join(blocks(B.quiet(probes={200: col + bytes(QUIET[:3])}))), spec, ["dup/slot0_taken"],
                    [("cand", 0, 3, {C_I: 1000, C_TABLE: 0, C_DIST: 2 * BLK - (BLK + 200), C_HIT: 0}), ("block", 0, 3, {B_DUP: 0})]))
    out.append(Case("dup/slot0_kept", b"".join(blocks(B.quiet())), spec, ["dup/slot0_kept"],
                    [("cand", 0, 3, {C_I: 1000, C_TABLE: 0, C_DIST: 2 * BLK - 100, C_HIT: 1}), ("block", 0, 3, {B_DUP: 1})]))
    # an empty slot in the first chunk: dist = pos_ - 0 >= vld_rge whatever the block holds -- 19 zero bytes at a probed offset
    z = B.quiet(probes={1000: bytes(24)})
    out.append(Case("dup/empty_slot_zeros", b"".join([B.normal(), B.bad(), z]), _spec(2), ["dup/empty_slot"],
                    [("cand", 0, 2, {C_I: 1000, C_HIT: 0, C_DIST: (1 << 20) + 10240 - BLK - 4 + BLK}), ("block", 0, 2, {B_DUP: 0})]))
    # the copy inside the PENDING run (not compressed yet: not found) and the same copy one run earlier (found)
    src = B.quiet(probes={100: k})
    out.append(Case("dup/in_pending_run", b"".join([B.normal(), src, B.quiet(probes={1000: k})]), _spec(2), ["dup/pending_run"],
                    [("block", 0, 2, {B_AN: DT_ENTROPY, B_DUP: 0, B_FINAL: DT_ENTROPY}), ("nruns", 0, 2)]))
    out.append(Case("dup/one_run_earlier", b"".join([src, B.normal(), B.quiet(probes={1000: k})]), _spec(2), ["dup/one_run_earlier"],
                    [("block", 0, 2, {B_AN: DT_ENTROPY, B_DUP: 1, B_FINAL: DT_NORMAL}), ("cand", 0, 2, {C_I: 1000, C_HIT: 1})]))
    # the source inside an LZ-coded run that has JUST been compressed (in the inserter forms by another wavefront) when the test
    # block is typed: [normal with the key][bad][test] -- the `bad` block's typing compresses the normal run, the test block is next
    n = bytearray(B.normal())
    n[5000:5000 + len(k)] = k
    assert B.o.analyze(bytes(n))[0] == DT_NORMAL
    out.append(Case("dup/behind_lz_run", b"".join([bytes(n), B.bad(), B.quiet(probes={1000: k})]), _spec(2), ["dup/behind_lz_run"],
                    [("block", 0, 2, {B_AN: DT_ENTROPY, B_DUP: 1, B_FINAL: DT_NORMAL}), ("cand", 0, 2, {C_I: 1000, C_DIST: BLK - 5000, C_HIT: 1})]))
    # BT + HT6 (the adv_generic row): HT6 slot 0 taken, the BT head still the source -- and the other way round
    spec = _spec(5, 1 << 20, hash_width=4, hash_bits=13, bt_hash_bits=20)
    col = _collider(k, 13, 20)
    out.append(Case("dup/bt_head_only", b"".join(blocks(B.quiet(probes={200: col + bytes(QUIET[:3])}))), spec, ["dup/bt_head_only"],
                    [("cand", 0, 3, {C_I: 1000, C_TABLE: 0, C_DIST: BLK - 200, C_HIT: 0}), ("cand", 0, 3, {C_I: 1000, C_TABLE: 1, C_DIST: 2 * BLK - 100, C_HIT: 1}),
                     ("block", 0, 3, {B_DUP: 1})]))
    spec = _spec(5, 1 << 20, hash_width=4, hash_bits=20, bt_hash_bits=13)
    col = _collider(k, 13, 20)
    out.append(Case("dup/ht6_only", b"".join(blocks(B.quiet(probes={200: col + bytes(QUIET[:3])}))), spec, ["dup/ht6_only"],
                    [("cand", 0, 3, {C_I: 1000, C_TABLE: 0, C_DIST: 2 * BLK - 100, C_HIT: 1}), ("block", 0, 3, {B_DUP: 1})]))
    # a block vetoed to DT_NORMAL between two DT_BAD blocks: three runs; and a vetoed delta block
    r1 = B.bad()
    at = next(i for i in range(200, BLK) if r1[i] & 15 == 0)
    t = bytearray(B.bad())
    t[3000:3000 + 40] = r1[at:at + 40]
    out.append(Case("dup/veto_between_bad", b"".join([r1, B.normal(), B.bad(), bytes(t), B.bad()]), _spec(2), ["dup/veto/bad"],
                    [("block", 0, 3, {B_AN: DT_BAD, B_DUP: 1, B_FINAL: DT_NORMAL}),
                     ("runs", 0, [(DT_BAD, 0, BLK, 0), (DT_NORMAL, BLK, BLK, 0), (DT_BAD, 2 * BLK, BLK, 0), (DT_NORMAL, 3 * BLK, BLK, 0), (DT_BAD, 4 * BLK, BLK, 1)])]))
    d1 = B.dlt(1)
    at = next(i for i in range(200, BLK) if d1[i] & 15 == 0)
    t = bytearray(B.dlt(1))
    t[3001:3001 + 40] = d1[at:at + 40]
    t = bytes(t)
    assert B.o.analyze(t)[0] == DT_DLT + 1
    out.append(Case("dup/veto_delta", b"".join([d1, B.normal(), B.bad(), t, B.dlt(1)]), _spec(2), ["dup/veto/delta"],
                    [("block", 0, 3, {B_AN: DT_DLT + 1, B_BPB95: DT_DLT + 1, B_DUP: 1, B_FINAL: DT_NORMAL})]))
    return out


FAMILIES = (("types", types_cases), ("skip", skip_cases), ("bpb95", bpb95_cases), ("runs", runs_cases), ("dup", dup_cases),
            ("dup", window_cases), ("dup", table_cases))


def all_cases(orc_lib):
    """every case, in a fixed order; `orc_lib` is the oracle (ctypes CDLL)"""
    o = Orc(orc_lib)
    out = []
    for _, make in FAMILIES:
        out += make(Blocks(o))
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


# the hit and near-miss cases of the duplicate check that hang on no particular table: these run in every kernel form
FORM_CASES = ("dup/equal18", "dup/equal19", "dup/at_size-19", "dup/at_size-18", "dup/only_probe/lane0", "dup/only_probe/lane63",
              "dup/only_probe/round2", "dup/only_probe/last_round", "dup/no_probe", "dup/in_pending_run", "dup/one_run_earlier",
              "dup/behind_lz_run", "dup/veto_between_bad", "dup/veto_delta")

def in_form(case, variant):
    """the case under another props row: `variant` is (level, overrides) of tests/test_gpu_forms.py FORMS; dictionary 1 MiB"""
    level, over = variant
    return case._replace(spec={"level": level, "dict": 1 << 20, "props": dict(over)})


def dup_claims(case):
    """the duplicate verdicts a case claims, which hold in every props row: [(chunk, block, verdict)]"""
    return [(cl[1], cl[2], cl[3][B_DUP]) for cl in case.claims if cl[0] == "block" and B_DUP in cl[3]]


COVERAGE = tuple(
    [f"types/verdict/{n}" for n in TYPE_OF]
    + [f"types/pair/{a}>{b}" for a in MAIN_TYPES for b in MAIN_TYPES]
    + ["types/fast_splits_a_normal_run"]
    + [f"types/switch_off/{s}" for s in ("D", "T", "E", "DT", "DE", "TE", "DTE")]
    + [f"skip/{n}/{t}" for n in MAIN_TYPES for t in TAILS]
    + ["skip/alone/1", "skip/alone/511"]
    + [f"skip/second_chunk/{n}/{t}" for n in ("dlt2", "bad", "entropy") for t in TAILS[:5]]
    + [f"skip/in_second_chunk/dlt2/{t}" for t in (1, 19, 511)]
    + ["bpb95/under", "bpb95/on", "bpb95/over"]
    + ["runs/exactly_raw/normal", "runs/exactly_raw/bad", "runs/same_type_across_chunks/normal", "runs/same_type_across_chunks/bad",
       "runs/raw_not_a_multiple", "runs/type_change/first", "runs/type_change/last"]
    + ["dup/equal/18", "dup/equal/19", "dup/limit/19", "dup/limit/18", "dup/only_probe/lane0", "dup/only_probe/lane63",
       "dup/only_probe/round2", "dup/only_probe/last_round", "dup/no_probe", "dup/dist/vld-1", "dup/dist/vld", "dup/dist/vld+1",
       "dup/window_end/19", "dup/window_end/18", "dup/wpos/eq_dist", "dup/wpos/eq_dist-1", "dup/laps/1", "dup/laps/2",
       "dup/slot0_taken", "dup/slot0_kept", "dup/empty_slot", "dup/pending_run", "dup/one_run_earlier", "dup/behind_lz_run", "dup/bt_head_only",
       "dup/ht6_only", "dup/veto/bad", "dup/veto/delta"])


# ---- claims against a trace ------------------------------------------------------------------------------------------------

def _rows(rows, chunk, block=None):
    return [r for r in rows if r[0] == chunk and (block is None or r[1] == block)]


def failed_claims(case, tr):
    """the claims of a case its trace does not show, as strings (empty: all hold)"""
    bad = []
    for cl in case.claims:
        kind = cl[0]
        if kind == "block":
            _, ch, blk, want = cl
            rows = _rows(tr.blocks, ch, blk)
            if len(rows) != 1 or any(rows[0][k] != v for k, v in want.items()):
                bad.append(f"{cl} -- trace {rows}")
        elif kind == "cand":
            _, ch, blk, want = cl
            if not any(all(r[k] == v for k, v in want.items()) for r in _rows(tr.cands, ch, blk)):
                bad.append(f"{cl} -- candidates {[r for r in _rows(tr.cands, ch, blk) if r[C_I] == want.get(C_I, r[C_I])][:4]}")
        elif kind == "ncands":                              # offsets probed in a block
            _, ch, blk, n = cl
            got = len({r[C_I] for r in _rows(tr.cands, ch, blk)})
            if got != n:
                bad.append(f"{cl} -- {got} probed offsets")
        elif kind == "runs":
            _, ch, want = cl
            got = [r[1:] for r in _rows(tr.runs, ch)]
            if got != [tuple(w) for w in want]:
                bad.append(f"{cl} -- runs {got}")
        elif kind == "nruns":
            _, ch, n = cl
            if len(_rows(tr.runs, ch)) != n:
                bad.append(f"{cl} -- runs {_rows(tr.runs, ch)}")
        elif kind == "nchunks":
            if len({r[0] for r in tr.runs}) != cl[1]:
                bad.append(f"{cl} -- runs {tr.runs}")
        elif kind == "inherits":                            # a DT_SKIP block takes the previous block's final type and keeps its bpb
            _, ch, blk = cl
            prev, cur = _rows(tr.blocks, ch, blk - 1)[0], _rows(tr.blocks, ch, blk)[0]
            if cur[B_AN] != DT_SKIP or cur[B_SKIP] != prev[B_FINAL] or cur[B_BPB] != prev[B_BPB]:
                bad.append(f"{cl} -- {prev} {cur}")
            if prev[B_FINAL] >= DT_DLT and cur[B_DLT_USED] != cur[B_DLT5 + prev[B_FINAL] - DT_DLT]:
                bad.append(f"{cl} -- GetDltBpb did not run on the tail: {cur}")
        elif kind == "analyzed":
            _, ch, blk = cl
            if _rows(tr.blocks, ch, blk)[0][B_AN] == DT_SKIP:
                bad.append(f"{cl}")
        elif kind == "bpb95":
            _, ch, blk, side = cl
            r = _rows(tr.blocks, ch, blk)[0]
            gap = r[B_DLT_USED] - r[B_BPB] * 0.95
            ok = {"under": -1.0 < gap < 0, "on": gap == 0.0, "over": 0 < gap < 1.0}[side]
            if not ok:
                bad.append(f"{cl} -- bpb {r[B_BPB]} GetDltBpb {r[B_DLT_USED]}")
        else:
            raise KeyError(kind)
    return bad


# ---- plain-Python restatements, with room for one planted mistake each ------------------------------------------------------

def walk(blocks, raw_blocksize, switches, mistake=None):
    """CSCEncoder::Compress over the trace's block rows of a STREAM (analyzer type, bpb, five GetDltBpb figures, duplicate
    verdict; chunks in order): the run list [(chunk, type, offset, size, tail)].  `switches` = (DLT, TXT, EXE).  The duplicate
    verdict is taken from the row when the row has one (a mistake that asks where the reference did not gets "no")."""
    dlt_on, txt_on, exe_on = switches
    use = (dlt_on + txt_on + exe_on) != 0
    runs = []
    last_type, last_begin, last_size, bpb, chunk = DT_NORMAL, 0, 0, 0, None
    for r in list(blocks) + [None]:
        if r is None or r[B_CHUNK] != chunk:
            merged = mistake == "merge_across_chunks" and r is not None and chunk is not None
            if last_size and not merged:
                runs.append((chunk, last_type, last_begin, last_size, 1))
                last_size = 0
            if r is None:
                break
            if not merged:
                last_type, last_begin, bpb = DT_NORMAL, 0, 0
            chunk = r[B_CHUNK]
        i, cur = r[B_OFF], r[B_SIZE]
        t = r[B_AN] if use else DT_NORMAL
        if t != DT_SKIP:
            bpb = r[B_BPB]
        elif mistake == "bpb_cleared_on_skip":
            bpb = 0
        if t == DT_SKIP:
            t = last_type

        def switch(t):
            if t == DT_EXE and not exe_on or t == DT_ENGTXT and not txt_on or t >= DT_DLT and not dlt_on:
                return DT_NORMAL
            return t

        def rule95(t):
            if t >= DT_DLT:
                d = r[B_DLT5 + t - DT_DLT]
                if (d > bpb * 0.95) if mistake == "gt_at_095" else (d >= bpb * 0.95):
                    return DT_NORMAL
            return t
        t = switch(rule95(t)) if mistake == "switches_after_delta_rule" else rule95(switch(t))
        if t >= DT_NO_LZ and r[B_DUP] == 1:
            t = DT_NORMAL
        if mistake == "fast_merged" and t == DT_FAST:       # coded as normal, so taken for normal one step early
            t = DT_NORMAL
        over = (last_size + cur >= raw_blocksize) if mistake == "ge_at_raw_blocksize" else (last_size + cur > raw_blocksize)
        if last_type != t or over:
            if last_size:
                runs.append((chunk, last_type, last_begin, last_size, 0))
            last_begin, last_size = i, 0
        last_type = t
        last_size += cur
    return runs


def test_find_verdict(cands, mistake=None):
    """MatchFinder::TestFind over one block's candidate rows: true when one of them is in range and has more than 18 equal
    bytes before min(limit, wnd_size - cmp_pos)"""
    for c in cands:
        dist, vld, limit, room, eq = c[C_DIST], c[C_VLD], c[C_LIMIT], c[C_ROOM], c[C_EQ]
        if (dist > vld) if mistake == "dist_gt_vld" else (dist >= vld):
            continue
        if mistake == "wpos_gt_dist" and c[C_CMP] == 0:     # wpos == dist taken for the wrapping side: cmp_pos = wnd_size, no room
            room = 0
        climit = limit if mistake == "climit_without_window" else min(limit, room)
        n = min(eq, climit)
        if (n >= 18) if mistake == "ge_18" else (n > 18):
            return True
    return False


def digest(b):
    return hashlib.sha256(b).hexdigest()


def golden_entry(stream, dec):
    """the JSON-able line of one case: sizes, digests, the reference decoder's answer, small streams whole"""
    ent = {"stream_size": len(stream), "stream_sha256": digest(stream), "dec_rc": dec[0], "dec_sha256": digest(dec[1])}
    if len(stream) <= 1200:
        ent["stream_hex"] = stream.hex()
    return ent
