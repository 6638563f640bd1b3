"""Seeded SCRIPT generator for the stream synthesizer (oracle/orc_synth.c), shared by tests/test_synth_gen.py,
tests/test_gpu_synth.py and tools/make_golden_synth.py.  Not a conftest: a plain module like soak_gen.

The decoders are otherwise tested on streams an encoder wrote.  Here a script says packet by packet what to code, and
this module simulates the decoder's window (numpy) while it draws the packets, so every case comes with the PREDICTED
answer of the reference decoder: (rc, bytes delivered).  A case is a dict
  meta     one JSON-able line: family, seed, index, name, header geometry (dict, bsize, raw)
  script   numpy uint32 words for orc_synth        rc, out   the prediction        cover   the coverage cells it hit
and `stream(orc, case)` is header + orc_synth(script).  Every assertion message should carry `describe(case)`.

Families (FAMILIES gives the fixed seeds): walk, lengths, distances, edges, blocks, geometry, refused, long_chain, long_rle,
filters (adversarial bytes in DT_ENGTXT / DT_EXE runs; predicted by the restated inverse filters further down).
`coverage(cases)` is the union of the cells; tests/test_synth_gen.py writes out what "complete" means.

Kept out ON PURPOSE, because the REFERENCE decoder runs past its own buffers on them, so there is nothing to compare
with; the simulator makes them impossible by construction (Sim refuses to draw them, nothing is filtered afterwards):
  * a literal or a one-byte rep match at i == limit (the loop runs while i <= limit, the run's buffer holds limit bytes);
  * a DT_ENGTXT run whose expansion exceeds raw_blocksize (outside the `filters` family ENGTXT / EXE runs only carry
    orc_forward_dict / orc_forward_e89 of corpus data, whose inverse is the corpus data);
  * a DT_ENGTXT run on which Inverse_Dict reads src[i] at i >= size: an escape marker spends two source bytes on one output
    byte, so a run with more markers than its word symbols pay for is read past its end -- stale memory.  txt_source()
    puts four-letter symbols early in a run until the highest index read is below the run's size, and asserts it;
  * a copy with distance >= wnd_size;
  * a match of length 2 at distance 65 (that IS the end-of-run marker), and distances the length context has no slot for
    (length 2: > 64, lengths 3 and 4: > 16 385).
"""
import ctypes as C
import hashlib
import json
import random

import numpy as np

import filter_cases
from csc_amd import corpus
from csc_amd.capi import BytesWriter, CSCProps, DECODE_ERROR

(OP_BLOCK, OP_LIT, OP_MATCH, OP_REP, OP_REP0LEN1, OP_END_RUN, OP_RESTART, OP_BAD, OP_ENTROPY, OP_DLT, OP_RLE_LIT,
 OP_RLE_RUN, OP_EOF, OP_RAW_TYPE, OP_LITS, OP_FLUSH) = range(1, 17)
DT_NORMAL, DT_ENGTXT, DT_EXE, DT_ENTROPY, DT_BAD, SIG_EOF, DT_DLT = 1, 2, 3, 7, 8, 9, 0x10
DLT_CHN = [1, 2, 3, 4, 8]
T = [0, 1, 2, 3] + [(1 << k) + 1 for k in range(2, 31)]          # first coded distance (= distance - 1) of each slot
KB, MB = 1 << 10, 1 << 20
BSIZE, RAW = 64 * KB, 2 * MB                                        # CSCEncProps_Init's csc_blocksize / raw_blocksize
SEED = int(corpus.SEED_ENWIK9)

FAMILIES = {"walk": [11, 12], "lengths": [21], "distances": [31], "edges": [41, 42], "blocks": [51, 52],
            "geometry": [61], "refused": [71, 72], "long_chain": [81], "long_rle": [91], "filters": [101]}


def len_ctx(length):
    """the distance model's context of a match length (decode_match): coded length 0, 1, 2, 3, 4, 5, 6 and above"""
    return min(length - 2, 6)


def max_dist(length):
    """the largest distance the coding has a slot for under this length (one less for length 2: 65 is the end marker)"""
    return 64 if length == 2 else 16385 if length <= 4 else (1 << 30) + 1


def slot_of(d):
    k = 0
    while k + 1 < len(T) and T[k + 1] <= d:
        k += 1
    return k


def slot_edges(d):
    """which edges of its slot a coded distance is: 'lo' (first), 'lo1' (second), 'hi' (last)"""
    k = slot_of(d)
    e = []
    if d == T[k]:
        e.append("lo")
    if d == T[k] + 1 and T[k + 1] - T[k] >= 2:
        e.append("lo1")
    if d == T[k + 1] - 1 and T[k + 1] - T[k] >= 2:
        e.append("hi")
    return k, e


def len_class(n):
    for name, lo, hi in (("2..17", 2, 17), ("142..146", 142, 146), ("285..288", 285, 288), ("8191..8194", 8191, 8194)):
        if lo <= n <= hi:
            return f"{n}"
    return "65536" if n == 65536 else "1MiB" if n == MB else None


class Sim:
    """The decoder's window, rep distances, state and run counter, restated from the format alone; collects the script,
    the predicted output and the coverage cells.  Every drawing method asserts legality: a generator bug, never a case."""

    def __init__(self, dict_size, bsize=BSIZE, raw=RAW):
        self.wnd_size, self.bsize, self.raw = dict_size, bsize, raw
        self.wnd = np.zeros(dict_size + 8, np.uint8)          # + slack, zero like the zeroing allocator's
        self.cur = 0
        self.rep = [0, 0, 0, 0]
        self.state = 0
        self.i = None                                         # bytes of the open LZ run (None: no run open)
        self.s = []
        self.out = []                                         # delivered runs
        self.run = []
        self.cover = set()
        self.wrapped = False
        self.rc = 0
        self.done = False
        self.flt = None
        self.packets = 0
        self._wrap_in_run = False

    # -- legality ---------------------------------------------------------------------------------------------
    def src(self, dist):
        return self.cur - dist if self.cur >= dist else self.cur + self.wnd_size - dist

    def why_not(self, dist, n):
        """None when a copy (dist, n) is legal now, else the name of the reference check that refuses it"""
        assert 0 <= dist < self.wnd_size and n >= 2
        if self.src(dist) + n > self.wnd_size:
            return "src"
        if n + self.i > self.raw:
            return "limit"
        if self.cur + n > self.wnd_size:
            return "dst"
        return None

    def room(self):
        """the longest copy the destination side allows now"""
        return min(self.raw - self.i, self.wnd_size - self.cur)

    # -- LZ packets -------------------------------------------------------------------------------------------
    def _kind(self, k):
        self.cover.add(("state", self.state, k))
        self.state = (self.state * 4 + k) & 63
        self.packets += 1

    def _advance(self, n):
        self.run.append(self.wnd[self.cur:self.cur + n].copy())
        self.cur += n
        self.i += n
        assert self.cur <= self.wnd_size and self.i <= self.raw
        if self.cur == self.wnd_size:
            self.cur = 0
            self.wrapped = True
            self.cover.add(("edge", "wrap"))
            self._wrap_in_run = True

    def lit(self, b):
        assert self.i < self.raw
        if self._wrap_in_run:
            self.cover.add(("edge", "wrap_inside_run"))
        self._kind(0)
        self.wnd[self.cur] = b
        self.s += [OP_LIT, int(b)]
        self._advance(1)

    def _copy(self, dist, n):
        a = self.src(dist)
        if dist > self.cur and not self.wrapped:
            self.cover.add(("edge", "source_never_written"))
        if a + n == self.wnd_size:
            self.cover.add(("edge", "src_ends_at_wnd"))
        if self.cur + n == self.wnd_size:
            self.cover.add(("edge", "dst_ends_at_wnd"))
        if self.i + n == self.raw:
            self.cover.add(("edge", "packet_ends_at_limit"))
        if self._wrap_in_run:
            self.cover.add(("edge", "wrap_inside_run"))
        if 0 < dist < n and a < self.cur:                      # overlapping forward copy replicates the last dist bytes
            self.wnd[self.cur:self.cur + n] = np.resize(self.wnd[a:a + dist].copy(), n)
        elif dist:
            self.wnd[self.cur:self.cur + n] = self.wnd[a:a + n].copy()
        last = int(self.wnd[self.cur + n - 1])
        return last

    def match(self, dist, n):
        assert 1 <= dist < self.wnd_size and dist <= max_dist(n) and self.why_not(dist, n) is None, (dist, n)
        k, edges = slot_edges(dist - 1)
        for e in edges:
            self.cover.add(("dist", len_ctx(n), k, e))
        self.cover.add(("len", "match", len_class(n)))
        if n <= dist <= self.cur:
            self.cover.add(("far_source", "match", len_class(n)))
        if dist in (1, 2, 3, 63, 64, 65) or n - 1 <= dist <= n + 1:
            self.cover.add(("overlap", "match", len_class(n), dist if dist in (1, 2, 3, 63, 64, 65) else dist - n))
        self._kind(1)
        self.rep = [dist] + self.rep[:3]
        last = self._copy(dist, n)
        self.s += [OP_MATCH, dist, n, last]
        self._advance(n)

    def repm(self, idx, n):
        dist = self.rep[idx]
        assert self.why_not(dist, n) is None, (dist, n)
        self.cover.add(("rep", self.state, idx))
        self.cover.add(("len", "rep", len_class(n)))
        if n <= dist <= self.cur:
            self.cover.add(("far_source", "rep", len_class(n)))
        if dist == 0:
            self.cover.add(("edge", "rep_distance_zero"))
        if dist in (1, 2, 3, 63, 64, 65) or n - 1 <= dist <= n + 1:
            self.cover.add(("overlap", "rep", len_class(n), dist if dist in (1, 2, 3, 63, 64, 65) else dist - n))
        self._kind(3)
        self.rep.insert(0, self.rep.pop(idx))
        last = self._copy(dist, n)
        self.s += [OP_REP, idx, n, last]
        self._advance(n)

    def rep1(self):
        assert self.i < self.raw
        if self.cur == self.rep[0]:
            self.cover.add(("edge", "rep1_at_curpos_eq_rep0" + ("_after_wrap" if self.wrapped else "")))
        if self.packets == 0:
            self.cover.add(("edge", "rep1_first_packet"))
        self._kind(2)
        a = self.cur - self.rep[0] if self.cur > self.rep[0] else self.cur + self.wnd_size - self.rep[0]
        self.wnd[self.cur] = self.wnd[a]
        self.s += [OP_REP0LEN1, int(self.wnd[self.cur])]
        self._advance(1)

    # -- runs and blocks --------------------------------------------------------------------------------------
    def begin(self, typ=DT_NORMAL, flt=None, size_field=0):
        assert self.i is None and not self.done
        self.s += [OP_BLOCK, typ] + ([size_field] if typ == DT_ENGTXT else [])
        self.i, self.run, self.flt, self._wrap_in_run = 0, [], flt, False
        self.cover.add(("block", typ))

    def end(self, restart):
        """END_RUN + the restart flag.  A run of zero bytes ends the stream like SIG_EOF."""
        self.s += [OP_END_RUN]
        self.cover.add(("end_run", self.state))               # coded like a match, counted apart: no copy comes out of it
        self.state = (self.state * 4 + 1) & 63
        n = self.i
        if n == self.raw:
            self.cover.add(("edge", "run_of_exactly_raw_blocksize"))
        got = np.concatenate(self.run) if self.run else np.zeros(0, np.uint8)
        self.i = None
        if n == 0:
            self.cover.add(("edge", "zero_byte_run"))
            self.s += [OP_RESTART, 0, OP_FLUSH]
            self.done = True
            return
        self.out.append(self.flt if self.flt is not None else got)
        if self.flt is not None:
            assert len(self.flt) == n
        self._restart(restart)

    def _restart(self, restart):
        self.cover.add(("restart", int(bool(restart))))
        self.s += [OP_RESTART, 1 if restart else 0]

    def _to_dict(self, b):
        n, p = len(b), 0
        while p < n:
            c = min(self.wnd_size - self.cur, n - p)
            self.wnd[self.cur:self.cur + c] = b[p:p + c]
            self.cur = (self.cur + c) % self.wnd_size if self.cur + c >= self.wnd_size else self.cur + c
            if self.cur == 0:
                self.wrapped = True
            p += c

    def raw_block(self, typ, data, restart):
        """DT_BAD / DT_ENTROPY: bytes coded directly / under the literal model, then copied into the window"""
        assert self.i is None and 0 < len(data) <= self.raw and typ in (DT_BAD, DT_ENTROPY)
        b = np.frombuffer(bytes(data), np.uint8)
        pad = bytes(data) + b"\0" * (-len(data) % 4)
        self.s += [OP_BLOCK, typ, OP_BAD if typ == DT_BAD else OP_ENTROPY, len(b)] + np.frombuffer(pad, "<u4").tolist()
        self.cover.add(("block", typ))
        if len(b) == self.raw:
            self.cover.add(("edge", "size_field_eq_max", typ))
        self._to_dict(b)
        self.out.append(b)
        self._restart(restart)

    def dlt_block(self, ci, n, items, restart):
        """DT_DLT + ci: size field n, then items ('lit', byte) / ('run', length >= 11); runs are clipped at n"""
        assert self.i is None and 0 < n <= self.raw
        self.s += [OP_DLT, DT_DLT + ci, n]
        self.cover.add(("block", DT_DLT + ci))
        dst = np.zeros(n, np.uint8)
        i = 0
        for kind, v in items:
            assert i < n
            if kind == "lit":
                dst[i] = v
                i += 1
                self.s += [OP_RLE_LIT, int(v)]
            else:
                assert i > 0 and v >= 11
                if i == 1:
                    self.cover.add(("edge", "rle_run_at_1"))
                if v > n - i:
                    self.cover.add(("edge", "rle_run_clipped"))
                if v - 11 > UNDO_CAP_BITS * 143:
                    self.cover.add(("edge", "rle_run_above_undo_cap"))
                c = min(v, n - i)
                dst[i:i + c] = dst[i - 1]
                i += c
                self.s += [OP_RLE_RUN, int(v)]
        assert i == n
        if n == self.raw:
            self.cover.add(("edge", "size_field_eq_max", DT_DLT))
        if n >= 512:                                          # Filters::Inverse_Delta leaves shorter blocks alone
            chn = DLT_CHN[ci]
            order = np.concatenate([np.arange(c, n, chn) for c in range(chn)])
            res = np.zeros(n, np.uint8)
            res[order] = np.cumsum(dst, dtype=np.uint64).astype(np.uint8)
            dst = res
            self.cover.add(("edge", "delta_inverse", chn))
        self._to_dict(dst)
        self.out.append(dst)
        self._restart(restart)

    def eof(self):
        """SIG_EOF.  The coder restarts before it whatever the family's flag policy says, as after an encoder's last block:
        without that the decoder's last flag read can run into the end of the last BC block (READ_ERROR after the last byte)."""
        assert self.i is None and not self.done and self.s[-2] == OP_RESTART
        self.s[-1] = 1
        self.s += [OP_EOF]
        self.done = True

    def refuse(self, name, ops, rc):
        """the stream ends in something the reference refuses before any byte of this run or block is delivered"""
        self.cover.add(("refused", name))
        self.s += list(ops) + [OP_FLUSH]
        self.rc, self.done, self.i = rc, True, None

    def case(self, meta):
        assert self.done
        out = np.concatenate(self.out).tobytes() if self.out else b""
        meta = dict(meta, dict=self.wnd_size, bsize=self.bsize, raw=self.raw)
        return {"meta": meta, "script": np.array(self.s, np.uint32), "rc": self.rc, "out": out, "cover": self.cover}


# ---- drawing helpers ---------------------------------------------------------------------------------------------------

def draw_len(rng, cap):
    r = rng.random()
    n = rng.randrange(2, 18) if r < 0.6 else rng.randrange(18, 300) if r < 0.9 else rng.randrange(300, 6000)
    return min(n, cap)


def draw_dist(sim, rng, n):
    """a distance that is legal for a copy of n now (None if there is none among a few draws)"""
    hi = min(max_dist(n), sim.wnd_size - 1)
    for _ in range(8):
        r = rng.random()
        d = rng.randrange(1, min(hi, 70) + 1) if r < 0.4 else rng.randrange(1, min(hi, max(sim.cur, 2)) + 1) if r < 0.8 \
            else rng.randrange(1, hi + 1)
        if sim.why_not(d, n) is None:
            return d
    return None


def walk(sim, rng, packets, kinds=(0, 1, 2, 3)):
    """`packets` random packets in the open run; stops early when the run or the window leaves no room"""
    for _ in range(packets):
        if sim.raw - sim.i < 2:
            break
        k = rng.choice(kinds)
        cap = sim.room()
        if k == 1 and cap >= 2:
            n = draw_len(rng, cap)
            d = draw_dist(sim, rng, n)
            if d is not None:
                sim.match(d, n)
                continue
        if k == 3 and cap >= 2:
            idx = rng.randrange(4)
            n = draw_len(rng, cap)
            while n >= 2 and sim.why_not(sim.rep[idx], n) is not None:
                n //= 2
            if n >= 2:
                sim.repm(idx, n)
                continue
        if k == 2:
            sim.rep1()
            continue
        sim.lit(rng.randrange(256) if rng.random() < 0.7 else rng.choice(b"etaoin \n"))


def rep1_at_rep0(sim, rng):
    """a match that ends exactly at curpos == its own distance (its source ends at wnd_size), then the one-byte rep"""
    n = rng.randrange(5, 20)
    d = sim.cur + n
    if d < sim.wnd_size and sim.i + n + 1 <= sim.raw and sim.why_not(d, n) is None:
        sim.match(d, n)
        sim.rep1()


def fill_to(sim, rng, target, restart=lambda: 0):
    """cheap output up to window position `target` (< wnd_size) without wrapping: literals, then long matches at a
    distance of a few thousand, in as many runs as the run limit needs; leaves a run open"""
    assert sim.cur <= target < sim.wnd_size
    if sim.i is None:
        sim.begin()
    while sim.cur < target:
        if sim.raw - sim.i < 2:
            if sim.raw - sim.i == 1:
                sim.lit(rng.randrange(256))
            sim.end(restart())
            sim.begin()
            continue
        if sim.cur < 3000 or target - sim.cur < 2:
            sim.lit(rng.randrange(256))
            continue
        n = min(target - sim.cur, sim.raw - sim.i, rng.randrange(2000, 300000))
        sim.match(rng.randrange(1000, 3000), n) if n >= 5 else sim.lit(rng.randrange(256))


def lits(sim, rng, n):
    for _ in range(n):
        if sim.raw - sim.i < 1:
            break
        sim.lit(rng.randrange(256))


def emit(sim, rng, data):
    """an LZ run's worth of given bytes: literals, and matches / one-byte reps where the window already holds them"""
    last = {}
    p, n = 0, len(data)
    base = sim.cur
    assert base + n <= sim.wnd_size
    while p < n:
        key = bytes(data[p:p + 3])
        q = last.get(key)
        if q is not None and p + 3 <= n and rng.random() < 0.8:
            d = p - q
            m = 3
            while p + m < n and m < 200 and data[p + m] == data[q + m]:
                m += 1
            if d <= max_dist(m) and sim.why_not(d, m) is None:
                sim.match(d, m)
                last[key] = p
                p += m
                continue
        if sim.rep[0] and p >= sim.rep[0] and data[p] == data[p - sim.rep[0]] and rng.random() < 0.5:
            sim.rep1()
        else:
            sim.lit(data[p])
        last[key] = p
        p += 1
    assert bytes(sim.wnd[base:base + n]) == bytes(data)


def filtered(orc, kind, rng, n):
    """(plain, forward-filtered) corpus bytes of n: 'exe' through orc_forward_e89, 'text' through orc_forward_dict"""
    for _ in range(20):
        plain = corpus.fill(kind, SEED, rng.randrange(0, 500_000_000), n).tobytes()
        buf = (C.c_uint8 * n).from_buffer_copy(plain)
        if kind == "exe":
            orc.orc_forward_e89(buf, n)
            return plain, bytes(buf)
        orc.orc_forward_dict.restype = C.c_uint32
        if orc.orc_forward_dict(buf, n):
            return plain, bytes(buf)
    raise AssertionError("orc_forward_dict refused 20 stretches of corpus text")


def flag_of(mode, rng):
    return {"always": lambda: 1, "never": lambda: 0, "random": lambda: rng.randrange(2)}[mode]


# ---- the families ------------------------------------------------------------------------------------------------------

def fam_walk(seed, orc):
    out = []
    for idx, wnd in enumerate([32 * KB, 32 * KB, 64 * KB, 64 * KB + 77, 256 * KB, MB]):
        rng = random.Random(seed * 1000 + idx)
        sim = Sim(wnd)
        sim.begin()
        if idx % 2 == 0:
            sim.rep1()                                    # first packet of the stream: curpos == rep0 == 0
            sim.repm(rng.randrange(4), rng.randrange(2, 40))      # rep distance 0: the copy's source is its own destination
        for r in range(8):
            walk(sim, rng, 500)
            rep1_at_rep0(sim, rng)
            if sim.room() > 40000 and sim.cur > 3000:     # help the window round: one long match a run
                sim.match(rng.randrange(1, 3000), rng.randrange(20000, min(sim.room(), 200000)))
            if r % 3 == 2:
                lits(sim, rng, 1)
                sim.end(rng.randrange(2))
                sim.begin()
        lits(sim, rng, 1)
        sim.end(1)
        sim.eof()
        out.append(sim.case({"family": "walk", "seed": seed, "index": idx}))
    return out


LENGTHS = list(range(2, 18)) + list(range(142, 147)) + list(range(285, 289)) + list(range(8191, 8195)) + [65536, MB]
OVERLAPS = [1, 2, 3, 63, 64, 65]


def _one_length(sim, rng, n, dists, as_rep):
    for d in dists:
        lits(sim, rng, rng.randrange(1, 4))
        if d == "real":                                   # a source of written bytes at least n back: no overlap, no zeros
            if sim.cur < n + 100:
                fill_to(sim, rng, n + rng.randrange(100, 4000))
            d = rng.randrange(n, sim.cur + 1)
        if d > max_dist(5) or d >= sim.wnd_size or d < 1:
            continue
        if sim.raw - sim.i < n + 16 or (not as_rep and d > max_dist(n)):
            if sim.raw - sim.i < n + 16:
                sim.end(rng.randrange(2))
                sim.begin()
            if not as_rep and d > max_dist(n):
                continue
        if as_rep:
            if sim.why_not(d, 5) is not None:
                continue
            sim.match(d, 5)                               # plant the distance, push it down 0..3 places, call it back
            idx = rng.randrange(4)
            for k in range(idx):
                lits(sim, rng, 1)
                sim.match(rng.randrange(1, 60) + 70 * k, 3)
            lits(sim, rng, 1)
            if sim.why_not(sim.rep[idx], n) is None:
                sim.repm(idx, n)
        elif sim.why_not(d, n) is None:
            sim.match(d, n)


def fam_lengths(seed, orc):
    out = []
    for idx, n in enumerate(LENGTHS + ["end"]):
        rng = random.Random(seed * 1000 + idx)
        big = n == "end" or n >= 65536
        for as_rep in (False, True):
            if n == "end":
                sim = Sim(RAW + 64 * KB)
                sim.begin()
                lits(sim, rng, 3000)
                d = 1 if not as_rep else 2500
                if as_rep:
                    sim.match(d, 6); lits(sim, rng, 2)
                m = sim.raw - sim.i
                sim.repm(0, m) if as_rep else sim.match(d, m)
                sim.cover.add(("len", "rep" if as_rep else "match", "to_end"))
            else:
                dists = OVERLAPS + [n - 1, n, n + 1, "far"]
                if n == MB:
                    dists = ["far"] if as_rep else OVERLAPS
                if n >= 65536:
                    dists = dists + ["real"]
                total = 5000 + len(dists) * (n + 40) + (n + 8000 if n >= 65536 else 0)
                sim = Sim(max(32 * KB, total + 4096))
                sim.begin()
                lits(sim, rng, 3000)
                dists = [rng.randrange(1000, 2900) if d == "far" else d for d in dists]
                _one_length(sim, rng, n, dists, as_rep)
            lits(sim, rng, 1)
            sim.end(1)
            sim.eof()
            out.append(sim.case({"family": "lengths", "seed": seed, "index": 2 * idx + as_rep, "name": f"{n}/{'rep' if as_rep else 'match'}",
                                 "big": big}))
    return out


def dist_cells(wnd):
    """every (length context, slot, edge) whose distance fits a window of wnd: what `distances` must cover"""
    cells = set()
    for ctx in range(7):
        n = ctx + 2
        for k in range(0, 31):
            for d in (T[k], T[k] + 1, T[k + 1] - 1):
                if d + 1 <= min(max_dist(n), wnd - 1):
                    for e in slot_edges(d)[1]:
                        cells.add(("dist", ctx, k, e))
    return cells


def fam_distances(seed, orc):
    out = []
    for idx, (wnd, wrap) in enumerate([(32 * KB, False), (32 * KB + 1, True), (2 * MB + 4096, False), (2 * MB + 4096, True)]):
        rng = random.Random(seed * 1000 + idx)
        sim = Sim(wnd)
        sim.begin()
        if wrap:
            fill_to(sim, rng, wnd - 1)
            lits(sim, rng, 1) if sim.raw - sim.i >= 1 else None
            if sim.cur != 0:                              # (the run was full: finish the lap in a new one)
                sim.end(0); sim.begin(); lits(sim, rng, 1)
            assert sim.cur == 0 and sim.wrapped
        lits(sim, rng, 40)
        todo = sorted({(ctx, d) for ctx in range(7) for k in range(31) for d in (T[k], T[k] + 1, T[k + 1] - 1)
                       if d + 1 <= min(max_dist(ctx + 2), wnd - 1)}, key=lambda cd: (cd[1], cd[0]))
        todo.append((6, wnd - 2))                         # the largest legal distance: wnd_size - 1
        for ctx, d in todo:
            n = ctx + 2 if ctx < 6 else rng.randrange(8, 300)
            if sim.raw - sim.i < n + 600:
                sim.end(rng.randrange(2)); sim.begin()
            for _ in range(600):                          # a source that straddles curpos: step past it
                if sim.why_not(d + 1, n) is None:
                    break
                sim.lit(rng.randrange(256))
            sim.match(d + 1, n)
            if d + 1 == wnd - 1:
                sim.cover.add(("edge", "largest_distance" + ("_after_wrap" if sim.wrapped else "")))
            if rng.random() < 0.3:
                lits(sim, rng, 1)
        lits(sim, rng, 1)
        sim.end(1)
        sim.eof()
        out.append(sim.case({"family": "distances", "seed": seed, "index": idx, "big": wnd > MB}))
    return out


def _prefix(sim, rng, lo=0, hi=400):
    sim.begin()
    walk(sim, rng, rng.randrange(lo, hi))
    lits(sim, rng, 1)


def fam_edges(seed, orc):
    out = []

    def done(sim, idx, name):
        if sim.i is not None:
            if sim.i == 0 and name != "zero_byte_run":
                lits(sim, rng, 1)
            sim.end(1)
        if not sim.done:
            sim.eof()
        out.append(sim.case({"family": "edges", "seed": seed, "index": idx, "name": name}))

    for idx, name in enumerate(["src_ends_at_wnd", "dst_ends_at_wnd", "wrap_inside_long_run", "limit_match", "limit_rep",
                                "limit_lit", "limit_rep1", "raw_run_default", "zero_byte_run", "rle_at_1", "size_eq_max"]):
        rng = random.Random(seed * 1000 + idx)
        raw = rng.choice([33000, 40000, 70001]) if name.startswith(("limit", "size")) else RAW
        wnd = 3 * MB if name == "raw_run_default" else MB if name.startswith("limit") else rng.choice([32 * KB, 48 * KB + 5, 64 * KB])
        sim = Sim(wnd, raw=raw)
        if name == "src_ends_at_wnd":
            _prefix(sim, rng)
            n = rng.randrange(5, 2000)
            sim.match(sim.cur + n, n)                     # before the wrap: the source is the never-written tail of the window
            lits(sim, rng, 3)
            fill_to(sim, rng, wnd - 1); lits(sim, rng, 1)
            walk(sim, rng, 50)
            n = rng.randrange(5, 2000)
            sim.match(sim.cur + n, n)                     # after it: the last n bytes of the previous lap
            walk(sim, rng, 50)
        elif name == "dst_ends_at_wnd":
            _prefix(sim, rng)
            fill_to(sim, rng, wnd - rng.randrange(2, 3000))
            sim.match(rng.randrange(1, 3000), wnd - sim.cur)
            assert sim.cur == 0
            walk(sim, rng, 100)
            fill_to(sim, rng, wnd - rng.randrange(2, 300))
            sim.match(rng.randrange(1, 3000), 5); lits(sim, rng, 1)
            sim.repm(0, wnd - sim.cur)
            assert sim.cur == 0
            walk(sim, rng, 100)
        elif name == "wrap_inside_long_run":
            _prefix(sim, rng)
            for lap in range(3):                          # three laps in ONE run: copied / copied_from hand over each time
                fill_to(sim, rng, wnd - rng.randrange(2, 500))
                sim.match(rng.randrange(1, 64), wnd - sim.cur)
                walk(sim, rng, 200)
        elif name in ("limit_match", "limit_rep", "limit_lit", "limit_rep1"):
            _prefix(sim, rng, 0, 60)
            sim.end(rng.randrange(2)); sim.begin()
            walk(sim, rng, 30, kinds=(0, 0, 1))
            lits(sim, rng, 6)
            gap = 1 if name in ("limit_lit", "limit_rep1") else rng.randrange(2, 300)
            while raw - sim.i > gap:                      # run the counter up to `gap` bytes short of the limit
                n = min(raw - sim.i - gap, 9000)
                sim.match(5, n) if n >= 2 else sim.lit(7)
            if name == "limit_lit":
                sim.lit(rng.randrange(256))
            elif name == "limit_rep1":
                sim.rep1()
            elif name == "limit_rep":
                sim.repm(0, gap)
            else:
                sim.match(rng.randrange(1, 4), gap)
            assert sim.i == raw
            sim.cover.add(("edge", "packet_ends_at_limit", name))
            sim.end(rng.randrange(2))
            _prefix(sim, rng, 5, 50)
        elif name == "raw_run_default":
            sim.begin()
            lits(sim, rng, 500)
            while sim.raw - sim.i >= 2:
                sim.match(rng.choice([1, 2, 64, 65, 300]), min(sim.raw - sim.i, rng.randrange(100000, 900000)))
            if sim.raw - sim.i:
                sim.lit(0)
            assert sim.i == RAW
        elif name == "zero_byte_run":
            _prefix(sim, rng)
            sim.end(rng.randrange(2))
            sim.begin()                                   # a run that ends at once: size 0 ends the stream, rc 0
        elif name == "rle_at_1":
            _prefix(sim, rng, 1, 50)
            sim.end(rng.randrange(2))
            n = rng.randrange(600, 3000)
            sim.dlt_block(rng.randrange(5), n, [("lit", rng.randrange(256)), ("run", n + 5)], rng.randrange(2))   # clipped too
            n = rng.randrange(14, 400)
            sim.dlt_block(rng.randrange(5), n, [("lit", 9), ("run", n - 1)], rng.randrange(2))
        elif name == "size_eq_max":
            for typ in rng.sample([DT_BAD, DT_ENTROPY, DT_DLT], 3):
                if typ == DT_DLT:
                    sim.dlt_block(rng.randrange(5), raw, [("lit", 3), ("run", raw - 1)], rng.randrange(2))
                else:
                    sim.raw_block(typ, bytes(rng.randrange(256) for _ in range(raw)), rng.randrange(2))
        done(sim, idx, name)
    return out


REFUSED = ["match_src", "match_dst", "match_limit", "rep_src", "rep_dst", "rep_limit", "rle_run_at_0", "size_bad", "size_entropy",
           "size_dlt", "type_0", "type_4", "type_5", "type_6", "type_10", "type_0x15", "type_0x1e", "type_big"]


def fam_refused(seed, orc):
    """every check of the reference at its FIRST illegal value (the legal twins are in `edges`); each after a legal
    prefix of random length whose bytes the decoder has already delivered"""
    out = []
    for idx, name in enumerate(REFUSED):
        rng = random.Random(seed * 1000 + idx)
        raw = rng.choice([33000, 40000, RAW])
        wnd = MB if name.endswith("limit") else rng.choice([32 * KB, 40000, 64 * KB])
        if name.endswith("limit"):
            raw = rng.choice([33000, 40000])
        sim = Sim(wnd, raw=raw)
        if rng.random() < 0.8:                            # delivered runs before the refused one (sometimes none)
            for _ in range(rng.randrange(1, 3)):
                _prefix(sim, rng, 1, 300)
                sim.end(rng.randrange(2))
        kind, _, what = name.partition("_")
        if kind in ("match", "rep"):
            _prefix(sim, rng, 1, 60)                      # the refused run's own packets: decoded, never delivered
            lits(sim, rng, 6)
            if what == "limit":
                gap = rng.randrange(1, 3000)
                while raw - sim.i > gap:
                    n = min(raw - sim.i - gap, 9000)
                    sim.match(5, n) if n >= 2 else sim.lit(1)
                d, n = sim.rep[0], gap + 1
                if kind == "match" or d == 0:
                    d = rng.randrange(1, 4)
                    if kind == "rep":
                        raise AssertionError("generator: no rep distance planted")
            elif what == "dst":
                if sim.cur > wnd - 3100:
                    fill_to(sim, rng, wnd - 1); lits(sim, rng, 1)
                fill_to(sim, rng, wnd - rng.randrange(12, 3000))
                if raw - sim.i < 4000:
                    sim.end(0); sim.begin()
                d = rng.randrange(1, 3000)
                sim.match(d, 5); lits(sim, rng, 1)        # (a rep needs the distance planted)
                n = wnd - sim.cur + 1
            else:
                if sim.cur > wnd - 500:
                    fill_to(sim, rng, wnd - 1); lits(sim, rng, 1)
                if raw - sim.i < 500:
                    sim.end(0); sim.begin()
                n = rng.randrange(5, 400)
                d = sim.cur + n + 5
                sim.match(d, 5); lits(sim, rng, 1)        # now source = [wnd - n + 1, wnd + 1): one byte past the window
            bad = [sim.src(d) + n > wnd, n + sim.i > raw, sim.cur + n > wnd]
            assert n >= 2 and bad == [what == "src", what == "limit", what == "dst"], (name, bad)
            assert sim.why_not(d, n - 1) is None or n == 2   # the legal twin: one less
            assert kind == "match" or sim.rep[0] == d
            sim.refuse(name, [OP_MATCH, d, n, 0] if kind == "match" else [OP_REP, 0, n, 0], DECODE_ERROR)
        elif name == "rle_run_at_0":
            sim.refuse(name, [OP_DLT, DT_DLT + rng.randrange(5), rng.randrange(20, 3000), OP_RLE_RUN, rng.randrange(11, 500)], -1)
        elif kind == "size":
            typ = {"bad": DT_BAD, "entropy": DT_ENTROPY, "dlt": DT_DLT + rng.randrange(5)}[what]
            ops = [OP_DLT, typ, raw + 1] if what == "dlt" else [OP_BLOCK, typ, OP_BAD if what == "bad" else OP_ENTROPY, raw + 1] + [0] * ((raw + 4) // 4)
            sim.refuse(name, ops, -1)
        else:
            v = {"0": 0, "4": 4, "5": 5, "6": 6, "10": 10, "0x15": 0x15, "0x1e": 0x1E, "big": rng.randrange(0x20, 1 << 31)}[what]
            sim.refuse(name, [OP_RAW_TYPE, v], DECODE_ERROR)
        out.append(sim.case({"family": "refused", "seed": seed, "index": idx, "name": name}))
    return out


def _rle_items(rng, n):
    items, i = [], 0
    while i < n:
        if i > 0 and rng.random() < 0.15:
            v = rng.randrange(11, 400) if rng.random() < 0.9 else rng.randrange(400, 20000)
            items.append(("run", v)); i += min(v, n - i)
        else:
            items.append(("lit", rng.randrange(256) if rng.random() < 0.5 else rng.randrange(4))); i += 1
    return items


def fam_blocks(seed, orc):
    out = []
    for idx, mode in enumerate(["always", "never", "random", "always", "never", "rc_full"]):
        rng = random.Random(seed * 1000 + idx)
        sim = Sim(rng.choice([32 * KB, 50000, 128 * KB]))
        flag = flag_of("never" if mode == "rc_full" else mode, rng)
        if mode == "rc_full":                             # > 64 KiB of coded bytes and no restart: an RC block fills to csc_blocksize
            sim.begin(); lits(sim, rng, 45000); sim.end(0)
            sim.raw_block(DT_ENTROPY, bytes(rng.randrange(256) for _ in range(45000)), 0)
            sim.raw_block(DT_BAD, bytes(rng.randrange(256) for _ in range(70000)), 0)     # and a BC block
        for b in range(40 if idx < 3 else 12):
            t = rng.choice(["normal", "normal", "bad", "entropy", "dlt", "dlt", "exe", "txt"]) if idx >= 3 or b % 8 else ["exe", "txt"][b // 8 % 2]
            tiny = rng.random() < 0.3
            if t == "normal":
                sim.begin()
                walk(sim, rng, 1 if tiny else rng.randrange(1, 120))
                if sim.i == 0:
                    sim.lit(rng.randrange(256))
                sim.end(flag())
            elif t in ("bad", "entropy"):
                n = rng.randrange(1, 4) if tiny else rng.randrange(1, 9000)
                sim.raw_block(DT_BAD if t == "bad" else DT_ENTROPY, bytes(rng.randrange(256) for _ in range(n)), flag())
            elif t == "dlt":
                n = rng.randrange(1, 4) if tiny else rng.choice([rng.randrange(4, 512), 511, 512, 513, rng.randrange(513, 9000)])
                sim.dlt_block(rng.randrange(5), n, _rle_items(rng, n), flag())
            else:
                kind = "exe" if t == "exe" else "text"
                n = rng.randrange(1, 20000) if kind == "exe" else rng.randrange(16384, 30000)
                if sim.wnd_size - sim.cur < n:            # emit() wants the run in one piece of the window: go round first
                    sim.begin(); fill_to(sim, rng, sim.wnd_size - 1); lits(sim, rng, 1); sim.end(flag())
                if sim.wnd_size - sim.cur < n:
                    continue
                plain, coded = filtered(orc, kind, rng, n)
                sim.begin(DT_EXE if kind == "exe" else DT_ENGTXT, flt=np.frombuffer(plain, np.uint8), size_field=rng.choice([n, 0, 1 << 20]))
                emit(sim, rng, coded)
                sim.end(flag())
        sim.eof()
        out.append(sim.case({"family": "blocks", "seed": seed, "index": idx, "name": mode}))
    return out


GEOMETRY = [(32 * KB, 4096, 8192), (32 * KB + 1, 5000, 33000), (40000, 64 * KB, 5000), (100003, 10007, 100000), (64 * KB, 128 * KB, 3 * MB),
            (100003, 4097, 40000)]


def fam_geometry(seed, orc):
    out = []
    for idx, (wnd, bsize, raw) in enumerate(GEOMETRY):
        rng = random.Random(seed * 1000 + idx)
        sim = Sim(wnd, bsize=bsize, raw=raw)
        flag = flag_of(["never", "random"][idx % 2], rng)
        laps = 0
        while laps < 2:
            sim.begin()
            w0 = sim.wrapped
            sim.wrapped = False
            walk(sim, rng, 400)
            while sim.raw - sim.i >= 1 and rng.random() < 0.5 and sim.room() > 2000:
                sim.match(rng.randrange(1, 3000), min(sim.room(), rng.randrange(2, 30000))) if sim.cur > 3000 else sim.lit(1)
            if sim.i == 0:
                sim.lit(0)
            laps += sim.wrapped
            sim.wrapped = sim.wrapped or w0
            sim.end(flag())
            n = rng.randrange(1, min(raw, 3000) + 1)
            if rng.random() < 0.5:
                sim.raw_block(rng.choice([DT_BAD, DT_ENTROPY]), bytes(rng.randrange(256) for _ in range(n)), flag())
            else:
                sim.dlt_block(rng.randrange(5), n, _rle_items(rng, n), flag())
        sim.eof()
        sim.cover.add(("geometry", wnd, bsize, raw))
        out.append(sim.case({"family": "geometry", "seed": seed, "index": idx}))
    return out


LONG_CHAIN_RAW = 6 * MB
UNDO_CAP_BITS = 32768                                     # the device decoder's journal: probability updates a packet


def fam_long_chain(seed, orc):
    """one distance-1 match of about 5.5 MiB under raw_blocksize = 6 MiB: more than 32 768 long-length bits in one packet"""
    rng = random.Random(seed)
    sim = Sim(8 * MB, raw=LONG_CHAIN_RAW)
    sim.begin()
    lits(sim, rng, 100)
    sim.end(0)                                            # a delivered run first: the documented answer keeps these bytes
    sim.begin()
    lits(sim, rng, 10)
    n = 5 * MB + 512 * KB + rng.randrange(1000)
    assert (n - 2) // 143 > 32768
    sim.match(1, n)
    lits(sim, rng, 5)
    sim.end(1)
    sim.eof()
    sim.cover.add(("edge", "long_chain"))
    return [sim.case({"family": "long_chain", "seed": seed, "index": 0, "big": True})]


def fam_long_rle(seed, orc):
    """default geometry: a DT_DLT block of a few hundred bytes whose RLE run is CODED as about 5 000 000 (more than 32 768
    long-length bits) and clipped by the block size, as decode_rle clips any run"""
    rng = random.Random(seed)
    sim = Sim(64 * KB)
    sim.begin()
    lits(sim, rng, 100)
    sim.end(0)                                            # a delivered run first: the documented answer keeps these bytes
    n = rng.randrange(520, 700)
    sim.dlt_block(rng.randrange(5), n, [("lit", rng.randrange(256)), ("run", 5_000_000 + rng.randrange(1000))], 1)
    sim.eof()
    return [sim.case({"family": "long_rle", "seed": seed, "index": 0})]


# ---- the inverse filters, restated from the reference (csc_filters.cpp:337-368, :557-610) -------------------------------

def inverse_dict(src, words):
    """Filters::Inverse_Dict over a run of len(src) bytes: (output, highest source index read).  An index >= the size is
    a read of stale memory (taken as 0 here): such a run is no case."""
    size, dst, i, hi = len(src), bytearray(), 0, -1
    while len(dst) < size:
        hi = max(hi, i)
        b = src[i] if i < size else 0
        if 0x82 <= b < 0x82 + len(words):
            dst += words[b - 0x82][:size - len(dst)]
        elif b == 254 and i + 1 < size and src[i + 1] >= 0x82:
            i += 1
            hi = max(hi, i)
            dst.append(src[i])
        else:
            dst.append(b)
        i += 1
    return bytes(dst), hi


DICT_MISTAKES = ("parity_not_carried", "run_of_64_even", "guard_dropped", "not_clipped", "max_symbol_fd")


def inverse_dict_steps(src, words, mistake=None):
    """Inverse_Dict the way a 64-lane step computes it: a byte >= 0x82 is swallowed by a marker iff the run of 254s
    below it is odd, the parity carried from step to step; the last 66 source bytes serially.  Equal to inverse_dict()
    without a mistake; `mistake` plants one of DICT_MISTAKES.  Reads past the run give 0xFF, output is not cut to size."""
    assert mistake is None or mistake in DICT_MISTAKES
    size, dst, i, carry = len(src), bytearray(), 0, 0
    top = 0xFE if mistake == "max_symbol_fd" else 0x82 + len(words)

    def at(k):
        return src[k] if k < size else 0xFF

    def word(b):
        w = words[b - 0x82] if b - 0x82 < len(words) else b"zz"
        return w if mistake == "not_clipped" else w[:max(0, size - len(dst))]

    while len(dst) < size and i + 66 < size:
        for lane in range(64):
            b = src[i + lane]
            r = 0
            while r < lane and src[i + lane - 1 - r] == 254:
                r += 1
            par = (r + (carry if r == lane and mistake != "parity_not_carried" else 0)) & 1
            esc = par and b >= 0x82
            if b == 254 and not esc and at(i + lane + 1) >= 0x82:
                continue                                          # a marker: nothing comes out
            dst += word(b) if not esc and 0x82 <= b < top else bytes([b])[:max(0, size - len(dst))]
        lead = 0
        while lead < 64 and src[i + 63 - lead] == 254:
            lead += 1
        carry = ((0 if mistake == "run_of_64_even" else carry + 64) if lead == 64 else lead) & 1
        i += 64
    escaped = bool(carry & 1) and at(i) >= 0x82
    while len(dst) < size:
        b = at(i)
        if escaped:
            dst.append(b)
            escaped = False
        elif 0x82 <= b < top:
            dst += word(b)
        elif b == 254 and (i + 1 < size or mistake == "guard_dropped") and at(i + 1) >= 0x82:
            i += 1
            dst.append(at(i))
        else:
            dst.append(b)
        i += 1
    return bytes(dst)


def inverse_e89(buf):
    """Filters::Inverse_E89 unrolled like filter_cases.forward_e89: yswap, then minus the position behind the operand"""
    b = bytearray(buf)
    n, next_ok = len(b), 0
    for j in range(max(0, n - 5)):
        if j < next_ok or b[j] & 0xFE != 0xE8:
            continue
        next_ok = j + 4
        x = (int.from_bytes(b[j + 1:j + 5], "little") - 0xFF000000) & 0xFFFFFFFF
        if x < 0x02000000:
            x = (((x >> 24) << 7) | ((x >> 16 & 255) << 8) | ((x >> 8 & 255) << 16) | ((x << 24) & 0xFFFFFFFF)) >> 7
            x = (((x - (j + 5)) & 0x01FFFFFF) + 0xFF000000) & 0xFFFFFFFF
            b[j + 1:j + 5] = x.to_bytes(4, "little")
    return bytes(b)


PLAIN = b"etaoin q\n"                                       # one source byte, one output byte
RUN254 = tuple(range(1, 10)) + (63, 64, 65, 127, 128, 129)
RUN254_STARTS = tuple(range(56, 65))
TXT_SIZES = (1, 2, 3, 65, 66, 67, 68, 130, 131, 195, 16384 + 123)
TAIL_SIZES = (40, 67, 131, 200, 259)
TAIL_BOUNDARY = ("marker_hi", "marker_lo", "pair_hi", "three_hi", "three_lo")
ALLWORDS_SIZES = (299, 301, 302, 303, 1000)


def txt_source(n, placed, rng, words, exact=False, reach=True):
    """the n source bytes of a DT_ENGTXT run: `placed` {position: byte} over plain filler; then the earliest free positions
    become four-letter word symbols until Inverse_Dict reads nothing at or behind n (THE condition of this family's
    header entry).  exact: the last source byte is read (the last symbol shortened as needed); reach: every placed byte is."""
    by_len = {k: [0x82 + i for i, w in enumerate(words) if len(w) == k] for k in (2, 3, 4)}
    src = bytearray(rng.choice(PLAIN) for _ in range(n))
    for p, b in placed.items():
        src[p] = b
    free = [p for p in range(n) if p not in placed]
    k = 0
    out, hi = inverse_dict(src, words)
    while hi >= n:
        for _ in range((hi - n + 3) // 3):
            assert k < len(free), "no room left to pay for the markers"
            src[free[k]] = rng.choice(by_len[4])
            k += 1
        out, hi = inverse_dict(src, words)
    want = n - 1 if exact else max(placed) if reach and placed else -1
    if hi < want:                                           # paid too much: a shorter word in the last symbol's place
        assert k > 0, (n, hi)
        for wl in (3, 2):
            src[free[k - 1]] = rng.choice(by_len[wl])
            out, hi = inverse_dict(src, words)
            if want <= hi < n:
                break
    assert hi < n and len(out) == n, (n, hi)
    assert not exact or hi == n - 1, (n, hi)
    assert not (reach and placed) or hi >= max(placed), (n, hi, max(placed))
    return bytes(src), out


def txt_runs(words):
    """{case name: [(source bytes, predicted plain bytes, coverage cells)]} of the family's DT_ENGTXT runs"""
    rng = random.Random(10101)
    sym = {k: [0x82 + i for i, w in enumerate(words) if len(w) == k] for k in (2, 3, 4)}
    cases = {}

    def run(name, n, placed, cells, **kw):
        src, out = txt_source(n, placed, rng, words, **kw)
        for p, b in placed.items():
            assert src[p] == b
        cases.setdefault(name, []).append((src, out, set(cells)))

    for n in TXT_SIZES:
        if n == 1:
            placed = {0: 254}
        elif n == 2:
            placed = {0: sym[2][0], 1: 0x71}
        elif n == 3:
            placed = {0: 254, 1: 0x90, 2: sym[3][0]}
        else:
            placed = {p: rng.choice((254, 254, 0x82, 0xFB, 0xFC, 0xFD, 0xFF, 0x80, 0x81, 0x90)) for p in rng.sample(range(n), n // 5)}
        run("txt_sizes", n, placed, [("flt", "txt_size", n)], reach=n in (1, 3))
    for follow in ("hi", "lo"):                             # runs of 254 of every listed length from every listed lane
        for start in RUN254_STARTS:
            placed, cells, pos = {}, [], 3 * 64 + start
            for k, length in enumerate(RUN254):
                for p in range(pos, pos + length):
                    placed[p] = 254
                placed[pos - 1] = 0x71
                placed[pos + length] = (0x90, 0xFF, 0xFB, 0x82)[k % 4] if follow == "hi" else (0x65, 0x81, 0x00, 0x20)[k % 4]
                placed[pos + length + 1] = 0x71
                cells.append(("flt", "run254", length, start, follow))
                if any(q % 64 == 0 and all(placed.get(q + t) == 254 for t in range(64)) for q in range(pos - 63, pos + length)):
                    cells.append(("flt", "whole_step_of_254", follow))
                pos = (pos + length + 2 + 63) // 64 * 64 + start
            run(f"txt_254_{follow}", pos + 70, placed, cells)
    for n in TAIL_SIZES:
        where = "serial" if n <= 66 else "tail"
        run("txt_tail", n, {n - 1: 254, n - 2: 0x71}, [("flt", "last_254", where)], exact=True)
        run("txt_tail", n, {n - 2: 254, n - 1: 0x90, n - 3: 0x71}, [("flt", "last_but_one_254_hi", where)], exact=True)
        i0 = 0
        while i0 + 66 < n:
            i0 += 64
        if i0:                                              # the last vector step's lane 63 and the serial tail's first byte
            for name, pat in zip(TAIL_BOUNDARY, ({-1: 254, 0: 0x90}, {-1: 254, 0: 0x65}, {-2: 254, -1: 254, 0: 0x90},
                                                 {-1: 254, 0: 254, 1: 254, 2: 0x90}, {-1: 254, 0: 254, 1: 254, 2: 0x65})):
                placed = {i0 + d: b for d, b in pat.items()}
                placed[i0 + min(pat) - 1] = 0x71
                run("txt_tail", n, placed, [("flt", "tail_boundary", name)])
    for n in (70, 150):
        pat = {5: 0x82, 9: 0xFB, 13: 0xFC, 17: 0xFD, 21: 0xFF, 24: 0x71, 25: 254, 26: 254, 27: 0x71, 30: 254, 31: 0x82, 35: 254, 36: 0xFB,
               40: 254, 41: 0x81, 45: 0x80, 46: 0x81}
        placed = dict(pat)
        placed.update({n - 50 + p: b for p, b in pat.items() if n > 100})
        run("txt_symbols", n, placed, [("flt", "byte", b) for b in (0x82, 0xFB, 0xFC, 0xFD, 0xFF)] + [("flt", "pair_254_254")])
    for n in (50, 200):                                     # a word symbol as the last source byte reached: clipped at size
        for wl in (2, 3, 4):
            for room in (1, 2, 3):
                placed = {p: 0x71 for p in range(n)}
                placed[n - room] = sym[wl][(n + room) % len(sym[wl])]
                src, out = txt_source(n, placed, rng, words, reach=False)
                assert inverse_dict(src, words)[1] == n - room + max(0, room - wl)
                assert out[n - room:n - room + wl] == words[placed[n - room] - 0x82][:room]
                cases.setdefault("txt_clip", []).append((src, out, {("flt", "clip", wl, room)}))
    for n in ALLWORDS_SIZES:                                # the output is full after a quarter of the source
        placed = {p: rng.choice(sym[4]) for p in range(n)}
        run("txt_allwords", n, placed, [("flt", "all_four_letter", n % 4)], reach=False)
    return cases


def exe_runs():
    """{case name: [(filtered bytes, predicted plain bytes, cells)]}: filter_cases.e89_cases() taken as the FILTERED side"""
    cases = {}
    for name, buf in filter_cases.e89_cases().items():
        group = name.split("/")[1]
        group = {"top": "operand", "all": "dense", "phase": "dense"}.get(group, group)
        cases.setdefault("exe_" + group, []).append((buf, inverse_e89(buf), {("flt", "exe", name)}))
    return cases


def fam_filters(seed, orc):
    words = filter_cases.words(orc)
    out = []
    groups = [(DT_ENGTXT, txt_runs(words)), (DT_EXE, exe_runs())]
    idx = 0
    for typ, byname in groups:
        for name, runs in byname.items():
            rng = random.Random(seed * 1000 + idx)
            sim = Sim(256 * KB)
            _prefix(sim, rng, 1, 40)
            sim.end(rng.randrange(2))
            for k, (coded, plain, cells) in enumerate(runs):
                n = len(coded)
                assert len(plain) == n and sim.wnd_size - sim.cur >= n
                field = [n, 0, 1 << 20][(k + idx) % 3]
                sim.begin(typ, flt=np.frombuffer(plain, np.uint8), size_field=field)
                emit(sim, rng, coded)
                sim.end(rng.randrange(2))
                sim.cover |= cells
                if typ == DT_ENGTXT:
                    sim.cover.add(("flt", "size_field", ["n", "0", "1MiB"][(k + idx) % 3]))
            sim.eof()
            out.append(sim.case({"family": "filters", "seed": seed, "index": idx, "name": name}))
            idx += 1
    return out


_FAMS = {"walk": fam_walk, "lengths": fam_lengths, "distances": fam_distances, "edges": fam_edges, "blocks": fam_blocks,
         "geometry": fam_geometry, "refused": fam_refused, "long_chain": fam_long_chain, "long_rle": fam_long_rle, "filters": fam_filters}


def cases(orc, family, seed):
    """the cases of one family and seed; `orc` is the oracle library (ctypes CDLL) for the forward filters"""
    return _FAMS[family](seed, orc)


def all_cases(orc, families=None):
    return [c for f in (families or FAMILIES) for s in FAMILIES[f] for c in cases(orc, f, s)]


def coverage(cs):
    cov = set()
    for c in cs:
        cov |= c["cover"]
    return cov


def describe(case):
    return "synth case " + json.dumps(case["meta"], separators=(",", ":"), sort_keys=True)


def case_id(case):
    m = case["meta"]
    return f"{m['family']}/{m['seed']}/{m['index']}"


def header(case):
    m = case["meta"]
    return bytes([m["dict"] >> 24 & 255, m["dict"] >> 16 & 255, m["dict"] >> 8 & 255, m["dict"] & 255,
                  m["bsize"] >> 16 & 255, m["bsize"] >> 8 & 255, m["bsize"] & 255, m["raw"] >> 16 & 255, m["raw"] >> 8 & 255, m["raw"] & 255])


def stream(orc, case):
    """the 10 property bytes + orc_synth(script)"""
    m = case["meta"]
    p = CSCProps()
    p.dict_size, p.csc_blocksize, p.raw_blocksize = m["dict"], m["bsize"], m["raw"]
    w = BytesWriter()
    s = np.ascontiguousarray(case["script"], np.uint32)
    orc.orc_synth.argtypes = [C.POINTER(CSCProps), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    orc.orc_synth.restype = C.c_int
    rc = orc.orc_synth(C.byref(p), s.ctypes.data, s.size, C.cast(w.ptr(), C.c_void_p), None)
    assert rc == 0, f"orc_synth: {rc}; {describe(case)}"
    return header(case) + bytes(w.out)


def blocks_of(stream_bytes):
    """[(is_rc, size, full flag)] of a stream's blocks (MemIO's framing)"""
    p, out = 10, []
    bsize = int.from_bytes(stream_bytes[4:7], "big")
    while p < len(stream_bytes):
        fb = stream_bytes[p]; p += 1
        if fb & 64:
            n = bsize
        else:
            n = int.from_bytes(stream_bytes[p:p + 3], "big"); p += 3
        out.append((fb >> 7, n, bool(fb & 64)))
        p += n
    return out


SHORT_READS = (257, 1000, 65537)


def short_reads(case):
    """the ragged Read sizes a case is decoded with (the big ones: only the size above every default block)"""
    return (65537,) if case["meta"].get("big") else SHORT_READS


def digest(rc, out):
    return [rc, len(out), hashlib.sha256(out).hexdigest()]


def golden_line(case, stream_bytes, rc, out):
    return {"id": case_id(case), "stream_sha256": hashlib.sha256(stream_bytes).hexdigest(), "rc": rc, "len": len(out),
            "out_sha256": hashlib.sha256(out).hexdigest()}
