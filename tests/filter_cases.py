"""Seeded adversarial inputs for the block filters and the analyzer, shared by tools/make_golden_filter_edges.py (which
records what the REFERENCE makes of them in tests/golden/filter_edges.json), tests/test_filter_edges.py (oracle, CPU) and
tests/test_gpu_stages.py (the HIP kernels).  A plain module like cases.py, not a conftest.

Every buffer is built from small parts: patterns, words of the dictionary (read back from the oracle's own inverse filter:
`words(orc)`), and corpus.fill stretches as background.  Every case has a stable name.  The groups:
  e89_cases()          name -> bytes                       Forward_E89 (and, as the filtered side, the synthesizer's DT_EXE runs)
  delta_cases()        name -> (bytes, channels)           Forward_Delta
  dict_cases(words)    name -> (bytes, intended dstSize or None)   Foward_Dict, 16 383 .. 16 500 bytes
  analyze_cases()      name -> bytes                       Analyzer::Analyze, one verdict per 8 KiB block

The plain-Python restatements of Forward_E89 and of the dictionary filter's token chain at the end are what the generator
counts dstSize with, and -- each with ONE planted mistake -- what tests/test_filter_edges.py shows the cases sensitive to."""
import ctypes as C
import hashlib
import random

import numpy as np

from csc_amd import corpus

STEP = 64                                                   # positions a wave step of the HIP filters covers
DICT_MIN = 16384                                            # Foward_Dict refuses shorter runs
FILLER = b"q"                                               # no dictionary word starts with j, k, q, x or z
ANALYZE_KINDS = (("text", 1), ("exe", 2), ("delta", 3), ("random", 4), ("entropy8", 5), ("silesia", 6))   # stages.json's


def words(orc):
    """the 122 dictionary words in symbol order (symbol 0x82 + k), asked of orc_inverse_dict one symbol at a time"""
    out = []
    for k in range(122):
        buf = (C.c_uint8 * 5)(0x82 + k, 0x20, 0x20, 0x20, 0x20)
        orc.orc_inverse_dict(buf, 5)
        w = bytes(buf).split(b" ")[0]
        assert 2 <= len(w) <= 4 and w.isalpha() and w.islower(), (k, w)
        out.append(w)
    return out


def _text(n, off=0):
    return corpus.fill("text", 1, off, n).tobytes()


def _put(buf, pos, b):
    assert 0 <= pos and pos + len(b) <= len(buf), (pos, len(b), len(buf))
    buf[pos:pos + len(b)] = b


# ---- Forward_E89 ---------------------------------------------------------------------------------------------------------

E89_SIZES = (1, 5, 6, 7, 68, 69, 70, 71, 133)
E89_OFFSETS = tuple(range(59, 65)) + tuple(range(123, 129))
E89_TOPS = (0x00, 0xFF, 0x01, 0xFE, 0xE8, 0xE9)


def _biased(rng, n):
    """bytes with E8 / E9 / 00 / FF each drawn at probability 1/8"""
    return bytes(rng.choice((0xE8, 0xE9, 0x00, 0xFF)) if rng.random() < 0.5 else rng.randrange(256) for _ in range(n))


def e89_cases():
    out = {}
    for n in E89_SIZES:
        out[f"e89/size/{n}/mix"] = _biased(random.Random(8900 + n), n)
        out[f"e89/size/{n}/e8"] = (bytes.fromhex("e812000000") * (n // 5 + 1))[:n]
        out[f"e89/size/{n}/e9tail"] = (b"\x20" * n + bytes.fromhex("e934120000ff"))[-n:]     # an opcode as close to the end as n allows
    for off in E89_OFFSETS:                                 # operand inside the group, across it, in the next one
        for op in (0xE8, 0xE9):
            b = bytearray(_text(200))
            _put(b, off, bytes([op, 0x34, 0x12, 0x00, 0x00]))
            out[f"e89/at/{off}/{op:02x}"] = bytes(b)
    for size in (70, 71, 100):                              # size-6 is the last eligible position
        for back in (7, 6, 5):
            for op in (0xE8, 0xE9):
                b = bytearray(_text(size))
                _put(b, size - back, bytes([op, 0x78, 0x56, 0x34, 0xFF])[:back])
                out[f"e89/end/{size}/{back}/{op:02x}"] = bytes(b)
    for top in E89_TOPS:                                    # E8 / E9 on top: not rewritten, and itself the next candidate
        for off in (10, 60):
            b = bytearray(_text(160))
            _put(b, off, bytes([0xE8, 0x11, 0x22, 0x33, top, 0x44, 0x55, 0x66, 0x00, 0x77]))
            out[f"e89/top/{top:02x}/{off}"] = bytes(b)
    out["e89/all/e8"] = b"\xe8" * 300
    out["e89/all/e9"] = b"\xe9" * 300
    for ph in range(4):                                     # E8 x 5 then zeros, at each phase of the skip chain
        b = bytearray(_text(200))
        _put(b, ph, b"\xe8" * 5 + b"\0" * 4)
        out[f"e89/phase/start/{ph}"] = bytes(b)
        b = bytearray(_text(200))
        _put(b, 56, bytes.fromhex("e800000000"))            # taken: the chain resumes at 60
        _put(b, 58 + ph, b"\xe8" * 5 + b"\0" * 4)
        out[f"e89/phase/chained/{ph}"] = bytes(b)
    for j in (20, 62):                                      # (x + j + 5) & 0x01FFFFFF wraps
        ops = {"00ffffff": 0x00FFFFFF, "ff000000": 0xFF000000, "ffffffff": 0xFFFFFFFF}
        for d in (-1, 0, 1):
            x = (0x01FFFFFF - (j + 5) + d) & 0xFFFFFFFF
            ops[f"raw{d:+d}"] = x                            # top byte 01: left alone
            ops[f"wrap{d:+d}"] = (x + 0xFF000000) & 0xFFFFFFFF   # the value the filter adds j + 5 to
        for name, x in ops.items():
            b = bytearray(_text(140))
            _put(b, j, b"\xe8" + x.to_bytes(4, "little"))
            out[f"e89/operand/{j}/{name}"] = bytes(b)
    out["e89/dense/2000"] = _biased(random.Random(8989), 2000)
    return out


# ---- Forward_Delta -------------------------------------------------------------------------------------------------------

DELTA_CHN = (1, 2, 3, 4, 8)


def delta_cases():
    out = {}
    for chn in DELTA_CHN:
        sizes = sorted({511, 512, 513, 8191, 8192, 8193} | {512 + r for r in range(chn)})
        for n in sizes:
            rng = random.Random(7700 + 16 * n + chn)
            out[f"delta/{chn}/{n}/ramp"] = (bytes((3 * i + 7) & 255 for i in range(n)), chn)
            out[f"delta/{chn}/{n}/const"] = (bytes([0xA5]) * n, chn)
            out[f"delta/{chn}/{n}/random"] = (bytes(rng.randrange(256) for _ in range(n)), chn)
    return out


# ---- Foward_Dict ---------------------------------------------------------------------------------------------------------

def _dict_buf(size, head, fill=b"that"):
    """`head` (the adversarial part) + four-letter words up to size - 8 + filler: the words pay for the 82 % test"""
    assert len(head) <= size - 8
    n = (size - 8 - len(head)) // len(fill)
    b = head + fill * n
    return bytes(b + FILLER * (size - len(b)))


def _counted(size, dst, escapes):
    """a buffer of `size` whose dstSize is `dst`: n4 four-letter words (4 -> 1), f filler bytes (1 -> 1) and e escaped
    bytes (1 -> 2), e the smallest count >= escapes that makes the equations whole; the last five bytes are filler"""
    for e in range(escapes, escapes + 3):
        if (size - dst + e) % 3 == 0:
            break
    n4 = (size - dst + e) // 3
    f = dst - 2 * e - n4
    assert n4 >= 0 and f >= 5 and 4 * n4 + f + e == size and n4 + f + 2 * e == dst, (size, dst, e, n4, f)
    return b"that" * n4 + FILLER * (f - 5) + b"\x90" * e + FILLER * 5


def reject_sizes():
    """sizes for the 82 % boundary: the first and the last the cases use, and those where 0.82 * size is a whole number in
    double arithmetic (there `>` and `>=` part ways)"""
    whole = [n for n in range(DICT_MIN, 16501) if float(n) * 0.82 == int(float(n) * 0.82)]
    assert len(whole) >= 2, whole
    return [DICT_MIN, 16399] + whole


def dict_cases(words):
    out = {}

    def add(name, buf, dst=None):
        assert name not in out and DICT_MIN - 1 <= len(buf) <= 16500, (name, len(buf))
        out["dict/" + name] = (bytes(buf), dst)

    by_len = {2: b"at", 3: b"the", 4: b"that"}
    assert all(w in words for w in by_len.values()) and b"with" in words
    for step in (0, 2):                                     # a word across the end of a step, the chain arriving in every state
        for arrive in (range(4) if step else (0,)):
            for wl, w in by_len.items():
                for s in range(60, 65):
                    head = bytearray(FILLER * (STEP * (step + 2)))
                    if arrive:
                        _put(head, STEP * step - 4 + arrive, b"with")
                    _put(head, STEP * step + s, w)
                    add(f"straddle/{step}/{arrive}/{wl}/{s}", _dict_buf(16400, bytes(head)))
    for off in range(4):
        add(f"backtoback/{off}", _dict_buf(16400 + off, FILLER * off))
    for s in (b"thethe", b"there", b"andand", b"tionion", b"oftion", b"sheshe"):   # greedy is not "longest word everywhere"
        add(f"greedy/{s.decode()}/packed", _dict_buf(16411, s * 43))
        add(f"greedy/{s.decode()}/spaced", _dict_buf(16411, (s + b" ") * 37))
    edge = b"".join(bytes([c]) + b"that" + bytes([c]) + b"at" for c in b"`{@[AZ") + bytes(range(0x41, 0x5B)) + b"That tHat thaT THAT"
    add("range_ends", _dict_buf(16420, edge * 3))
    hi = (0x80, 0x81, 0x82, 0xFB, 0xFC, 0xFD, 0xFE, 0xFF)
    add("high/single", _dict_buf(16430, b"".join(b"that" + bytes([c]) + b"the" + bytes([c]) + b"q" for c in hi) * 4))
    for c in hi:
        add(f"high/runs/{c:02x}", _dict_buf(16430, b"".join(b"that" + bytes([c]) * k for k in (2, 3, 5, 63, 64, 65))))
    add("high/all_ff", b"\xff" * 16500)                     # the largest expansion there is: rejected
    for wl, w in by_len.items():                            # the walked range ends at size - 5
        for back in range(9, 4, -1):
            b = bytearray(_dict_buf(16397, b""))
            _put(b, 16397 - 12, FILLER * 12)
            _put(b, 16397 - back, w)
            add(f"end/{wl}/{back}", b)
    for k in (5, 9):
        b = bytearray(_dict_buf(16397, b""))
        _put(b, 16397 - k, bytes([0x82, 0xFB, 0xFE, 0xFF, 0x90, 0xFC, 0x82, 0xFD, 0xFE][:k]))
        add(f"tail_high/{k}", b)
    for size in reject_sizes():                             # dstSize == floor(0.82 * size): accepted; one more: rejected
        lim = int(float(size) * 0.82)
        add(f"reject/{size}/at", _counted(size, lim, 3), lim)
        add(f"reject/{size}/above", _counted(size, lim + 1, 3), lim + 1)
    for size in (16384, 16385, 16399):                      # the vector copy-back's four loops: size and dst_size mod 16
        for r in (0, 1, 15):
            dst = 8000 + r
            add(f"copyback/{size % 16}/{r}", _counted(size, dst, 2), dst)
    add("size/16383", _text(16383))
    add("size/16384", _text(16384))
    for name, (buf, dst) in out.items():                    # what the generator intended, counted in plain Python
        if dst is not None:
            got = forward_dict(buf, words)[2]
            assert got == dst, (name, got, dst)
    return out


# ---- Analyzer ------------------------------------------------------------------------------------------------------------

ANALYZE_TAILS = (1, 2, 511, 512, 513, 8191)


def analyze_cases():
    out = {}
    for kind, seed in ANALYZE_KINDS:
        for t in ANALYZE_TAILS:                             # a short last block after a full one
            out[f"analyze/{kind}/tail/{t}"] = corpus.fill(kind, seed, 0, 8192 + t).tobytes()
    out["analyze/const"] = b"".join(bytes([v]) * 8192 for v in (0x00, 0x20, 0x61, 0x7F, 0x80, 0xE8, 0xFF))
    out["analyze/alternating"] = b"".join(bytes(p) * 4096 for p in ((0, 255), (0x20, 0x61), (0xE8, 0x00), (1, 2), (0x7F, 0x80)))
    out["analyze/ramp"] = b"".join(bytes((i // p + 37 * (i % p)) & 255 for i in range(8192)) for p in (1, 2, 3, 4, 8))
    return out


# ---- plain-Python restatements, with room for one planted mistake each ---------------------------------------------------

def _xswap(x):
    x = (x << 7) & 0xFFFFFFFF
    return (x >> 24) | ((x >> 16 & 255) << 8) | ((x >> 8 & 255) << 16) | ((x & 255) << 17)


def forward_e89(buf, skip=4, bound=5):
    """Filters::Forward_E89 unrolled: an opcode at j with j + 5 < size is looked at unless a taken one sits closer than four
    bytes below it; a 00 / FF operand becomes xswap((x + j + 5) & 0x01FFFFFF).  `skip` and `bound` are where mistakes go."""
    b = bytearray(buf)
    n, next_ok = len(b), 0
    for j in range(max(0, n - bound)):
        if j < next_ok or b[j] & 0xFE != 0xE8:
            continue
        next_ok = j + skip
        x = (int.from_bytes(b[j + 1:j + 5], "little") - 0xFF000000) & 0xFFFFFFFF
        if x < 0x02000000:
            x = (_xswap((x + j + 5) & 0x01FFFFFF) + 0xFF000000) & 0xFFFFFFFF
            b[j + 1:j + 5] = x.to_bytes(4, "little")[:max(0, n - j - 1)]
    return bytes(b)


def forward_dict(buf, words, carry=True, reject=lambda dst, size: dst > size * 0.82):
    """Filters::Foward_Dict: (accepted, bytes, dstSize).  The greedy chain of tokens over [0, size - 5), the escape-only
    tail, the 82 % test.  carry=False forgets the chain at every 64-position step (a token starts at each step's first
    position); `reject` is the comparison."""
    size = len(buf)
    if size < DICT_MIN:
        return 0, bytes(buf), 0
    trie = {}
    for k, w in enumerate(words):
        trie[w] = 0x82 + k
    prefixes = {w[:k] for w in words for k in range(1, len(w) + 1)}
    dst = bytearray()
    i = 0
    while i < size - 5:
        c = buf[i]
        adv = 1
        if 0x61 <= c <= 0x7A:
            sym, j = 0, 0
            while bytes(buf[i:i + j + 1]) in prefixes and i + j < size:
                j += 1
                if bytes(buf[i:i + j]) in trie:
                    sym, adv = trie[bytes(buf[i:i + j])], j
            dst.append(sym if sym else c)
        elif c >= 0x82:
            dst += bytes([254, c])
        else:
            dst.append(c)
        nxt = i + adv
        if not carry and nxt // STEP != i // STEP:
            nxt = nxt // STEP * STEP
        i = nxt
    for c in buf[i:]:
        dst += bytes([254, c]) if c >= 0x82 else bytes([c])
    n = len(dst)
    if reject(n, size):
        return 0, bytes(buf), n
    return 1, bytes(dst + b"\x20" * (size - n)), n


def first_difference(got, want):
    """None, or 'offset N: got .. / want ..' with sixteen bytes around the first differing offset from both sides"""
    if got == want:
        return None
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, np.uint8, n), np.frombuffer(want, np.uint8, n)
    d = np.flatnonzero(a != b)
    at = int(d[0]) if len(d) else n
    lo = max(0, at - 8)
    return f"first difference at offset {at} (lengths {len(got)} / {len(want)}): got {got[lo:lo + 16].hex()} want {want[lo:lo + 16].hex()}"


# ---- running the cases through a library's probes ------------------------------------------------------------------------

class Probes:
    """the filters and the analyzer of one library: prefix 'orc' (oracle/liborc.so) or 'ref' (oracle/_ref, ref_probe.cpp)"""

    def __init__(self, lib, prefix):
        f = lambda name: getattr(lib, f"{prefix}_{name}")   # noqa: E731
        for name in ("forward_e89", "inverse_e89", "inverse_dict"):
            f(name).argtypes, f(name).restype = [C.c_void_p, C.c_uint32], None
        f("forward_dict").argtypes, f("forward_dict").restype = [C.c_void_p, C.c_uint32], C.c_uint32
        for name in ("forward_delta", "inverse_delta"):
            f(name).argtypes, f(name).restype = [C.c_void_p, C.c_uint32, C.c_uint32], None
        f("analyze_block").argtypes, f("analyze_block").restype = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)], C.c_uint32
        f("dlt_bpb").argtypes, f("dlt_bpb").restype = [C.c_void_p, C.c_uint32, C.c_uint32], C.c_uint32
        self.f = f

    def run(self, name, data, *more):
        """(return value, transformed bytes) of one in-place filter over a private copy of `data`"""
        a = np.frombuffer(bytes(data), np.uint8).copy()
        r = self.f(name)(a.ctypes.data, len(a), *more)
        return r, a.tobytes()

    def analyze(self, data):
        """one row per 8 KiB block, as tools/make_golden.py writes them: type, bpb, and GetDltBpb x 5 for DT_DLT / DT_SKIP"""
        rows = []
        for i in range(0, len(data), 8192):
            blk = np.frombuffer(bytes(data[i:i + 8192]), np.uint8).copy()
            bpb = C.c_uint32(0xFFFFFFFF)
            t = self.f("analyze_block")(blk.ctypes.data, len(blk), C.byref(bpb))
            row = [int(t), int(bpb.value)]
            if 0x10 <= t < 0x15 or t == 0x1E:
                row += [int(self.f("dlt_bpb")(blk.ctypes.data, len(blk), c)) for c in DELTA_CHN]
            rows.append(row)
        return rows


def all_cases(orc):
    """{group: {name: case}} of all four groups; `orc` is the oracle library (ctypes CDLL), for the dictionary's words"""
    return {"e89": e89_cases(), "delta": delta_cases(), "dict": dict_cases(words(orc)), "analyze": analyze_cases()}


def digest(b):
    return hashlib.sha256(b).hexdigest()


def outputs_of(probes, groups):
    """name -> what the library makes of the case: ("e89" | "delta", bytes), ("dict", ok, bytes), ("analyze", rows)"""
    out = {}
    for name, data in groups["e89"].items():
        out[name] = ("e89", probes.run("forward_e89", data)[1])
    for name, (data, chn) in groups["delta"].items():
        out[name] = ("delta", probes.run("forward_delta", data, chn)[1])
    for name, (data, _) in groups["dict"].items():
        out[name] = ("dict",) + probes.run("forward_dict", data)
    for name, data in groups["analyze"].items():
        out[name] = ("analyze", probes.analyze(data))
    return out


def golden_entry(groups, name, res):
    """the JSON-able line of one case: digests and small integers only"""
    if res[0] == "analyze":
        return {"rows": res[1]}
    if res[0] == "dict":
        ent = {"dict_ok": int(res[1]), "sha256": digest(res[2])}
        if groups["dict"][name][1] is not None:
            ent["dst_size"] = groups["dict"][name][1]
        return ent
    return {"sha256": digest(res[1])}


def golden_of(probes, groups):
    return {name: golden_entry(groups, name, res) for name, res in outputs_of(probes, groups).items()}
