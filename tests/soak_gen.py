"""Seeded case generators for the randomized soaks, shared by tests/test_gpu_soak.py, tests/test_oracle_soak.py,
tests/test_gpu_forms.py and the wall-clock tools (tools/gpu_soak.py, tools/gpu_soak_batch.py), so that the tests and
the tools cannot drift apart.  Not a conftest: a plain module the tests import like `cases`.

A spec is a JSON-able dict, one line when printed:
  parts        input, in cases.build form ([kind, seed, offset, n], ["zeros", n], ...)
  level, dict  CSCEncProps_Init(dict, level), then
  props        field overrides (custom props; `row` names the dispatch row they select, see ROWS)
  nofilters    DLTFilter = TXTFilter = EXEFilter = 0
  max_read     the encoder's Read callback returns at most this many bytes (None: whole requests)
  dec_max_read the same for the decoder's Read
  pos          match-finder position right after Create (renormalisation cases; needs the stage build)

The generator is weighted toward what has found bugs: literal-rich data with two- and three-byte matches (delta,
entropy8, random splices into text), dictionaries smaller than the input, sizes within 64 of a power of two and
0 / 1 / 2 bytes, every parser row of the encoder's dispatch, filters off, ragged Read sizes."""
import ctypes as C
import json
import os

import cases
from csc_amd import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2 << 20                       # the batch drivers' chunk (= raw_blocksize)
RAW_BLOCKSIZE = 2 << 20               # CSCEncProps_Init, csc_enc.cpp
RENORM_LINE = 0xFFFFFFF0              # MatchFinder::normalize, csc_mf.cpp:108-114
KINDS = ["text", "exe", "delta", "random", "entropy8", "silesia", "mix5"]
KIND_WEIGHTS = [3, 2, 3, 1, 3, 1, 1]          # literal-rich kinds (delta, entropy8) as often as text
SEED = int(corpus.SEED_ENWIK9)

# Parser bits (csc_host.cpp, CSCEnc_Create) -> the dispatch row of the encoder's launchers (csc_kernels_blocks.inc).
ROWS = {
    3 | 4 | 8: "level3",        # level 3: bucket <= 2, good_len 2..16, advanced parser
    3 | 4: "level4",            # level 4; level 3 with good_len > 16 or a bucket of 3..9
    3 | 16: "level5",           # level 5: binary tree, no bucket, bt_cyc <= 32
    2 | 4 | 32: "level12",      # levels 1, 2: lazy / greedy parser over a bucket of up to eight
    2 | 4: "lazy_w9",           # lazy / greedy parser, a bucket of nine
    3: "adv_generic",           # BT + bucket, BT with bt_cyc > 32, advanced parser over a bucket wider than nine
    2: "lazy_generic",          # lazy / greedy parser with BT, or a bucket wider than nine
}
ROW_NAMES = list(ROWS.values())


def parser_bits(p):
    """csc_host.cpp, CSCEnc_Create: the launch kind of a CSCProps"""
    bt = bool(p.bt_hash_bits and p.bt_size)
    ht = bool(p.hash_bits and p.hash_width)
    k = 3 if p.lz_mode == 3 else 2
    if not bt and ht and p.hash_width <= 9:
        k |= 4
    if (k & 4) and p.lz_mode == 3 and p.hash_width <= 2 and 2 <= p.good_len <= 16:
        k |= 8
    if bt and not ht and p.lz_mode == 3 and p.bt_cyc <= 32:
        k |= 16
    if (k & 4) and p.lz_mode != 3 and p.hash_width <= 8:
        k |= 32
    return k


def row_of(p):
    return ROWS[parser_bits(p)]


def props_of(lib, spec):
    """the CSCProps of a spec for library `lib` (product, stage build, oracle or reference: same ABI)"""
    p = lib.props_init(spec["dict"], spec["level"])
    for k, v in spec.get("props", {}).items():
        setattr(p, k, v)
    if spec.get("nofilters"):
        p.DLTFilter = p.TXTFilter = p.EXEFilter = 0
    return p


def build_input(spec):
    return cases.build(spec["parts"])


def describe(seed, idx, spec):
    """one line that reproduces a case: seed, case index, spec"""
    return f"seed {seed} case {idx} spec {json.dumps(spec, separators=(',', ':'), sort_keys=True)}"


def seeds(default):
    """the fixed seeds plus CSCMI_SOAK_SEEDS=a,b,... from the environment (added, never replacing)"""
    extra = [int(s, 0) for s in os.environ.get("CSCMI_SOAK_SEEDS", "").replace(" ", "").split(",") if s]
    return list(default) + [s for s in extra if s not in default]


# ---- the pieces of a case -----------------------------------------------------------------------------------------

def _size(rng, cap):
    r = rng.random()
    if r < 0.08:
        return min(cap, rng.choice([0, 1, 2]))
    if r < 0.40:
        p = 1 << rng.randrange(0, max(1, min(22, cap.bit_length())))
        return max(1, min(cap, p + rng.randrange(-64, 65)))
    if r < 0.75:
        return rng.randrange(1, min(cap, 200_000) + 1)
    return rng.randrange(1, cap + 1)


def _kind(rng):
    return rng.choices(KINDS, KIND_WEIGHTS)[0]


def _parts(rng, n):
    """one corpus stretch, or a splice: a random kind cut into text (sometimes with text resuming after it)"""
    off = rng.randrange(0, 900_000_000)
    if n <= 4096 or rng.random() >= 0.3:
        return [[_kind(rng), SEED, off, n]] if n else []
    k2 = _kind(rng)
    a = rng.randrange(1, n)
    b = rng.randrange(a, n + 1) if rng.random() < 0.5 else n
    parts = [["text", SEED, off, a], [k2, SEED, off + 12345, b - a]]
    if b < n:
        parts.append(["text", SEED, off + a, n - b])
    return [p for p in parts if p[3]]


def _row_props(rng, row, small):
    """(level, overrides) of custom props that select `row`; `small` keeps a handle's tables small (batches of many)"""
    hb = rng.choice([12, 14, 16] if small else [12, 15, 16, 18, 20])
    if row == "level3":
        return 3, {"hash_width": rng.choice([1, 2]), "hash_bits": hb, "good_len": rng.choice([8, 12, 16])}
    if row == "level4":
        return rng.choice([(4, {"hash_width": rng.choice([3, 4, 5, 8, 9]), "hash_bits": hb, "good_len": rng.choice([16, 24, 48])}),
                           (3, {"good_len": rng.choice([24, 32, 48, 64, 65, 100, 200])}),
                           (3, {"hash_width": rng.choice([3, 4, 5, 8, 9]), "hash_bits": hb})])
    if row == "level5":
        return 5, {"bt_size": rng.choice([40000, 100000] if small else [40000, 100000, 300000, 1 << 20]),
                   "bt_cyc": rng.choice([4, 16, 32]), "good_len": rng.choice([8, 16, 48, 200])}
    if row == "level12":
        return rng.choice([1, 2]), {"hash_width": rng.choice([1, 2, 3, 4, 5, 8]), "hash_bits": hb,
                                    "good_len": rng.choice([8, 16, 24, 32, 64, 200]), "lz_mode": rng.choice([1, 2])}
    if row == "lazy_w9":
        return rng.choice([1, 2]), {"hash_width": 9, "hash_bits": hb, "good_len": rng.choice([8, 24, 64, 200]), "lz_mode": rng.choice([1, 2])}
    if row == "adv_generic":
        return rng.choice([(5, {"hash_width": rng.choice([2, 4, 8]), "hash_bits": hb}),                  # BT + bucket
                           (5, {"bt_cyc": rng.choice([33, 48, 64]), "bt_size": rng.choice([40000, 100000])}),
                           (3, {"hash_width": rng.choice([10, 12, 16]), "hash_bits": hb})])
    if row == "lazy_generic":
        return rng.choice([(5, {"lz_mode": rng.choice([1, 2]), "bt_size": rng.choice([40000, 100000])}),   # BT under the lazy parser
                           (5, {"lz_mode": 2, "hash_width": 4, "hash_bits": hb, "bt_size": 100000}),
                           (2, {"hash_width": rng.choice([10, 12, 16]), "hash_bits": hb, "lz_mode": rng.choice([1, 2])})])
    raise KeyError(row)


def _dict(rng, n, clamp):
    dsz = rng.choice([32 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20, 32 << 20, 64 << 20])
    if n > (64 << 10) and rng.random() < 0.4:
        dsz = max(32 << 10, min(dsz, n // rng.choice([2, 3, 5])))           # smaller than the input: the window wraps
    if clamp:
        dsz = max(32 << 10, min(dsz, n))            # (many streams: clamped to the input like csa_worker.cpp:35; device memory)
    return dsz


def _props_spec(rng, n, custom_p, small, clamp):
    spec = {}
    if rng.random() < custom_p:
        row = rng.choice(ROW_NAMES)
        level, over = _row_props(rng, row, small)
        spec.update(level=level, dict=_dict(rng, n, clamp), props=over)
    else:
        spec.update(level=rng.randrange(1, 6), dict=_dict(rng, n, clamp), props={})
    return spec


def _finish(spec):
    spec["row"] = spec_row(spec)
    return spec


class _Props:
    """enough of CSCProps for parser_bits without a library: CSCEncProps_Init restated (csc_enc.cpp:16-97, as oracle/orc_encoder.c)"""

    def __init__(self, dict_size, level):
        KB, MB = 1 << 10, 1 << 20
        d = min(max(dict_size + 10 * KB, 32 * KB), 1024 * MB)
        hb = 19 if d < MB else 20 if d <= 4 * MB else 21 if d <= 16 * MB else 22 if d <= 64 * MB else 23 if d <= 256 * MB else 24
        while (1 << hb) > d:
            hb -= 1
        self.bt_size = d if d <= 16 * MB else (d - 16 * MB) // 2 + 16 * MB if d <= 64 * MB else (d - 64 * MB) // 4 + 40 * MB \
            if d <= 256 * MB else (d - 256 * MB) // 8 + 88 * MB
        self.good_len, self.hash_bits, self.bt_hash_bits, self.bt_cyc = 32, hb, hb + 1, 0
        level = min(max(level, 1), 5)
        if level == 1:
            self.hash_width, self.lz_mode, self.bt_size, self.hash_bits = 1, 2, 0, hb + 1
        elif level == 2:
            self.hash_width, self.lz_mode, self.bt_size, self.good_len, self.hash_bits = 8, 2, 0, 24, hb - 1
        elif level == 3:
            self.hash_width, self.lz_mode, self.bt_size, self.good_len, self.hash_bits = 2, 3, 0, 16, hb + 1
        elif level == 4:
            self.hash_width, self.lz_mode, self.bt_size, self.good_len, self.hash_bits = 8, 3, 0, 24, hb - 1
        else:
            self.lz_mode, self.good_len, self.bt_cyc, self.hash_width = 3, 48, 32, 0


def spec_row(spec):
    """the dispatch row a spec selects (no library needed)"""
    p = _Props(spec["dict"], spec["level"])
    for k, v in spec.get("props", {}).items():
        setattr(p, k, v)
    return row_of(p)


# ---- the generators -----------------------------------------------------------------------------------------------

MAX_READS = [257, 511, 4095, 8191, 65537, RAW_BLOCKSIZE - 1]


def single_case(rng, size_cap=3 << 20):
    """one single-stream case (CSCEnc_Encode / CSCDec_Decode through the Read and Write callbacks)"""
    max_read = None
    if rng.random() < 0.25:
        max_read = rng.choice(MAX_READS + [None])
        if max_read is None:
            max_read = rng.randrange(257, RAW_BLOCKSIZE)
    cap = size_cap if max_read is None else min(size_cap, 256 * max_read)       # at most 256 Reads a case
    n = _size(rng, cap)
    spec = {"parts": _parts(rng, n)}
    spec.update(_props_spec(rng, n, 0.4, False, False))
    spec["nofilters"] = rng.random() < 0.25
    spec["max_read"] = max_read
    spec["dec_max_read"] = rng.choice([257, 1000, 4097, 65537, rng.randrange(257, 200_000)]) if rng.random() < 0.25 else None
    return _finish(spec)


def renorm_case(rng, size_range=(512 << 10, 3 << 19)):
    """a stream that crosses the match finder's renormalisation: 0.5-1.5 MiB, started 0 .. n positions before the line"""
    n = rng.randrange(*size_range)
    spec = {"parts": _parts(rng, n)}
    spec.update(_props_spec(rng, n, 0.5, False, False))
    spec["nofilters"] = rng.random() < 0.25
    spec["max_read"] = None
    spec["dec_max_read"] = None
    spec["pos"] = RENORM_LINE - rng.randrange(0, n + 1)
    return _finish(spec)


def batch_round(rng, max_streams=900, byte_cap=48_000_000):
    """the specs of one batch round (CSCMI_EncodeDeviceChunkBatch / CSCMI_FlushBatch / CSCMI_DecodeBatch): 2 .. max_streams
    streams, mixed levels and rows; rounds beyond 768 streams are of one row each (the regime past the pipeline / inserter
    forms' thresholds), the rest mixes up to every row in one call"""
    r = rng.random()
    hi = max(2, max_streams)
    if r < 0.6 or hi <= 40:
        S = rng.randrange(2, min(40, hi) + 1)
    elif r < 0.85 or hi <= 400:
        S = rng.randrange(41, min(400, hi) + 1)
    else:
        S = rng.randrange(min(769, hi), hi + 1)
    cap = max(1, min(5 << 20, byte_cap // S * 2))
    many = S > 40
    fixed = None
    if S > 400:
        fixed = rng.choice(["level3", "level3", "level12", "level5", "level4"])
    elif rng.random() < 0.3:
        fixed = rng.choice(ROW_NAMES)
    specs = []
    for _ in range(S):
        n = _size(rng, cap)
        spec = {"parts": _parts(rng, n)}
        if fixed is None:
            spec.update(_props_spec(rng, n, 0.25, many, many))
        else:
            default = {"level3": 3, "level4": 4, "level5": 5, "level12": rng.choice([1, 2])}.get(fixed)
            if default is not None and rng.random() < 0.7:
                spec.update(level=default, dict=_dict(rng, n, many), props={})
            else:
                level, over = _row_props(rng, fixed, many)
                spec.update(level=level, dict=_dict(rng, n, many), props=over)
        spec["nofilters"] = rng.random() < 0.15
        spec["max_read"] = None
        spec["dec_max_read"] = None
        specs.append(_finish(spec))
    return specs


# ---- the checker and the batch drivers ----------------------------------------------------------------------------

def checker():
    """(lib, zeroing allocator, is_reference): the reference build when oracle/_ref has it, the oracle otherwise"""
    from csc_amd.capi import CscLib
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libcsc_ref.so")
    chk = CscLib(ref_path if os.path.exists(ref_path) else os.path.join(ROOT, "oracle", "liborc.so"))
    o = C.CDLL(os.path.join(ROOT, "oracle", "liborc.so"))
    o.orc_zero_alloc.restype = C.c_void_p
    return chk, o.orc_zero_alloc(), os.path.exists(ref_path)


def check_one(chk, za, spec, data, set_pos=None):
    """the checker's stream for a spec and its own decoder's (rc, bytes) for that stream (with the spec's Read sizes on both sides)"""
    hook = None
    if spec.get("pos") is not None:
        hook = lambda h: set_pos(h, spec["pos"])         # noqa: E731
    rc, s = chk.encode(data, props=props_of(chk, spec), alloc=za, max_read=spec.get("max_read"), after_create=hook)
    rcd, back = chk.decode(s, alloc=za, max_read=spec.get("dec_max_read")) if rc == 0 else (rc, b"")
    return rc, s, rcd, back


class CSCMIStats(C.Structure):
    """include/csc_mi355x.h, CSCMIStats (the leading fields; the rest kept as padding)"""
    _fields_ = [("chunks", C.c_uint64), ("input_bytes", C.c_uint64), ("output_bytes", C.c_uint64),
                ("encode_launches", C.c_uint64), ("rest", C.c_uint64 * 8)]


def bind_batch(L):
    L.CSCMI_EncodeDeviceChunkBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.CSCMI_EncodeDeviceChunkBatch.restype = C.c_int
    L.CSCMI_FlushBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.CSCMI_FlushBatch.restype = C.c_int
    L.CSCMI_DecodeBatch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.CSCMI_DecodeBatch.restype = C.c_int
    L.CSCMI_GetStats.argtypes = [C.c_void_p, C.c_void_p]
    L.CSCMI_GetStats.restype = None
    return L


def encode_batch(prod, props, datas, chunk=CHUNK, stats=None):
    """Every stream through the batch entry points: one handle each, inputs resident in device memory, one
    CSCMI_EncodeDeviceChunkBatch per chunk round over the streams that still have bytes, then one CSCMI_FlushBatch.
    Returns (streams, chunk rounds).  `stats`, a list, receives the lead handle's CSCMIStats before the flush.  `chunk` may be
    a list, one chunk size a stream (streams whose props carry their own raw_blocksize)."""
    import torch
    from csc_amd.capi import BytesWriter
    L = bind_batch(prod.lib)
    S = len(datas)
    chunks = list(chunk) if isinstance(chunk, (list, tuple)) else [chunk] * S
    hs, ws, devs = [], [], []
    try:
        for p, d in zip(props, datas):
            w = BytesWriter()
            h = L.CSCEnc_Create(C.byref(p), C.cast(w.ptr(), C.c_void_p), None)
            assert h, "CSCEnc_Create returned NULL"
            w.out += prod.write_properties(p)
            hs.append(h); ws.append(w)
            devs.append(torch.frombuffer(bytearray(d) if d else bytearray(1), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        k = 0
        while True:
            Z = [max(0, min(c, len(d) - k * c)) for c, d in zip(chunks, datas)]
            live = [i for i in range(S) if Z[i] > 0]
            if not live:
                break
            H = (C.c_void_p * len(live))(*[hs[i] for i in live])
            P = (C.c_void_p * len(live))(*[devs[i].data_ptr() + k * chunks[i] for i in live])
            rc = L.CSCMI_EncodeDeviceChunkBatch(len(live), H, P, (C.c_size_t * len(live))(*[Z[i] for i in live]))
            assert rc == 0, f"CSCMI_EncodeDeviceChunkBatch round {k}: {rc}"
            k += 1
        if stats is not None:
            st = CSCMIStats()
            L.CSCMI_GetStats(hs[0], C.byref(st))
            stats.append(st)
        rc = L.CSCMI_FlushBatch(S, (C.c_void_p * S)(*hs))
        assert rc == 0, f"CSCMI_FlushBatch: {rc}"
    finally:
        for h in hs:
            L.CSCEnc_Destroy(h)
    return [bytes(w.out) for w in ws], k


def decode_batch(prod, streams, group=256):
    """CSCMI_DecodeBatch over `streams`, `group` handles a call: [(rc, bytes)] like CscLib.decode ((None, b"") where
    CSCDec_Create refuses the stream)"""
    from csc_amd.capi import BytesReader, BytesWriter, CSC_PROP_SIZE
    L = bind_batch(prod.lib)
    out = [None] * len(streams)
    for a in range(0, len(streams), group):
        part, rs, dws, dhs = [], [], [], []
        for i in range(a, min(len(streams), a + group)):
            props = prod.read_properties(streams[i][:CSC_PROP_SIZE])
            r = BytesReader(streams[i][CSC_PROP_SIZE:]); w = BytesWriter()
            h = L.CSCDec_Create(C.byref(props), C.cast(r.ptr(), C.c_void_p), None)
            if not h:
                out[i] = (None, b"")
                continue
            part.append(i); rs.append(r); dws.append(w); dhs.append(h)
        if not part:
            continue
        R = (C.c_int * len(part))()
        try:
            rc = L.CSCMI_DecodeBatch(len(part), (C.c_void_p * len(part))(*dhs),
                                     (C.c_void_p * len(part))(*[C.cast(w.ptr(), C.c_void_p) for w in dws]), R)
        finally:
            for h in dhs:
                L.CSCDec_Destroy(h)
        assert rc == 0, f"CSCMI_DecodeBatch: {rc}"
        for j, i in enumerate(part):
            out[i] = (R[j], bytes(dws[j].out))
    return out
