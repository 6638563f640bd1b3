"""The encoder census: named rare branches of the reference's coder, model, match finder and parsers (oracle/orc_api.h, enum
OrcEvent), counted inside the oracle while it encodes, and the frozen cases that provably reach them.  Shared by
tools/make_census_cases.py (the seeded search that writes tests/golden/census_cases.json), tests/test_census_host.py (the
coverage claim, on the CPU) and tests/test_gpu_census.py (the cases through every kernel form).  Not a conftest: a plain module
the tests import like `cases`.

A case is {"name", "row", "spec", "size", "events", "decodes"}: `spec` in soak_gen form (parts, level, dict, props -- csc_blocksize among
the props where a coder event needs small blocks), `events` the counts the oracle recorded for the events the case was picked
for, `decodes` whether the checker's decoder reads the checker's stream (not below the block-size floor, not where a Flush left an
empty BC block).  The golden file holds no input bytes."""
import ctypes as C
import json
import os

import soak_gen
import test_gpu_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "census_cases.json")

ROWS = list(soak_gen.ROW_NAMES)
BT_ROWS = ["level5", "adv_generic", "lazy_generic"]                   # rows whose props can carry a binary tree
BUCKET_ROWS = [r for r in ROWS if r != "level5"]                      # rows whose props can carry a bucket
LAZY_ROWS = ["level12", "lazy_w9", "lazy_generic"]
ADV_ROWS = ["level3", "level4", "level5", "adv_generic"]
# rows in which find_match can push 30 candidates at one position: rep0len1 + 4 reps + HT2 + HT3 is 7, a bucket of up to nine makes
# 16, so only a tree descent (one candidate a step, bt_cyc steps) or a bucket wider than 22 gets there: the rows with a tree, which
# are also the two rows that take buckets wider than nine
OVERFLOW_ROWS = BT_ROWS

CODER = ["rc_carry_cache2", "rc_carry_cache3", "rc_ff_run2", "rc_seam", "rc_seam_mid", "bc_seam", "rc_bc_seam_packet",
         "flush", "flush_stale_nz", "flush_bsize_m1", "flush_after_seam", "flush_bc_empty"]

# event -> the rows in which its branch exists (enum order, oracle/orc_api.h; test_census_host checks the names against the oracle's)
APPLIES = {}
APPLIES.update({ev: ROWS for ev in CODER})
APPLIES.update({"len_chain1": ROWS, "len_chain2": ROWS, "len_price_rebuild": ADV_ROWS})
APPLIES.update({"sp_skip": ROWS, "sp_noshift": BUCKET_ROWS, "sp_bt_pos_wrap": BT_ROWS, "sp_bt_cyc": BT_ROWS,
                "sp_good_len_splice": BT_ROWS, "sp_climit_wnd": BT_ROWS})
APPLIES.update({"fm_rep_range": ROWS, "fm_rep_good_len": ROWS, "fm_rep_wrapped": ROWS, "fm_climit_wnd": ROWS,
                "fm_ht2_wpos_eq_dist": ROWS, "fm_kbound_ht23": ROWS, "fm_kbound_bt_head": BT_ROWS, "fm_kbound_bt": BT_ROWS,
                "fm_kbound_ht6": BUCKET_ROWS, "fm_bt_head_beyond": BT_ROWS, "fm_bt_cyc": BT_ROWS,
                "fm_bt_good_len_splice": BT_ROWS, "fm_cand_overflow": OVERFLOW_ROWS})
APPLIES.update({"fmp_kbound_zero": ADV_ROWS})
APPLIES.update({ev: LAZY_ROWS for ev in ["lazy_clause1", "lazy_clause2", "lazy_clause3", "lazy_clause4", "lazy_clause5",
                                         "lazy_second_twice"]})
APPLIES.update({ev: ADV_ROWS for ev in ["ap_literal_no_window", "ap_exit_literal", "ap_exit_good_len", "ap_exit_aplimit_len",
                                        "ap_limit_tail", "ap_rep0len1_coded", "ap_cur_eq_limit", "ap_first_rep0len1"]})
APPLIES.update({"lz_wnd_wrap": ROWS})
EVENTS = list(APPLIES)

# events no input reaches: dead branches of the reference (the arguments stand beside the events in oracle/orc_encoder.c)
DEAD = {
    "ap_cur_eq_limit": "a window leaves through the literal exit or the aplimit exit at apcur == aplimit - 1 at the latest",
    "ap_first_rep0len1": "find_match pushes the rep0 match itself right behind every rep0len1, so rep0len1 is never the last candidate",
}

MAX_CASE = 128 << 10                  # a case's input
MAX_ROW = 1 << 20                     # the inputs of one row's cases together

# (event, row) cells without a case, each with its reason.  test_census_host holds this table to its cap: beside DEAD, at most two
# reachable events open in every row, any other event open in at most one row, no coder event at all.
OPEN = {
}

# ---- the block-size family: one mixed input (text, random, zeros: both coders fill blocks), every row, csc_blocksize 16 / 17 / 255 /
# 4096.  The encoder's Read returns 2048 bytes a call, so a stream has twelve chunks and as many flushes: with one flush the chance
# that rc_size + 1 == csc_blocksize in all seven rows at once is nil, with twelve a seed is found within a few tries (805 was the
# first of 800 .. 859 that hits FAMILY_MUST_HIT in every row; tests/test_census_host.py asserts it from the census).  And 1 / 3 on two
# texts, below the floor from which the reference's decoder reads the reference's own streams: encode-only members.
FAMILY_PARTS = [["text", 805, 0, 8192], ["random", 806, 0, 8192], ["zeros", 4000], ["text", 805, 50000, 3616]]
FAMILY_READ = 2048
FAMILY_BSIZES = [16, 17, 255, 4096]
FAMILY_MUST_HIT = ["rc_seam", "bc_seam", "rc_seam_mid", "flush_bsize_m1", "flush_stale_nz"]
FAMILY_BELOW_FLOOR = [(1, [["text", 813, 0, 3000]]), (3, [["text", 813, 0, 3000]]),
                      (1, [["text", 814, 0, 20000]]), (3, [["text", 814, 0, 20000]])]
FAMILY_DEVICE_BATCH_BSIZE = 17        # the member that also runs through CSCMI_EncodeDeviceBatch


ROW_VARIANTS = {row: f["variants"] for row, f in test_gpu_forms.FORMS.items()}        # the (level, overrides) that select a row


def row_variant(row, k=0):
    return ROW_VARIANTS[row][k % len(ROW_VARIANTS[row])]


def family_members(row):
    """the block-size family of a row: [(member name, spec)]"""
    level, over = row_variant(row)
    out = []
    for b in FAMILY_BSIZES:
        out.append((f"bsize{b}", {"parts": FAMILY_PARTS, "level": level, "dict": 32768, "props": dict(over, csc_blocksize=b),
                                  "max_read": FAMILY_READ, "row": row}))
    for b, parts in FAMILY_BELOW_FLOOR:
        out.append((f"bsize{b}-text{parts[0][3]}", {"parts": parts, "level": level, "dict": 32768, "props": dict(over, csc_blocksize=b),
                                                    "row": row}))
    return out


def family_specs(row):
    """[(member id, spec, decodes)]: `decodes` as recorded in the golden file -- whether the checker's decoder reads the checker's
    stream (not below the floor, and not where a Flush left an empty BC block); the id says so"""
    rec = load()["family"][row]
    return [(name + ("" if rec[name]["decodes"] else "-encode-only"), spec, rec[name]["decodes"]) for name, spec in family_members(row)]


_loaded = None


def load():
    global _loaded
    if _loaded is None:
        with open(GOLDEN) as f:
            _loaded = json.load(f)
    return _loaded


def cases_of(row):
    return [c for c in load()["cases"] if c["row"] == row]


# ---- running the oracle with the census attached ------------------------------------------------------------------

def bind(orc):
    """liborc.so's census entry points on a CscLib"""
    L = orc.lib
    L.orc_census_attach.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.orc_census_attach.restype = None
    L.orc_census_name.argtypes = [C.c_int]
    L.orc_census_name.restype = C.c_char_p
    return L


def oracle_names(orc):
    L = bind(orc)
    out = []
    while True:
        n = L.orc_census_name(len(out))
        if n is None:
            return out
        out.append(n.decode())


class CSink:
    """a `writer` for CscLib.encode that collects in C (liborc.so, orc_sink_*): no Python callback per Write call"""

    def __init__(self):
        self.L = L = C.CDLL(os.path.join(ROOT, "oracle", "liborc.so"))
        L.orc_sink_new.restype = C.c_void_p
        L.orc_sink_data.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.orc_sink_data.restype = C.c_void_p
        L.orc_sink_free.argtypes = [C.c_void_p]
        self.p = L.orc_sink_new()
        self.out = bytearray()              # (the property bytes, which CscLib.encode puts in front itself)

    def ptr(self):
        return C.c_void_p(self.p)

    def take(self):
        """the whole stream; frees the sink"""
        n = C.c_size_t()
        d = self.L.orc_sink_data(self.p, C.byref(n))
        s = bytes(self.out) + (C.string_at(d, n.value) if n.value else b"")
        self.L.orc_sink_free(self.p)
        self.p = None
        return s


def census(orc, za, spec, data=None):
    """(rc, stream, {event: count}) of the oracle's encode of a spec"""
    L = bind(orc)
    if data is None:
        data = soak_gen.build_input(spec)
    counts = (C.c_uint64 * len(EVENTS))()
    rc, s = orc.encode(data, props=soak_gen.props_of(orc, spec), alloc=za, max_read=spec.get("max_read"),
                       after_create=lambda h: L.orc_census_attach(h, counts))
    return rc, s, {ev: int(counts[i]) for i, ev in enumerate(EVENTS)}
