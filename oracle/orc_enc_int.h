/*
 * oracle/orc_enc_int.h -- the oracle encoder's state and its coder / model primitives, shared between
 * orc_encoder.c (which defines them) and orc_synth.c (which drives them from a script).
 *
 * TEST INFRASTRUCTURE, internal to liborc.so: ORC_INT symbols are not exported.
 */
#ifndef ORC_ENC_INT_H_
#define ORC_ENC_INT_H_

#include <setjmp.h>

#include "orc_api.h"

#define ORC_INT __attribute__((visibility("hidden")))

#define KB 1024u
#define MB 1048576u
#define MIN_BLOCK (8u * KB)       /* csc_typedef.h:9 MinBlockSize */
#define UMIN(a, b) ((a) < (b) ? (a) : (b))

/* block types, csc_typedef.h:20-40 */
enum {
    DT_NORMAL = 1, DT_ENGTXT = 2, DT_EXE = 3, DT_FAST = 4, DT_NO_LZ = 5,
    DT_ENTROPY = 7, DT_BAD = 8, SIG_EOF = 9, DT_DLT = 0x10, DT_SKIP = 0x1E
};

#define HT2_SIZE (16u * KB)       /* csc_mf.h:18 */
#define HT3_SIZE (64u * KB)       /* csc_mf.h:17 */
#define MF_CAND_LIMIT 32          /* csc_mf.h:34 */
#define AP_LIMIT 2048             /* csc_lz.h:43 */

typedef struct { uint32_t len; uint32_t dist; } MFUnit; /* len doubles as price, csc_mf.h:8-14 */

typedef struct {
    uint32_t dist, state;
    int back_pos, next_pos;
    uint32_t price, lit;
    uint32_t rep_dist[4];
} APUnit; /* csc_lz.h:33-41 */

typedef struct {
    uint32_t next[26];
    uint8_t symbol;
} TrieNode; /* csc_filters.h:30-33 */

typedef struct OrcEnc {
    ISzAlloc *alloc;
    ISeqOutStream *os;
    CSCProps props;
    jmp_buf on_error;             /* replaces `throw (int)` of csc_coder.h:11 */

    /* ---- MemIO + Coder, csc_coder.h:15-64 ---- */
    uint32_t bsize;
    uint8_t *rc_buf, *bc_buf;
    uint32_t rc_size, bc_size;
    uint64_t rc_low, rc_cachesize;
    uint32_t rc_range;
    uint8_t rc_cache;
    uint32_t bc_curbits, bc_curval;
    int64_t outsize;

    /* ---- Model, csc_model.h:58-122 ---- */
    uint32_t p_state[64 * 3];
    uint32_t state, ctx;
    uint32_t p_rle_flag;
    uint32_t *p_lit, *p_delta;
    uint32_t p_repdist[64 * 4];
    uint32_t p_dist[8 + 16 * 2 + 32 * 4];
    uint32_t p_longlen;
    uint32_t p_2_bits[512];
    uint32_t p_len_slot[2], p_len_x1[8], p_len_x2[8], p_len_x3[128];
    uint32_t p_dist_extra[29 * 16];
    uint32_t len_price[32];
    uint32_t lp_rebuild_int;

    /* ---- MatchFinder, csc_mf.h:16-53 ---- */
    uint8_t *wnd;
    uint32_t wnd_size, vld_rge;
    uint32_t *mfbuf, *ht2, *ht3, *ht6, *bt_head, *bt_nodes;
    uint64_t mf_size;
    uint32_t ht_bits, ht_width, ht_low;
    uint32_t bt_bits, bt_size, bt_pos;
    uint32_t ht_cyc, bt_cyc, good_len;
    uint32_t pos;
    MFUnit mfcand[MF_CAND_LIMIT];

    /* ---- LZ, csc_lz.h:19-56 ---- */
    uint32_t wnd_curpos;
    uint32_t rep_dist[4];
    uint32_t lz_good_len, lz_bt_cyc, lz_ht_cyc;
    MFUnit *appt;
    APUnit *ap;

    /* ---- Analyzer, csc_analyzer.h:19 ---- */
    uint32_t log_table[(MIN_BLOCK >> 4) + 1];

    /* ---- Filters, csc_filters.h:26-62 ---- */
    TrieNode trie[300];
    uint8_t *swap_buf;
    uint32_t swap_size;
    uint32_t x0, x1, ei, ek;
    uint8_t ecs;

    /* ---- walk trace (orc_trace_*; NULL unless a test attached one) ---- */
    struct OrcTrace *trace;

    /* ---- census (orc_census_attach; NULL unless a test attached one): ORC_EV_COUNT counters ---- */
    uint64_t *census;
} OrcEnc;

/* count one event of the census (orc_api.h, enum OrcEvent) */
#define ORC_EV(e, ev) do { if (__builtin_expect((e)->census != NULL, 0)) (e)->census[ev]++; } while (0)

ORC_INT int write_block(OrcEnc *e, uint8_t *buf, uint32_t size, int rc1bc0);
ORC_INT void coder_reset_state(OrcEnc *e);
ORC_INT void rc_shift_low(OrcEnc *e);
ORC_INT void enc_direct16(OrcEnc *e, uint32_t val, uint32_t len);
ORC_INT void enc_direct(OrcEnc *e, uint32_t v, uint32_t l);
ORC_INT void coder_flush(OrcEnc *e);
ORC_INT void fill_probs(uint32_t *p, int n);
ORC_INT void encode_matchlen_2(OrcEnc *e, uint32_t len);
ORC_INT void encode_byte_tree(OrcEnc *e, uint32_t *row, uint32_t c);
ORC_INT void encode_literal(OrcEnc *e, uint32_t c);
ORC_INT void encode_rep0len1(OrcEnc *e);
ORC_INT void encode_rep_match(OrcEnc *e, uint32_t rep_idx, uint32_t match_len);
ORC_INT void encode_match(OrcEnc *e, uint32_t dist, uint32_t len);
ORC_INT void encode_int(OrcEnc *e, uint32_t num);
ORC_INT void compress_literals(OrcEnc *e, const uint8_t *src, uint32_t size);
ORC_INT void compress_bad(OrcEnc *e, const uint8_t *src, uint32_t size);
ORC_INT void model_reset(OrcEnc *e);
ORC_INT void rle_begin(OrcEnc *e, uint32_t size);
ORC_INT void rle_lit(OrcEnc *e, uint32_t sctx, uint32_t c);
ORC_INT void rle_run(OrcEnc *e, uint32_t len);

/* EncodeBit macro, csc_coder.h:67-81 */
static inline void enc_bit(OrcEnc *e, uint32_t v, uint32_t *p)
{
    uint32_t bound = (e->rc_range >> 12) * *p;
    if (v) {
        e->rc_range = bound;
        *p += (0xFFF - *p) >> 5;
    } else {
        e->rc_low += bound;
        e->rc_range -= bound;
        *p -= *p >> 5;
    }
    if (e->rc_range < (1u << 24)) {
        e->rc_range <<= 8;
        rc_shift_low(e);
    }
}

#endif
