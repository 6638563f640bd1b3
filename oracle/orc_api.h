/*
 * oracle/orc_api.h -- C view of the libcsc boundary, used ONLY by the oracle.
 *
 * TEST INFRASTRUCTURE.  Nothing under oracle/ is part of the product: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.
 *
 * Restates the public types of the reference boundary:
 *   CSCProps             /root/reference/src/libcsc/csc_common.h:19-63
 *   ISeqInStream         /root/reference/src/libcsc/Types.h:137-142
 *   ISeqOutStream        /root/reference/src/libcsc/Types.h:149-154
 *   ICompressProgress    /root/reference/src/libcsc/Types.h:220-225
 *   ISzAlloc             /root/reference/src/libcsc/Types.h:227-231
 *   error codes          /root/reference/src/libcsc/csc_common.h:13-17
 *
 * Beside the boundary, oracle-only probes (none of them in the product):
 *   orc_analyze_block .. orc_tables   single stages, for intermediate goldens
 *   orc_trace_*                       the chunk walk's and TestFind's decisions during an encode (tests/walk_cases.py)
 *   orc_synth                         a script of packets -> a stream body
 */
#ifndef ORC_API_H_
#define ORC_API_H_

#include <stddef.h>
#include <stdint.h>

#define CSC_PROP_SIZE 10
#define DECODE_ERROR (-96)
#define WRITE_ERROR (-97)
#define READ_ERROR (-98)
#define CSC_WRITE_ABORT ((size_t)-1)

typedef int SRes;

typedef struct { SRes (*Read)(void *p, void *buf, size_t *size); } ISeqInStream;
typedef struct { size_t (*Write)(void *p, const void *buf, size_t size); } ISeqOutStream;
typedef struct { SRes (*Progress)(void *p, uint64_t in_size, uint64_t out_size); } ICompressProgress;
typedef struct {
    void *(*Alloc)(void *p, size_t size);
    void (*Free)(void *p, void *address);
} ISzAlloc;

typedef struct _CSCProps {
    size_t dict_size;
    uint32_t csc_blocksize;
    uint32_t raw_blocksize;
    uint8_t hash_bits;
    uint8_t hash_width;
    uint8_t bt_hash_bits;
    uint32_t bt_size;
    uint32_t bt_cyc;
    uint8_t good_len;
    uint8_t lz_mode;
    uint8_t DLTFilter;
    uint8_t TXTFilter;
    uint8_t EXEFilter;
} CSCProps;

typedef void *CSCEncHandle;
typedef void *CSCDecHandle;

void CSCEncProps_Init(CSCProps *p, uint32_t dict_size, int level);
void CSCEnc_WriteProperties(const CSCProps *props, uint8_t *stream, int full);
uint64_t CSCEnc_EstMemUsage(const CSCProps *props);
CSCEncHandle CSCEnc_Create(const CSCProps *props, ISeqOutStream *outstream, ISzAlloc *alloc);
void CSCEnc_Destroy(CSCEncHandle p);
int CSCEnc_Encode(CSCEncHandle p, ISeqInStream *instream, ICompressProgress *progress);
int CSCEnc_Encode_Flush(CSCEncHandle p);

void CSCDec_ReadProperties(CSCProps *props, uint8_t *stream);
CSCDecHandle CSCDec_Create(const CSCProps *props, ISeqInStream *instream, ISzAlloc *alloc);
void CSCDec_Destroy(CSCDecHandle p);
int CSCDec_Decode(CSCDecHandle p, ISeqOutStream *outstream, ICompressProgress *progress);

/* ---- oracle-only probes (intermediate goldens; not part of the boundary) ---- */
/* Analyzer::Analyze on one <=8 KiB block: returns type, writes bpb (untouched for DT_SKIP). */
uint32_t orc_analyze_block(const uint8_t *src, uint32_t size, uint32_t *bpb);
uint32_t orc_dlt_bpb(const uint8_t *src, uint32_t size, uint32_t chn);
void orc_forward_e89(uint8_t *buf, uint32_t size);
void orc_inverse_e89(uint8_t *buf, uint32_t size);
uint32_t orc_forward_dict(uint8_t *buf, uint32_t size);
void orc_inverse_dict(uint8_t *buf, uint32_t size);
void orc_forward_delta(uint8_t *buf, uint32_t size, uint32_t chn);
void orc_inverse_delta(uint8_t *buf, uint32_t size, uint32_t chn);
/* the two float-built tables */
void orc_tables(uint32_t p2bits[512], uint32_t logtab[513]);

/* ---- walk trace: what CSCEncoder::Compress and MatchFinder::TestFind decided while a stream was encoded.  Off unless a
 * trace is attached to the handle right after CSCEnc_Create; rows are plain uint32 words, widths below.
 *   ORC_TRACE_BLOCK  per 8 KiB block: chunk, block, offset, size, analyzer type, bpb in force, GetDltBpb x 5 (1, 2, 3, 4, 8
 *                    channels), the GetDltBpb figure the 0.95 rule used (0xFFFFFFFF: rule not reached), type after DT_SKIP
 *                    inheritance, after the filter switches, after the 0.95 rule, final type, duplicate verdict (2: not asked)
 *   ORC_TRACE_CAND   per candidate TestFind looked at: chunk, block, offset i in the block, table (0: HT6 slot 0, 1: BT head),
 *                    dist, vld_rge, cmp_pos, limit, wnd_size - cmp_pos, equal bytes (counted on past the window's end into its
 *                    eight bytes of slack, up to min(limit, 64); all three 0 where dist > wnd_size), hit
 *   ORC_TRACE_RUN    per run handed to compress_block: chunk, type, offset, size, tail (EncodeInt after it) */
enum { ORC_TRACE_BLOCK = 0, ORC_TRACE_CAND = 1, ORC_TRACE_RUN = 2 };
enum { ORC_TRACE_BLOCK_W = 17, ORC_TRACE_CAND_W = 11, ORC_TRACE_RUN_W = 5 };
struct OrcTrace;
struct OrcTrace *orc_trace_new(void);
void orc_trace_attach(CSCEncHandle h, struct OrcTrace *t);
const uint32_t *orc_trace_rows(const struct OrcTrace *t, int kind, size_t *count);
void orc_trace_free(struct OrcTrace *t);

/* ---- census: how often the encoder took each named rare branch of the reference while a stream was encoded (tests/census_cases.py,
 * tools/make_census_cases.py).  Off unless a counter array of ORC_EV_COUNT words is attached to the handle right after CSCEnc_Create
 * (NULL detaches); per handle, so encodes on several threads do not share counters.  Detached, an event costs one predictable branch.
 * Each event is defined where it is counted in orc_encoder.c, beside the reference lines of its branch. */
enum OrcEvent {
    /* coder */
    ORC_EV_RC_CARRY_CACHE2,       /* a carry propagated through cache byte + >= 1 FF byte (rc_cachesize >= 2) */
    ORC_EV_RC_CARRY_CACHE3,       /* ... through >= 2 FF bytes */
    ORC_EV_RC_FF_RUN2,            /* rc_cachesize >= 2 flushed without a carry (FF bytes really written) */
    ORC_EV_RC_SEAM,               /* an RC block filled */
    ORC_EV_RC_SEAM_MID,           /* ... with bytes of the same RC_ShiftLow emission still to come */
    ORC_EV_BC_SEAM,               /* a BC block filled */
    ORC_EV_RC_BC_SEAM_PACKET,     /* both inside one packet (EncodeMatch is the only packet that feeds both coders) */
    ORC_EV_FLUSH,
    ORC_EV_FLUSH_STALE_NZ,        /* the byte Flush counts but never stores is not zero in the buffer */
    ORC_EV_FLUSH_BSIZE_M1,        /* Flush arrives at rc_size + 1 == csc_blocksize: the short header goes missing */
    ORC_EV_FLUSH_AFTER_SEAM,      /* Flush's five bytes end exactly on a seam (rc_size == 0) */
    ORC_EV_FLUSH_BC_EMPTY,        /* Flush's two BC bytes end exactly on a seam: an empty BC block is written, which the decoder refuses */
    /* model */
    ORC_EV_LEN_CHAIN1,            /* match length 143 .. 285: the 143 escape once */
    ORC_EV_LEN_CHAIN2,            /* >= 286: the p_longlen loop runs */
    ORC_EV_LEN_PRICE_REBUILD,
    /* MatchFinder::SlidePos */
    ORC_EV_SP_SKIP,               /* i + 128 < len: four positions a step, no bucket / tree insert */
    ORC_EV_SP_NOSHIFT,            /* h6 == lasth6: slot 0 overwritten without shifting the bucket */
    ORC_EV_SP_BT_POS_WRAP,
    ORC_EV_SP_BT_CYC,             /* descent ended by cyc >= bt_cyc */
    ORC_EV_SP_GOOD_LEN_SPLICE,    /* clen >= good_len: the node takes the matched node's children */
    ORC_EV_SP_CLIMIT_WND,         /* climit set by the window's end, not by the block */
    /* MatchFinder::find_match */
    ORC_EV_FM_REP_RANGE,          /* rep distance >= vld_rge skipped */
    ORC_EV_FM_REP_GOOD_LEN,       /* a rep match >= good_len ends the search */
    ORC_EV_FM_REP_WRAPPED,        /* rep compare position on the far side of the window's wrap */
    ORC_EV_FM_CLIMIT_WND,         /* climit set by the window's end (any table) */
    ORC_EV_FM_HT2_WPOS_EQ_DIST,   /* HT2's strict compare: wpos == dist names wnd_size, not 0 */
    ORC_EV_FM_KBOUND_HT23,        /* a short match rejected by kBound: HT2 / HT3 */
    ORC_EV_FM_KBOUND_BT_HEAD,     /* ... the head candidate beyond the tree range */
    ORC_EV_FM_KBOUND_BT,          /* ... in the descent */
    ORC_EV_FM_KBOUND_HT6,         /* ... in the bucket */
    ORC_EV_FM_BT_HEAD_BEYOND,     /* head candidate with bt_size <= dist < vld_rge compared */
    ORC_EV_FM_BT_CYC,             /* descent ended by cyc >= bt_cyc */
    ORC_EV_FM_BT_GOOD_LEN_SPLICE,
    ORC_EV_FM_CAND_OVERFLOW,      /* cnt + 2 < MF_CAND_LIMIT false: the slot is overwritten */
    /* MatchFinder::FindMatchWithPrice */
    ORC_EV_FMP_KBOUND_ZERO,       /* a length's entry zeroed by kBound */
    /* lazy parser: the preference predicate (FindMatch's candidate choice and the lazy step), by deciding clause */
    ORC_EV_LAZY_CLAUSE1, ORC_EV_LAZY_CLAUSE2, ORC_EV_LAZY_CLAUSE3, ORC_EV_LAZY_CLAUSE4, ORC_EV_LAZY_CLAUSE5,
    ORC_EV_LAZY_SECOND_TWICE,     /* the later match preferred at two positions running */
    /* advanced parser */
    ORC_EV_AP_LITERAL_NO_WINDOW,  /* no candidate: a literal without opening a window */
    ORC_EV_AP_EXIT_LITERAL,
    ORC_EV_AP_EXIT_GOOD_LEN,
    ORC_EV_AP_EXIT_APLIMIT_LEN,   /* a match that reaches aplimit */
    ORC_EV_AP_LIMIT_TAIL,         /* aplimit < AP_LIMIT: the sub-block's tail */
    ORC_EV_AP_REP0LEN1_CODED,     /* the back trace codes a rep0len1 */
    ORC_EV_AP_CUR_EQ_LIMIT,       /* apcur == aplimit (argued dead in orc_encoder.c) */
    ORC_EV_AP_FIRST_REP0LEN1,     /* a first node whose last candidate is rep0len1 (argued dead in orc_encoder.c) */
    /* LZ::EncodeNormal */
    ORC_EV_LZ_WND_WRAP,
    ORC_EV_COUNT
};
void orc_census_attach(CSCEncHandle h, uint64_t *counts);
const char *orc_census_name(int ev);

/* ---- an ISeqOutStream that collects in C (zalloc.c), for streams of so many Write calls that a Python callback is too slow ---- */
ISeqOutStream *orc_sink_new(void);
const uint8_t *orc_sink_data(const ISeqOutStream *s, size_t *size);
void orc_sink_free(ISeqOutStream *s);

/* ---- stream synthesizer (orc_synth.c): a script of packets -> a stream body, through the oracle's coder and model ---- */
enum {
    ORC_OP_BLOCK = 1, ORC_OP_LIT, ORC_OP_MATCH, ORC_OP_REP, ORC_OP_REP0LEN1, ORC_OP_END_RUN, ORC_OP_RESTART,
    ORC_OP_BAD, ORC_OP_ENTROPY, ORC_OP_DLT, ORC_OP_RLE_LIT, ORC_OP_RLE_RUN, ORC_OP_EOF, ORC_OP_RAW_TYPE,
    ORC_OP_LITS, ORC_OP_FLUSH
};
int orc_synth(const CSCProps *props, const uint32_t *script, size_t words, ISeqOutStream *out, ISzAlloc *alloc);

#endif
