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

/* ---- stream synthesizer (orc_synth.c): a script of packets -> a stream body, through the oracle's coder and model ---- */
enum {
    ORC_OP_BLOCK = 1, ORC_OP_LIT, ORC_OP_MATCH, ORC_OP_REP, ORC_OP_REP0LEN1, ORC_OP_END_RUN, ORC_OP_RESTART,
    ORC_OP_BAD, ORC_OP_ENTROPY, ORC_OP_DLT, ORC_OP_RLE_LIT, ORC_OP_RLE_RUN, ORC_OP_EOF, ORC_OP_RAW_TYPE,
    ORC_OP_LITS, ORC_OP_FLUSH
};
int orc_synth(const CSCProps *props, const uint32_t *script, size_t words, ISeqOutStream *out, ISzAlloc *alloc);

#endif
