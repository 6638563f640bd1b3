/*
 * csc_mi355x.h -- C ABI of libcsc_mi355x.so, the MI355X-native drop-in for the libcsc
 * encode/decode path of fusiyuan2010/CSC.
 *
 * The eleven CSCEnc_ / CSCDec_ entry points are exactly the ones the reference exports
 * (inside EXTERN_C_BEGIN/END, compiled with -D_7Z_TYPES_); each declaration cites the reference
 * interface it replaces.  Plain pointers and sizes only -- no C++ or torch types cross this line,
 * and no C++ exception crosses it either.
 *
 *   reference header                      what it declares
 *   src/libcsc/csc_common.h:11-63         CSC_PROP_SIZE, error codes, CSC_WRITE_ABORT, CSCProps
 *   src/libcsc/Types.h:137-154,220-231    ISeqInStream, ISeqOutStream, ICompressProgress, ISzAlloc
 *   src/libcsc/csc_enc.h:11-30            CSCEncProps_Init .. CSCEnc_Encode_Flush
 *   src/libcsc/csc_dec.h:8-21             CSCDec_ReadProperties .. CSCDec_Decode
 *
 * A program that already includes the reference's csc_enc.h / csc_dec.h / Types.h can keep
 * including those and just link against this library: the struct layouts below are identical.
 */
#ifndef CSC_MI355X_H_
#define CSC_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSC_PROP_SIZE (4 + 3 + 3)          /* csc_common.h:11 */
#define DECODE_ERROR (-96)                 /* csc_common.h:13 */
#define WRITE_ERROR (-97)                  /* csc_common.h:14 */
#define READ_ERROR (-98)                   /* csc_common.h:15 */
#define CSC_WRITE_ABORT ((size_t)-1)       /* csc_common.h:17 */
/* Not in the reference: the GPU side failed (no device, HIP error, output arena exhausted, or the watchdog of the
 * multi-wavefront parser tripped -- a bug, reported instead of hanging the GPU).
 * Returned by CSCEnc_Encode / CSCEnc_Encode_Flush only; details go to stderr. */
#define CSCMI_DEVICE_ERROR (-95)

#ifndef CSC_MI355X_NO_7Z_TYPES            /* define this if the reference's Types.h is included already */
typedef int SRes;
typedef struct { SRes (*Read)(void *p, void *buf, size_t *size); } ISeqInStream;          /* Types.h:137-142 */
typedef struct { size_t (*Write)(void *p, const void *buf, size_t size); } ISeqOutStream; /* Types.h:149-154 */
typedef struct { SRes (*Progress)(void *p, uint64_t inSize, uint64_t outSize); } ICompressProgress; /* Types.h:220-225 */
typedef struct {                                                                            /* Types.h:227-231 */
    void *(*Alloc)(void *p, size_t size);
    void (*Free)(void *p, void *address); /* address can be 0 */
} ISzAlloc;
#endif

typedef struct _CSCProps {                 /* csc_common.h:19-63, field for field */
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

typedef void *CSCEncHandle;                /* csc_enc.h:17 */
typedef void *CSCDecHandle;                /* csc_dec.h:10 */

/* ---- encoder, csc_enc.h ---- */
void CSCEncProps_Init(CSCProps *p, uint32_t dict_size, int level);                 /* csc_enc.h:11  (C++ defaults 64000000 / 2) */
void CSCEnc_WriteProperties(const CSCProps *props, uint8_t *stream, int full);     /* csc_enc.h:13 */
uint64_t CSCEnc_EstMemUsage(const CSCProps *props);                                /* csc_enc.h:15 */
CSCEncHandle CSCEnc_Create(const CSCProps *props, ISeqOutStream *outstream, ISzAlloc *alloc); /* csc_enc.h:20-22 */
void CSCEnc_Destroy(CSCEncHandle p);                                               /* csc_enc.h:24 */
int CSCEnc_Encode(CSCEncHandle p, ISeqInStream *instream, ICompressProgress *progress);       /* csc_enc.h:26-28 */
int CSCEnc_Encode_Flush(CSCEncHandle p);                                           /* csc_enc.h:30 */

/* ---- decoder, csc_dec.h ---- */
void CSCDec_ReadProperties(CSCProps *props, uint8_t *stream);                      /* csc_dec.h:8 */
CSCDecHandle CSCDec_Create(const CSCProps *props, ISeqInStream *instream, ISzAlloc *alloc);   /* csc_dec.h:13-15 */
void CSCDec_Destroy(CSCDecHandle p);                                               /* csc_dec.h:17 */
int CSCDec_Decode(CSCDecHandle p, ISeqOutStream *outstream, ICompressProgress *progress);     /* csc_dec.h:19-21 */
/* LIMIT: a single packet coded in more than 32 768 model bits is refused with DECODE_ERROR (earlier runs and blocks delivered,
 * no byte of that run or block).  No encoder writes one, but valid streams that the reference decodes can hold one in two ways:
 *   - an LZ copy longer than 32 768 x 143 bytes: needs raw_blocksize > ~4.5 MiB in the header (the default is 2 MiB);
 *   - an RLE run of a delta block (DT_DLT) whose CODED length exceeds 32 768 x 143: the reference clips a run at the block's
 *     size whatever was coded, so this is reachable at the default geometry, in a block of a few bytes.
 * Parity with the reference is knowingly not reached for these two. */

/* ---- extensions of this library (measurement + device-resident input); not in the reference ---- */
typedef struct {
    uint64_t chunks;              /* CSCEncoder::Compress calls served */
    uint64_t input_bytes;
    uint64_t output_bytes;        /* coder payload bytes (GetCompressedSize, csc_encoder_main.cpp:174) */
    uint64_t encode_launches;     /* k_encode_runs launches */
    double encode_kernel_ms;      /* HIP-event time of those launches, on the stream they ran on */
    double analyze_kernel_ms;     /* k_analyze */
    uint64_t find_match_calls, slide_positions, bt_steps, literals, matches;
} CSCMIStats;

/* Same as one iteration of CSCEnc_Encode's read loop (csc_enc.cpp:170-181), but the <= raw_blocksize
 * chunk is already resident in device memory (bench.py keeps inputs in HBM).  Returns 0 or an error. */
int CSCMI_EncodeDeviceChunk(CSCEncHandle p, const void *device_ptr, size_t size);
/* n independent handles (tasks of a -p / per-extension split) advanced by one chunk each with ONE kernel
 * launch, one workgroup per stream; handles must live on the current device.  sizes[i] == 0 skips handle i. */
int CSCMI_EncodeDeviceChunkBatch(int n, CSCEncHandle *hs, const void *const *device_ptrs, const size_t *sizes);
/* CSCEnc_Encode_Flush (csc_enc.cpp:193-203) for n handles of the current device with one round trip: the EOF kernels queued on one
 * stream, one wait, the last coder blocks handed to the handles' output streams on this thread, in handle order.  Returns 0 or
 * the first error; the streams are byte for byte what n CSCEnc_Encode_Flush calls write. */
int CSCMI_FlushBatch(int n, CSCEncHandle *hs);
/* CSCDec_Decode for n independent handles at once: one kernel launch per round advances every stream (one
 * workgroup each); block reads and Write calls happen on the calling thread, per stream in the order CSCDec_Decode
 * would make them.  rcs[i] = what CSCDec_Decode(hs[i], oss[i], NULL) would return.  Returns 0 or CSCMI_DEVICE_ERROR. */
int CSCMI_DecodeBatch(int n, CSCDecHandle *hs, ISeqOutStream *const *oss, int *rcs);
/* Device-resident decode: n whole streams that lie in device memory, decoded into device memory.  The block reader and the
 * delivery of the decoded runs are inside the kernel: no payload and no run crosses the bus, no callback is made, and a launch
 * does not end at a coder block.  One-shot: per-stream state comes from the decoder's resource cache and goes back to it; any
 * n >= 0, in groups sized to the free device memory; launches go to the library's pooled stream and the call returns when all
 * jobs have their answer.
 *
 * jobs[i].rc and dst[0 .. produced) are exactly what CSCDec_Create + CSCDec_Decode give over an ISeqInStream that serves
 * src[0 .. src_size) with full-size reads and an ISeqOutStream that accepts a Write only while the total stays <= dst_cap and
 * returns a short count otherwise:
 *   rc        0, -1, DECODE_ERROR, READ_ERROR or WRITE_ERROR as CSCDec_Decode returns them; CSCMI_NO_DECODER where CSCDec_Create
 *             would have returned NULL for this stream (illegal props, or the first RC or BC block missing or cut);
 *             CSCMI_DEVICE_ERROR if this job could not get its device memory (the other jobs proceed)
 *   dst       a run that does not fit in dst_cap is not delivered at all and ends the stream with WRITE_ERROR; the LIMIT above
 *             (a packet of more than 32 768 model bits) keeps its DECODE_ERROR; bytes of src behind the end-of-stream signal are
 *             ignored; nothing outside [src, src + src_size) is loaded and nothing outside [dst, dst + dst_cap) is stored
 * Returns 0, or CSCMI_DEVICE_ERROR if the GPU side failed or no device is visible; without a visible device no field of any
 * job is touched.  opts and stats may be NULL; one launch is made per host round, so stats->rounds == stats->launches.
 * Where the two differ, the answer is the REFERENCE's, not this library's CSCDec_Create: for a stream whose first block is a
 * bit-coder block the reference (and this call) takes it from the queue, while CSCDec_Create here always reads on for a second. */
#define CSCMI_NO_DECODER (-92)   /* where CSCDec_Create would have returned NULL for this stream */
typedef struct {
    CSCProps props;          /* in: as CSCDec_ReadProperties gives them (host memory) */
    const void *src;         /* in: device pointer, the stream AFTER its 10 property bytes; any alignment */
    size_t src_size;
    void *dst;               /* in: device pointer, any alignment; must not overlap src */
    size_t dst_cap;
    size_t produced;         /* out: bytes written to dst */
    size_t consumed;         /* out: bytes of src the block reader took (defined when rc == 0) */
    int rc;                  /* out */
} CSCMIDevDecode;
typedef struct { uint64_t launch_bytes; } CSCMIDevDecodeOpts;   /* output per stream after which a launch returns; 0 = the library's default (4 MiB) */
typedef struct { uint64_t launches, rounds; double kernel_ms; } CSCMIDevDecodeStats;   /* kernel launches, host rounds, HIP-event time of the launches */
int CSCMI_DecodeDeviceBatch(int n, CSCMIDevDecode *jobs, const CSCMIDevDecodeOpts *opts, CSCMIDevDecodeStats *stats);
/* CSCMI_DecodeDeviceBatch with a stop position per stream: job i is wanted only the first stop_at[i] raw bytes of, and its
 * decoder stops once they are delivered.  stop_at == NULL, or stop_at[i] == UINT64_MAX, means no stop: rc, produced, consumed and
 * dst of that job are then exactly what CSCMI_DecodeDeviceBatch gives (which is this call with NULL).
 *
 * jobs[i] is the answer of CSCDec_Create + CSCDec_Decode over an ISeqOutStream that wants the first stop_at[i] bytes and answers
 * CSC_WRITE_ABORT (csc_dec.cpp:768-769) once it has them.  Per completed run of `size` bytes: n = min(size, stop_at - produced);
 * if n > dst_cap - produced the stream ends with WRITE_ERROR and nothing of this run is delivered; otherwise n bytes are
 * delivered, and once produced has reached stop_at the stream ends with rc = 0.  So
 *   produced  min(stop_at, the stream's raw size) where rc == 0; with stop_at > dst_cap the call behaves as the plain one
 *   consumed  the bytes the block reader had taken when the stream stopped, <= src_size: informative for a stopped stream (the
 *             reader takes whole coder blocks, ahead of the decoder)
 *   dst       bytes at and behind produced stay untouched, nothing outside [dst, dst + dst_cap) is stored
 * No run is decoded once produced >= stop_at: not the run right behind one that ended exactly at stop_at, not the end-of-stream
 * signal, and with stop_at == 0 no run at all -- the answers of CSCDec_Create still hold then (CSCMI_NO_DECODER for illegal
 * props or a first block that is missing or cut).  Damage of the stream wholly behind the run that reaches stop_at is therefore
 * not seen.  The position holds across launches (opts->launch_bytes): a stopped stream is not launched again.
 * Where this differs from the reference: there `finished_` is set by the writer thread, asynchronously, with up to 8 MiB queued
 * (csa_io.h:300-375), so how far the reference decodes behind the last wanted byte depends on timing; this library's callback
 * path (CSA_Extract / CSA_Test) decodes exactly one run more than is wanted; this call decodes none.
 * Out of scope: stopping INSIDE a run -- filtered runs are inverse-filtered whole, so the granularity of the work saved is one
 * run (at most raw_blocksize, 2 MiB by default); the run that crosses stop_at is decoded whole and delivered clipped. */
int CSCMI_DecodeDeviceBatchStop(int n, CSCMIDevDecode *jobs, const uint64_t *stop_at, const CSCMIDevDecodeOpts *opts,
                                CSCMIDevDecodeStats *stats);
/* Device-resident encode, the mirror image of CSCMI_DecodeDeviceBatch: n whole inputs that lie in device memory, encoded into
 * streams that lie in device memory.  The finished coder blocks are framed into dst by a kernel of their own (k_frame_blocks):
 * no block crosses the bus and no callback is made.  One-shot: per-stream state comes from the encoder's resource caches,
 * initialised exactly as CSCEnc_Create initialises it, and goes back to them; any n >= 0, in groups sized to the free device
 * memory and to 2048 streams; launches go to the library's pooled stream, the call returns when all jobs have their answer, and
 * it is safe from several threads at once.
 *
 * jobs[i].rc and dst[0 .. produced) are exactly what CSCEnc_Create + CSCEnc_Encode + CSCEnc_Encode_Flush write over an
 * ISeqInStream that serves src[0 .. src_size) with full-size reads (chunks of raw_blocksize bytes, the last one ragged) and an
 * ISeqOutStream that accepts a Write only while the total stays <= dst_cap.  The 10 property bytes are the caller's
 * (CSCEnc_WriteProperties), as with the reference; src_size == 0 gives the stream CSCEnc_Encode_Flush alone writes.
 *   rc        0, or WRITE_ERROR where dst_cap is too small; CSCMI_NO_ENCODER where CSCEnc_Create would have returned NULL for
 *             these props; CSCMI_DEVICE_ERROR if this job could not get its device memory or its kernel reported an error
 *             (output arena exhausted, watchdog).  The last two do not stop the other jobs of the call.
 *   dst       the first Write that does not fit ends the stream with WRITE_ERROR: produced is the bytes of all EARLIER Write
 *             calls and nothing after it is written, not even a later flag byte that would fit.  The granularity is
 *             MemIO::WriteBlock's (csc_memio.cpp:83-108): the flag byte, then the 3 size bytes when the block is not exactly
 *             csc_blocksize long, then the payload -- each all or nothing, in the order the blocks were finished.
 *             Nothing outside [src, src + src_size) is loaded, nothing outside [dst, dst + dst_cap) is stored, and the bytes
 *             of dst at and beyond produced are untouched.
 * Returns 0, or CSCMI_DEVICE_ERROR if the GPU side failed or no device is visible; without a visible device no field of any
 * job is touched.  stats may be NULL.  A round is one chunk of every stream that still has one (the last round is the flush of
 * all): stats->rounds is the most chunks any job of a group has, plus one, summed over the groups.  Per round the host reads
 * back ONE status array, 16 bytes {error, rc, produced} per stream of the round, and nothing else: stats->readback_bytes, which
 * counts every device-to-host byte of the call, is at most 16 * n * rounds.  stats->launches counts the encode launches (one per
 * kernel flavour and round), the flush kernels (one per stream) and the framing launches (one per round); stats->kernel_ms is the
 * HIP-event time of exactly those.  The analyzer launches and the device-to-device copies of the chunks are neither counted nor
 * timed. */
#define CSCMI_NO_ENCODER (-91)   /* where CSCEnc_Create would have returned NULL for these props */
typedef struct {
    CSCProps props;          /* in: as CSCEncProps_Init gives them, or custom (host memory) */
    const void *src;         /* in: device pointer to the raw bytes; any alignment */
    size_t src_size;         /* may be 0 */
    void *dst;               /* in: device pointer; receives the stream AFTER its 10 property bytes; any alignment; must not overlap src */
    size_t dst_cap;
    size_t produced;         /* out: bytes written to dst */
    int rc;                  /* out */
} CSCMIDevEncode;
typedef struct { uint64_t launches, rounds, readback_bytes; double kernel_ms; } CSCMIDevEncodeStats;   /* encode, flush and framing launches; host rounds; device-to-host bytes; HIP-event time of those launches */
int CSCMI_EncodeDeviceBatch(int n, CSCMIDevEncode *jobs, CSCMIDevEncodeStats *stats);
/* Host-memory variant used by CSCEnc_Encode itself. */
int CSCMI_EncodeHostChunk(CSCEncHandle p, const void *host_ptr, size_t size);
void CSCMI_GetStats(CSCEncHandle p, CSCMIStats *out);
/* 0 if a usable gfx950-class HIP device is visible, else a negative code (and a message on stderr). */
int CSCMI_DeviceCheck(void);

#ifdef __cplusplus
}
#endif
#endif
