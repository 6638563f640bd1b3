/*
 * csa_mi355x.h -- C ABI of the `.csa` container layer of libcsc_mi355x.so.
 *
 * The reference's archiver (src/archiver) is a command-line program, not a library: its interface
 * is the four operations of `class CSArc` (csarc.cpp:37-70) and their options (ParseArg,
 * csarc.cpp:137-208).  This header gives each of them a C entry point with the same meaning, the
 * same return value and -- for `CSA_Add` -- the same bytes on disk as `csarc a -t1`:
 *
 *   reference                                    here
 *   CSArc::Add      csarc.cpp:472-575            CSA_Add
 *   CSArc::Extract  csarc.cpp:600-650            CSA_Extract
 *   CSArc::Test     csarc.cpp:667-700            CSA_Test
 *   CSArc::List     csarc.cpp:652-665            CSA_List
 *   adler32()       csa_adler32.cpp:63-129       CSA_Adler32 (host), CSAMI_Adler32Device (HIP: k_frag_pieces)
 *   PackIndex / UnpackIndex csa_indexpack.cpp:166-211   inside CSA_Add / the readers; CSA_ReadIndex exposes the raw bytes
 *
 * What runs where: the task streams and the index stream are libcsc streams produced by the HIP
 * encoder behind CSCEnc_* (many task streams advance together, one workgroup per stream); the
 * per-fragment adler32 is a HIP reduction over the chunk that is already in HBM for the encoder;
 * decoding uses the HIP decoder behind CSCDec_*.  Directory scan, task split, block table, index
 * packing and file I/O are host code, as in the reference.  No CPU codec exists in this library.
 */
#ifndef CSA_MI355X_H_
#define CSA_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Options of `csarc` (ParseArg, csarc.cpp:137-208).  CSA_OptionsInit sets the reference defaults. */
typedef struct CSAOptions {
    int level;              /* -m#      1..5, default 2                         csarc.cpp:141,150-156 */
    uint32_t dict_size;     /* -d##[k|m] 32 KiB..1 GiB, default 32000000        csarc.cpp:140,157-168 */
    int recurse;            /* -r                                               csarc.cpp:169-170 */
    int overwrite;          /* -f                                               csarc.cpp:171-172 */
    int verbose;            /* -v (List: report fragments)                      csarc.cpp:173-174 */
    int mt_count;           /* -t#  accepted for parity with the reference and otherwise unused: Add always
                               writes the single-worker (task-id order) layout, Extract/Test decode
                               `device_streams` tasks per kernel launch                                  */
    int split_count;        /* -p##  single-file split, default 1               csarc.cpp:190-191 */
    const char *to_dir;     /* -o dir, default "./"                             csarc.cpp:147,183-189 */
    /* --- not in the reference --- */
    int device_streams;     /* task streams advanced per kernel launch; 0 = as many as fit the HBM budget,
                               at most 1024 (Add) / 256 = one per CU (Extract, Test)                    */
    uint64_t hbm_budget;    /* Add: bytes of HBM the concurrent task encoders may use; 0 = 3/4 of
                               the free device memory                                                */
    uint64_t task_bytes;    /* Add: 0 = the reference's task split (archive identical to csarc's).
                               > 0: tasks are additionally cut so that none exceeds this many bytes
                               (files are split into fragments where needed).  The archive is then NOT
                               the one `csarc a` would write, but it is a valid .csa that `csarc x/t/l`
                               read; it gives the GPU many independent streams on any input.  At most
                               127 fragments per file are produced (the index format's limit).          */
} CSAOptions;

typedef struct CSAStats {
    uint64_t raw_bytes;              /* bytes read from the input files */
    uint64_t archive_bytes;          /* final size of the archive */
    uint64_t index_raw_size;
    uint64_t index_compressed_size;
    uint32_t n_entries;              /* index entries (files and directories) */
    uint32_t n_tasks;
    uint32_t n_blocks;               /* archive blocks of all tasks */
    uint32_t verify_failures;        /* Extract/Test: fragments whose adler32 did not match */
    double seconds_total;
    double seconds_encode;           /* Add: inside the batched encoder calls; Extract/Test: decode wall time */
    uint32_t peak_streams;           /* Add: most task streams in flight at once */
    uint32_t reserved;
    double seconds_io;               /* Add: file reads + uploads + adler32 kernel on the calling thread -- a stream's FIRST chunk; the later
                                        chunks are read by a second thread during the encode calls (round 5) and do not count here */
    double seconds_setup;            /* Add: creating / flushing / destroying the task encoders */
} CSAStats;

typedef struct CSAFrag {             /* FileEntry::Frag, csa_typedef.h:18-24 */
    uint32_t bid;                    /* task (archive-blocks) id */
    uint32_t checksum;               /* adler32, seed 0 */
    uint64_t posblock;               /* offset inside the task's raw stream */
    uint64_t size;
    uint64_t posfile;                /* offset inside the file */
} CSAFrag;

/* One call per index entry in name order (what `csarc l` prints, csarc.cpp:656-663). */
typedef void (*CSAListFn)(void *ctx, const char *name, int64_t esize, int64_t edate, int64_t eattr,
                          int nfrags, const CSAFrag *frags);

void CSA_OptionsInit(CSAOptions *o);

/* Not in the reference: a file that the chosen split_count / task_bytes would cut into more than 127 fragments is refused
 * before anything is written (the index keeps the count in one signed byte, csa_indexpack.cpp:84,105 -- the reference CLI
 * writes such an archive and cannot read it back). */
#define CSA_MAX_FRAGMENTS 127
#define CSA_TOO_MANY_FRAGMENTS (-94)
/* Extract / Test: entries whose stored name is empty or has a `..` component are skipped with a message and make the call
 * return CSA_UNSAFE_NAME (after everything else was processed); the reference would follow them out of to_dir. */
#define CSA_UNSAFE_NAME (-93)

/* `csarc a [opts] arcname filenames...`.  Returns 0; 1 if the archive exists and !overwrite
 * (csarc.cpp:474-483); CSCMI_DEVICE_ERROR / READ_ERROR / WRITE_ERROR style negatives when the
 * encoder or the file system fails (the reference ignores those). */
int CSA_Add(const char *arcname, const char *const *filenames, int nfilenames, const CSAOptions *o, CSAStats *st);

/* Sharded Add -- one process per GPU (the reference's counterpart is compress_mt, csarc.cpp:338-409,
 * whose worker threads each take the next task of the size-sorted list and hand their archive blocks to
 * one writer).  Every rank plans the same tasks from the same file names and makes the same deal (CSAMI_PlanShards: the next
 * task of the cost-sorted list to the least loaded rank -- what csarc.cpp:361-398 does dynamically); rank r encodes its tasks on ITS GPU and returns them as one
 * opaque blob (malloc'ed; release with CSAMI_FreeBlob).  The caller moves the blobs to the writing rank
 * (RCCL over xGMI in csc_amd/sharded.py -- the only exchange on this path) and calls CSAMI_AddShardAssemble
 * there with all of them: the archive is byte for byte the one CSA_Add / `csarc a -t1` writes.
 * Return values as CSA_Add; -1 for blobs that do not match the plan. */
int CSAMI_AddShardEncode(const char *const *filenames, int nfilenames, const CSAOptions *o, int rank, int world,
                         uint8_t **blob, uint64_t *blob_len, CSAStats *st);
void CSAMI_FreeBlob(uint8_t *blob);
/* The deal CSAMI_AddShardEncode uses (host only, no GPU): task i of the plan -> rank_of[i], with the cost estimate it was made from
 * (bytes x a data-kind factor; longest-processing-time-first, deterministic on every rank; CSA_DEAL=mod in the environment: i mod
 * world).  Fills at most `cap` entries; returns the number of tasks, or < 0. */
int CSAMI_PlanShards(const char *const *filenames, int nfilenames, const CSAOptions *o, int world, uint32_t *rank_of, double *cost, uint32_t cap);
int CSAMI_AddShardAssemble(const char *arcname, const char *const *filenames, int nfilenames, const CSAOptions *o,
                           const uint8_t *const *blobs, const uint64_t *blob_lens, int nblobs, CSAStats *st);

/* `csarc x`: 0 ok, 1 bad header (csarc.cpp:602-603), -1 decode error (csarc.cpp:464-468), CSA_UNSAFE_NAME (above).
 * A failed adler32 is reported on stderr like the reference does and counted in st->verify_failures;
 * it does not change the return value (csa_io.h:331-332). */
int CSA_Extract(const char *arcname, const char *const *filenames, int nfilenames, const CSAOptions *o, CSAStats *st);

/* `csarc t`: 0 ok, -1 bad header or decode error (csarc.cpp:669-670,697-700). */
int CSA_Test(const char *arcname, const char *const *filenames, int nfilenames, const CSAOptions *o, CSAStats *st);

/* `csarc l`: 0 ok, -1 bad header (csarc.cpp:654-655). */
int CSA_List(const char *arcname, const char *const *filenames, int nfilenames, CSAListFn fn, void *ctx);

/* The plan CSA_Add would execute for these names and options, without executing it (host only, no GPU): number of task
 * streams and the largest fragment count any file gets.  Returns what CSA_Add would return at that point (0 or
 * CSA_TOO_MANY_FRAGMENTS). */
int CSAMI_PlanInfo(const char *const *filenames, int nfilenames, const CSAOptions *o, uint32_t *n_tasks, uint32_t *max_frags);

/* Index pack / unpack round trip on a raw index buffer, for tests and fuzzing (no GPU involved): parses `buf` with the
 * bounds-checked reader and, if it parses, re-packs it.  Returns the re-packed size (<= cap bytes are copied to out, out
 * may be NULL), -1 if the buffer does not parse (truncated, counts beyond the buffer, negative fragment count),
 * CSA_UNSAFE_NAME if it parses but holds a name Extract would refuse. */
int64_t CSA_IndexRoundTrip(const uint8_t *buf, uint64_t size, uint8_t *out, uint64_t cap);

/* The raw (unpacked) index bytes of an archive, for tools and tests: returns the raw size, or -1.
 * Copies at most cap bytes into buf (buf may be NULL to query the size). */
int64_t CSA_ReadIndex(const char *arcname, uint8_t *buf, uint64_t cap);

/* adler32 of csa_adler32.cpp:63-129 (zlib's, with the running value passed in; the archiver seeds
 * fragments with 0).  Host version, and the HIP reduction over a device buffer. */
uint32_t CSA_Adler32(uint32_t adler, const uint8_t *buf, uint64_t len);
int CSAMI_Adler32Device(uint32_t adler, const void *device_ptr, uint64_t len, uint32_t *out);

/* ---- device-resident archive read: a .csa that lies in device memory to file bytes in device memory; not in the reference ----
 *
 * `csarc x` / `csarc t` (CSArc::Extract csarc.cpp:600-650, CSArc::Test :667-700, decompress_mt :411-470) for an archive the
 * caller already holds in HBM.  No archive block, no decoded run and no file byte crosses the bus: the task streams are decoded
 * where they lie by CSCMI_DecodeDeviceBatch, and what the reference's reader and writer threads do around the decoder is three
 * kernels of this layer per wave of tasks:
 *   k_gather_extents   AsyncArchiveReader (csa_io.h:466-542): a task's archive blocks back to back.  A task whose stream is ONE
 *                      block is decoded in place from the archive and not copied.
 *   k_frag_pieces      AsyncFileWriter (csa_io.h:274-408): each fragment from its task's decoded bytes to its place in dst, and
 *                      adler32's partial sums (csa_adler32.cpp:63-129) in the same pass; without dst (csarc t) the sums alone
 *   k_frag_fold        the sums of a fragment folded and compared with the index's checksum (csa_io.h:331-332,397-399)
 * The host reads back the 24 header bytes, the index, the 10 property bytes of every task and 8 bytes per fragment.
 *
 * The layout of dst, shared by CSAMI_DevicePlan, CSAMI_DeviceRead and CSAMI_PlanDeviceLayout: the selected entries in index order
 * (byte-wise by name, std::map of csa_typedef.h:50), selected by the rule of CSA_List (isselected, csarc.cpp:807-816; no names =
 * all).  An entry's `size` is max(posfile + size) over its fragments, 0 for directories, empty files and files the index gives no
 * fragment; its `offset` is the sum of the earlier entries' sizes, each rounded up to 16; dst_bytes is that sum after the last.
 * The unsafe-name rule of CSA_Extract does NOT apply: no name reaches a file system here, so `..` entries are listed and read.
 *
 * A task (archive-blocks id `bid`) is decoded when a selected fragment of non-zero size lies in it.  Its raw size -- the capacity
 * it is decoded into -- is max(posblock + size) over ALL fragments of the index with that bid, selected or not.  Tasks go largest
 * first (csarc.cpp:430), in waves sized by o->hbm_budget (0 = 3/4 of the free device memory; o == NULL = defaults) and
 * o->device_streams (0 = no limit); a wave's buffers are released before the next one's are taken.
 *
 * Safety contract.  Every extent, fragment and size of the index is validated on the host, in overflow-checked 64-bit arithmetic,
 * before the first launch.  Nothing outside [arc, arc + arc_size) is loaded, not even by an aligned 16-byte window, and nothing
 * outside [dst, dst + dst_bytes) is stored; bytes of dst that no delivered fragment covers (rounding gaps, holes, everything at and
 * behind dst_bytes) stay untouched.  An archive block that passes arc_size is clipped there and ends its task's stream -- the short
 * read AsyncArchiveReader turns into end of file -- so the stream fails in the decoder, not in a kernel.  A fragment is clipped to
 * what its task's decoder produced.  Sizes whose buffers cannot be allocated give CSCMI_DEVICE_ERROR.
 * The archive buffer must stay valid and unchanged from CSAMI_DeviceOpen until CSAMI_DeviceClose; dst must not overlap it. */
typedef struct CSADevArchive CSADevArchive;                 /* opaque */
typedef struct CSADevFile {
    const char *name;        /* owned by the handle, valid until CSAMI_DeviceClose (CSAMI_PlanDeviceLayout: see there) */
    int64_t esize, edate, eattr;   /* as CSA_List reports them */
    uint64_t offset;         /* into dst; a multiple of 16 */
    uint64_t size;           /* max(posfile + size) over the entry's fragments, 0 without any */
    uint32_t nfrags, failed_frags;   /* failed_frags: CSAMI_DeviceRead / CSAMI_DeviceReadStop only, else 0 */
} CSADevFile;
typedef struct CSADevReadStats {
    uint64_t tasks, frags, waves;   /* tasks decoded; their selected fragments of non-zero size; waves */
    uint64_t launches;          /* gather + scatter + fold launches of THIS layer: 3 * waves */
    uint64_t decode_launches;   /* what CSCMI_DecodeDeviceBatch reports, summed over the waves */
    uint64_t readback_bytes;    /* device-to-host bytes of this layer: CSAMI_DeviceOpen's 24 + 10 + index raw size, plus at most
                                   16 * tasks + 8 * frags in this call */
    uint64_t raw_bytes;         /* sum of the sizes of those fragments */
    uint32_t verify_failures; uint32_t reserved;
    double kernel_ms, seconds_total;   /* HIP-event time of this layer's launches (the decoder's is not in it); wall time of the call */
} CSADevReadStats;

/* decompress_index (csarc.cpp:290-336) on the device: check_header (csarc.cpp:577-598) over the 24 header bytes read back; the
 * index stream decoded where it lies (its 10 property bytes read back first); its raw bytes read back and parsed by the
 * bounds-checked UnpackIndex.  Returns 0; 1 for a bad header (as CSA_Extract) or arc_size < 24; -1 for an index that is out of
 * bounds, undecodable or unparsable, or whose sizes wrap in 64 bits; CSCMI_DEVICE_ERROR without a usable device (*out is
 * untouched then) or when memory cannot be had.  *out is set only when 0 is returned. */
int CSAMI_DeviceOpen(const void *arc_dev, uint64_t arc_size, CSADevArchive **out);
/* The layout for a selection, without reading anything (host only): at most `cap` entries are stored to files (files may be NULL),
 * *n_files is the number of selected entries, *dst_bytes the bytes CSAMI_DeviceRead needs.  Returns 0, or -1 if the sum wraps. */
int CSAMI_DevicePlan(CSADevArchive *a, const char *const *names, int nnames,
                     CSADevFile *files, uint32_t cap, uint32_t *n_files, uint64_t *dst_bytes);
/* `csarc x` into dst (dst == NULL: `csarc t`, dst_cap ignored).  files / cap as CSAMI_DevicePlan, with failed_frags filled in.
 * Returns what CSA_Test returns: 0; -1 if any task's stream has no decoder, ends early, fails to decode or holds more than its raw
 * size (a WRITE_ERROR of a task stream is a decode error); CSCMI_DEVICE_ERROR where memory cannot be had; WRITE_ERROR, with
 * nothing launched and *st zeroed, if dst != NULL and dst_cap < dst_bytes.
 * A failed adler32 is counted per file in failed_frags and summed in st->verify_failures and does not change the return value
 * (csa_io.h:331-332).  A fragment is verified only if at least one of its bytes was delivered (posblock < produced of its task) --
 * that is when AsyncFileWriter opens it, and only opened fragments are closed and verified (csa_io.h:390-406); fragments wholly
 * behind the end of a short stream are not counted, the -1 reports them.
 * Where this differs from CSA_Test on a damaged archive: the callback path stops a task's decoder once its last selected fragment
 * is complete (CSC_WRITE_ABORT, csa_io.h:176-179), this call decodes every task to its end, so damage BEHIND the last selected
 * fragment of a task is reported here and not there. */
int CSAMI_DeviceRead(CSADevArchive *a, const char *const *names, int nnames, void *dst, uint64_t dst_cap,
                     const CSAOptions *o, CSADevFile *files, uint32_t cap, CSADevReadStats *st);
/* CSAMI_DeviceRead that costs what it selects: every decoded task stops behind its last selected byte.  Arguments, the layout of
 * dst, files and *st are those of CSAMI_DeviceRead; stop_stats may be NULL.  It differs in four places only:
 *   - a decoded task gets stop = max(posblock + size) over its SELECTED fragments of non-zero size (<= its raw size) and is decoded
 *     by CSCMI_DecodeDeviceBatchStop (csc_mi355x.h) with stop_at = dst_cap = stop: the decoder delivers the run that reaches `stop`
 *     clipped to it and decodes nothing behind it -- the callback path (CSA_Extract / CSA_Test) decodes one run more, the
 *     reference an amount that depends on its writer thread's timing;
 *   - the task's scratch is `stop` bytes (rounded up to 256) instead of its raw size;
 *   - wave sizing reckons the decoded bytes at `stop`; the dictionary term (bounded by the raw size) and the room for a copy of
 *     the coded stream stay as they are;
 *   - the return value: as CSAMI_DeviceRead, except that damage wholly behind the run that reaches a task's `stop` is not seen,
 *     nor a stream that holds more than its raw size -- which is what CSA_Test answers for damage behind the run after that one.
 * Unchanged: a fragment is clipped to what was produced and verified only if a byte of it was delivered; st->launches ==
 * 3 * st->waves; the read-back bound; and the gather: a task stream of more than one archive block is still copied WHOLE, because
 * how many coded bytes a prefix of the raw bytes needs is not known before it is decoded.
 * Out of scope: stopping inside a run (the granularity is one run, at most raw_blocksize = 2 MiB by default), gathering part of a
 * multi-block stream, and the host paths (CSA_Extract / CSA_Test), which stop as they did.  The unit of selection here is the whole
 * entry; byte ranges and strided slices inside an entry are CSAMI_DeviceReadSlices' (below).
 * Without a visible device CSCMI_DEVICE_ERROR is returned and nothing of the caller's is touched. */
typedef struct CSADevStopStats {
    uint64_t decoded_bytes;     /* sum of the decode jobs' `produced`: the sum of the tasks' stops where every stream is intact */
    uint64_t task_raw_bytes;    /* sum of the decoded tasks' raw sizes: the capacities CSAMI_DeviceRead would have decoded into */
    uint64_t scratch_bytes;     /* device bytes taken for decoded bytes: per wave, the sum of its tasks' stops each rounded up to 256 */
    uint64_t stopped_tasks;     /* tasks with stop < raw size */
} CSADevStopStats;
int CSAMI_DeviceReadStop(CSADevArchive *a, const char *const *names, int nnames, void *dst, uint64_t dst_cap,
                         const CSAOptions *o, CSADevFile *files, uint32_t cap, CSADevReadStats *st, CSADevStopStats *stop_stats);
/* HIP-event milliseconds of the last CSAMI_DeviceRead's launches by kernel: [0] k_gather_extents, [1] k_frag_pieces, [2] k_frag_fold
 * (after CSAMI_DeviceCompare: [1] k_frag_compare, [2] k_frag_fold_diff) */
void CSAMI_DeviceKernelMs(const CSADevArchive *a, double ms[3]);
void CSAMI_DeviceClose(CSADevArchive *a);
/* host only, no GPU: the same plan from raw (unpacked) index bytes, as CSA_ReadIndex returns them.  files[i].name points at the
 * entry's name INSIDE raw_index: not NUL-terminated, its 32-bit little-endian length in the four bytes in front of it.
 * task_raw_sizes receives (at most task_cap; may be NULL) the raw sizes of the tasks CSAMI_DeviceRead would decode for this
 * selection, in the order it decodes them (largest sum of selected fragment sizes first, equal sums by bid); *n_tasks their number.
 * This call is the strict one: it returns -1 for an index that does not parse, whose sizes wrap, or with an archive block that
 * does not lie inside [0, arc_size) -- which the device path would read short. */
int CSAMI_PlanDeviceLayout(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                           CSADevFile *files, uint32_t cap, uint32_t *n_files, uint64_t *dst_bytes,
                           uint64_t *task_raw_sizes, uint32_t task_cap, uint32_t *n_tasks);
/* host only, no GPU: the tasks CSAMI_DeviceReadStop would decode for this selection, in the order it decodes them, from raw index
 * bytes and with the strictness of CSAMI_PlanDeviceLayout (-1 for what that call refuses).  bids / stops / raws (each may be NULL)
 * receive at most `cap` entries: the task's archive-blocks id, its stop position and its raw size (stop <= raw); *n_tasks their
 * number.  No task is listed for a selection of directories and empty files only. */
int CSAMI_PlanDeviceStops(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                          uint64_t *bids, uint64_t *stops, uint64_t *raws, uint32_t cap, uint32_t *n_tasks);

/* ---- device-resident archive write: file bytes that lie in device memory to a .csa in device memory; not in the reference ----
 *
 * `csarc a -t1` (CSArc::Add csarc.cpp:472-575, compress_mt :338-409, compress_index :219-288) for entries the caller already holds
 * in HBM: arc[0, archive_bytes) is byte for byte what CSA_Add writes for the same entries and options.  What the reference's
 * reader and writer threads do around the encoder is, per wave of tasks, at most five launches of this layer whatever the number
 * of tasks and fragments:
 *   k_frag_pieces      AsyncFileReader (csa_io.h:215-272): a task's fragments back to back, and adler32's partial sums in the same
 *                      pass.  A task whose input is ONE range of one entry is encoded where it lies: summed, not copied.
 *                      (one launch for the pieces that are copied, one for those that are not)
 *   k_frag_fold        the sums of each fragment folded (csa_io.h:250); the host reads the checksums, 8 bytes a fragment
 *   CSCMI_EncodeDeviceBatch   every task of the wave at once, into scratch of this layer: raw + raw/8 + 64 KiB a stream; a stream
 *                      that does not fit is encoded once more, alone, into 2 raw + 1 MiB (st->retries).  CSA_DEVWRITE_SLACK=<bytes>
 *                      in the environment, read per call, makes the first size raw/4 + <bytes> (for tests of that second try)
 *   k_block_table      AsyncWriter::Write / flush (csa_io.h:145-201): the task's archive-block table, from the sizes of the Write
 *                      calls the encoder would have made -- read off the framing of the stream where it lies
 *   k_gather_extents   the 10 property bytes and the stream of each task to arc, in task-id order (csa_io.h:559-573)
 * and after the last wave the index (PackIndex, csa_indexpack.cpp:166-189) is uploaded, encoded on the device and placed with the
 * 24 header bytes by one more launch: st->launches <= 5 * waves + 2.
 *
 * Input.  `files` is the table CSAMI_DeviceRead fills, so a read can be fed straight back: name, esize, edate and eattr go into the
 * index as given; an entry's bytes are src[offset, offset + esize), offset of any alignment; a name that ends in '/' is a directory
 * and must have esize 0.  size, nfrags and failed_frags are ignored on input; on return (0 only) size = esize and nfrags is the
 * number of fragments the entry got.  The order of the table does not matter: the index is in byte-wise name order
 * (csa_typedef.h:50).  No selection and no unsafe-name rule applies -- nothing reaches a file system.  arcname enters through its
 * length alone (csa_indexpack.cpp:129-134).  Of the options level, dict_size, split_count, task_bytes, device_streams and
 * hbm_budget mean what they mean for CSA_Add and CSAMI_DeviceRead, the others are ignored; o == NULL gives the defaults.
 * The plan is CSA_Add's (the same text, over an index built from the table instead of a directory scan); tasks go in waves of
 * consecutive ids, largest first, sized by hbm_budget and device_streams (at most 2048), a wave's buffers released before the next.
 *
 * Returns 0; CSA_TOO_MANY_FRAGMENTS as CSA_Add, nothing launched and nothing stored; -1 for a table the host refuses before any
 * launch (n_files > 0 with files == NULL, a NULL or duplicate name, esize < 0, a directory with bytes, offset + esize past
 * src_size or wrapping, sizes that sum past 2^60, [src, src + src_size) overlapping [arc, arc + arc_cap)); WRITE_ERROR when the
 * archive does not fit in arc_cap (refused before the launch that would pass it); CSCMI_DEVICE_ERROR without a usable device (no
 * argument touched then), when memory cannot be had, when a task's encode job reports it or fails its second try, or when the
 * block-table walk finds a stream that does not end at its `produced` (an internal inconsistency, never a fault).
 *
 * Safety contract.  Every size is checked on the host, in overflow-checked 64-bit arithmetic, before the first launch.  Nothing
 * outside [src, src + src_size) is loaded, not even by an aligned 16-byte window, and nothing outside [arc, arc + arc_cap) is stored.
 * On success the bytes of arc at and behind archive_bytes are untouched; on failure the bytes inside arc_cap are unspecified.
 *
 * What crosses the bus.  Host to device: the piece tables (24 bytes per <= 16 KiB piece of a fragment, 24 per fragment, 32 per task,
 * 24 per <= 64 KiB piece of a placed stream), 10 property bytes a task, the raw index and the 24 header bytes.  Device to host: the
 * encoder's own 16 bytes a stream a round, 8 bytes a fragment, and per task 8 bytes (block count, status) plus 8 bytes per archive
 * block.  No file byte and no stream byte crosses in either direction. */
typedef struct CSADevWriteStats {
    uint64_t tasks, frags, waves, blocks;     /* task streams; fragments of all entries; waves; archive blocks of all tasks */
    uint64_t launches;                        /* launches of THIS layer (gather/sum, fold, block table, placement) */
    uint64_t encode_launches;                 /* what CSCMI_EncodeDeviceBatch reports, summed (index stream included) */
    uint64_t readback_bytes, upload_bytes;    /* every device-to-host / host-to-device byte of this layer (tables included in upload) */
    uint64_t raw_bytes, archive_bytes, index_raw_size, index_compressed_size;
    uint32_t n_entries, retries;              /* retries: task streams re-encoded because the scratch was too small */
    double kernel_ms, seconds_encode, seconds_total;
} CSADevWriteStats;
/* The plan CSAMI_DeviceWrite would execute (host only, no GPU): number of task streams, the largest fragment count of any entry,
 * the bytes of all tasks.  Returns 0, CSA_TOO_MANY_FRAGMENTS, or -1 for a table refused as above (offsets are not looked at). */
int CSAMI_DeviceWritePlan(const CSADevFile *files, uint32_t n_files, const char *arcname, const CSAOptions *o,
                          uint32_t *n_tasks, uint32_t *max_frags, uint64_t *raw_bytes);
int CSAMI_DeviceWrite(const void *src_dev, uint64_t src_size, CSADevFile *files, uint32_t n_files, const char *arcname,
                      void *arc_dev, uint64_t arc_cap, const CSAOptions *o, CSADevWriteStats *st);
/* HIP-event milliseconds of this thread's last CSAMI_DeviceWrite by kernel: [0] k_frag_pieces (or k_frag_rows), [1] k_frag_fold, [2] k_block_table,
 * [3] k_gather_extents (placement) */
void CSAMI_DeviceWriteKernelMs(double ms[4]);

/* ---- the device-resident archive over the caller's own buffers: write from, read into, compare against; not in the reference ----
 *
 * CSAMI_DeviceWrite and CSAMI_DeviceRead want every entry in ONE buffer -- src plus an offset per entry, dst in a layout the library
 * chooses.  The three calls below take one device pointer per entry instead, so a set of separately allocated buffers (the tensors
 * of a state dict, a batch of shards) is archived where it lies, an archive is read straight into the buffers that are to hold it,
 * and "does this archive hold exactly what these buffers hold?" is answered on the device, byte for byte -- what `tar --compare`
 * answers.  The contiguous calls are these calls with ptrs[i] = src + offset_i / dst + offset_i: there is one write path and one
 * read path, and every sentence of the two sections above that does not speak of src, dst or the layout of dst holds here.
 * Every pointer may have any alignment.  Without a visible device all three return CSCMI_DEVICE_ERROR and touch nothing. */

/* host only, no GPU: the address checks the three calls below make before anything is launched.
 * Range i is [ptrs[i], ptrs[i] + sizes[i]); a range of size 0 overlaps nothing and may be NULL.
 * Returns 0, or -1 with *bad (bad may be NULL) set to the lowest index of a range that is refused: a NULL pointer with size > 0; one
 * whose end wraps in 64 bits (ptr + size == 2^64 does not); one that overlaps [excl, excl + excl_size) (excl_size 0: nothing does);
 * and, with disjoint != 0, one that overlaps another range of the table -- both ranges of such a pair are refused, ranges that touch
 * are not.  ptrs or sizes NULL with n > 0 refuses index 0.  The ranges are sorted, not compared pair by pair: n log n. */
int CSAMI_CheckBuffers(const void *const *ptrs, const uint64_t *sizes, uint32_t n,
                       const void *excl, uint64_t excl_size, int disjoint, uint32_t *bad);

/* CSAMI_DeviceWrite with entry i's bytes at ptrs[i][0, esize_i); files[i].offset is ignored, ptrs[i] is not looked at where esize_i
 * is 0 and may be NULL there.  The plan, the archive bytes (byte for byte what CSA_Add and CSAMI_DeviceWrite write for the same entries
 * and options), the return values, *st, the safety contract -- nothing outside [ptrs[i], ptrs[i] + esize_i) is loaded, not even by an
 * aligned 16-byte window -- the bus contract, CSA_DEVWRITE_SLACK and CSAMI_DeviceWriteKernelMs are CSAMI_DeviceWrite's; a task that
 * is one range of one entry is still encoded where it lies.  The entries are only read, so they may alias each other.  -1 with
 * nothing launched, besides what CSAMI_DeviceWrite refuses in a table: ptrs == NULL with n_files > 0, and whatever
 * CSAMI_CheckBuffers(ptrs, esizes, n_files, arc_dev, arc_cap, 0) refuses -- an entry that overlaps [arc, arc + arc_cap) above all. */
int CSAMI_DeviceWriteFrom(const void *const *ptrs, CSADevFile *files, uint32_t n_files, const char *arcname,
                          void *arc_dev, uint64_t arc_cap, const CSAOptions *o, CSADevWriteStats *st);

#define CSAMI_DEV_STOP_EARLY 1u
/* CSAMI_DeviceRead (flags == 0) or CSAMI_DeviceReadStop (flags & CSAMI_DEV_STOP_EARLY; then *stop_stats is filled, else zeroed;
 * it may be NULL) with entry i of the selection -- in the order CSAMI_DevicePlan lists it -- delivered to ptrs[i][0, size_i), of which
 * caps[i] bytes are the caller's.  n must be that plan's *n_files, else -1; files, if not NULL, has room for n and is filled as by
 * CSAMI_DeviceRead, with offset 0.  ptrs[i] == NULL (or ptrs == NULL: all of them): the entry is verified only, `csarc t` for that
 * entry; it is still selected, so it counts for which tasks are decoded and where they stop.  A wave stays three launches:
 * k_frag_pieces sums a piece without a destination and does not store it.
 * Refused with nothing launched and *st zeroed: WRITE_ERROR for a non-NULL ptrs[i] with caps[i] < size_i; -1 for what
 * CSAMI_CheckBuffers(ptrs, sizes, n, arc, arc_size, 1) refuses -- destinations that overlap each other or the archive.
 * Nothing outside [ptrs[i], ptrs[i] + size_i) is stored, and bytes of it that no delivered fragment covers stay untouched.
 * The return value otherwise, which fragments are verified, failed_frags and st->verify_failures, st->launches == 3 * st->waves,
 * the read-back bound and CSAMI_DeviceKernelMs: as documented at CSAMI_DeviceRead and CSAMI_DeviceReadStop. */
int CSAMI_DeviceReadInto(CSADevArchive *a, const char *const *names, int nnames, void *const *ptrs, const uint64_t *caps, uint32_t n,
                         uint32_t flags, const CSAOptions *o, CSADevFile *files, CSADevReadStats *st, CSADevStopStats *stop_stats);

/* Entry i of the selection against the sizes[i] bytes at ptrs[i]: `csarc t` and a byte-for-byte comparison in the same pass.
 * Arguments as CSAMI_DeviceReadInto; nothing of the caller's is written, so the buffers may alias each other, but not the archive
 * (-1, nothing launched, for what CSAMI_CheckBuffers(ptrs, sizes, n, arc, arc_size, 0) refuses, and for diffs == NULL with n > 0).
 * diffs[i].status == 0: the entry equals the buffer.  Otherwise it is the sum of
 *   CSA_DIFF_SIZE     sizes[i] != size_i; the comparison then covers the offsets below the smaller of the two (the compared size)
 *   CSA_DIFF_BYTES    a compared byte differs; first_diff is the smallest such offset in the entry (UINT64_MAX without this flag):
 *                     the minimum, taken on the host, of posfile + offset over the entry's fragments
 *   CSA_DIFF_SKIPPED  ptrs[i] == NULL: the entry is verified only; no other flag is set then
 *   CSA_DIFF_SHORT    a byte below the compared size belongs to a fragment but was not delivered -- its task failed or ended early --
 *                     so it was not compared
 * Bytes of the entry that no fragment covers are not compared.  failed_frags is the entry's count of failed adler32s, as in files.
 * adler32 is taken over every delivered fragment in the same pass and reported as by CSAMI_DeviceRead with dst == NULL, and the return
 * value is the archive's health, exactly what CSAMI_DeviceReadInto with every pointer NULL returns: differences never change it.
 * Per wave three launches of this layer: k_gather_extents; k_frag_compare -- k_frag_pieces with two loads in the place of a load and
 * a store, its time in slot [1] of CSAMI_DeviceKernelMs; k_frag_fold_diff, which also folds each fragment's first differing offset.
 * Read back: at most 16 bytes a task and 16 bytes a fragment (st->readback_bytes, with CSAMI_DeviceOpen's).
 * Nothing outside [ptrs[i], ptrs[i] + min(sizes[i], size_i)) is loaded, not even by an aligned 16-byte window. */
typedef struct CSADevDiff { uint64_t first_diff; uint32_t status; uint32_t failed_frags; } CSADevDiff;
#define CSA_DIFF_BYTES 1u
#define CSA_DIFF_SIZE 2u
#define CSA_DIFF_SKIPPED 4u
#define CSA_DIFF_SHORT 8u
int CSAMI_DeviceCompare(CSADevArchive *a, const char *const *names, int nnames, const void *const *ptrs, const uint64_t *sizes, uint32_t n,
                        uint32_t flags, const CSAOptions *o, CSADevFile *files, CSADevDiff *diffs, CSADevReadStats *st,
                        CSADevStopStats *stop_stats);

/* ---- byte ranges and strided slices of entries: a read that costs what it selects INSIDE an entry; not in the reference ----
 *
 * Of an entry of `size` bytes (the size CSAMI_DevicePlan lists) a slice selects the bytes [offset + k * stride, offset + k * stride +
 * run) for k < count, and they are delivered packed, row after row, into ptrs[i][0, run * count): a block of rows of a row-major
 * matrix is count == 1 (a byte range; stride is ignored then), a block of columns is one run out of every row.  count == 0 selects
 * nothing: the entry is neither decoded, summed nor verified, and run is ignored.
 * A slice is refused (-1, nothing launched, *st zeroed) for count > 0 with run == 0; count > 1 with stride < run (stride == run is
 * allowed); any product or sum that wraps in 64 bits; a last selected byte at or behind `size` -- a slice lies inside its entry and is
 * not clipped.
 *
 * Which tasks, how far, what is verified.  A fragment is TOUCHED when at least one selected byte lies in [posfile, posfile + size) --
 * decided with one division a fragment, not by walking rows.  A task is decoded when it holds a touched fragment of non-zero size;
 * without CSAMI_DEV_STOP_EARLY to its raw size, with it to stop = max(posblock + size) over its TOUCHED fragments, exactly as
 * CSAMI_DeviceReadStop stops a task (scratch `stop` rounded up to 256, wave sizing at `stop`).  Every touched fragment is summed
 * WHOLE and checked against the index, so no byte is delivered from a fragment whose adler32 was not taken, and a stop never falls
 * inside a touched fragment.  Untouched fragments are neither summed nor verified, even where they lie in front of a stop and are
 * decoded on the way.  st->tasks, st->frags and st->raw_bytes count the decoded tasks and their touched fragments; tasks go largest
 * sum of touched fragment sizes first, equal sums by bid.  The return value, failed_frags, st->verify_failures, the clipping of a
 * fragment to what its task produced, "verified only if a byte of it was delivered", st->launches == 3 * st->waves and the read-back
 * bound: as documented at CSAMI_DeviceReadInto.  Bytes of a destination that no delivered fragment covers stay untouched.
 *
 * A wave is three launches: k_gather_extents, k_frag_slices, k_frag_fold.  The pieces of a fragment stay on its fixed 16 KiB grid.
 * A piece that lies inside one run is stored whole and one without a selected byte is summed only, both as k_frag_pieces does it
 * (slice_stats->plain_pieces); any other piece (periodic_pieces) is summed whole and stored in part: every source byte loaded once,
 * a 16-byte unit inside one run stored as 16 bytes, a unit across a run border byte by byte.  Its table entry holds 32-bit
 * quantities whatever run and stride are.  Nothing outside a fragment's decoded bytes is loaded, not even by an aligned 16-byte
 * window, and nothing but the selected bytes' destinations is stored.
 * Out of scope: stopping inside a fragment, a slice of an entry into a slice of a buffer in one call, updating a slice in place (an
 * update that writes a new archive and copies the unchanged tasks' streams is CSAMI_DeviceUpdate), and the host paths (CSA_Extract /
 * CSA_Test). */
typedef struct CSADevSlice { uint64_t offset, run, stride, count; } CSADevSlice;
typedef struct CSADevSliceStats {
    uint64_t selected_bytes;    /* sum of run * count over the entries */
    uint64_t touched_bytes;     /* sum of the touched fragments' sizes: what is summed where every task delivers its bytes */
    uint64_t periodic_pieces;   /* pieces summed whole and stored in part */
    uint64_t plain_pieces;      /* pieces stored whole or summed only */
} CSADevSliceStats;
/* Arguments as CSAMI_DeviceReadInto, with slices[i] for entry i of the selection in CSAMI_DevicePlan's order.  n must be that plan's
 * *n_files, and slices == NULL with n > 0 is refused: -1.  ptrs[i] == NULL (or ptrs == NULL: all of them): the touched fragments are
 * verified only.  WRITE_ERROR for a non-NULL ptrs[i] with caps[i] < run * count; -1 for what CSAMI_CheckBuffers(ptrs, run * count, n,
 * arc, arc_size, 1) refuses; all refusals with nothing launched and *st, *stop_stats and *slice_stats (each may be NULL) zeroed.
 * files[i].size is the entry's size, not the slice's.  CSAMI_DeviceKernelMs: [1] is k_frag_slices.  Without a visible device
 * CSCMI_DEVICE_ERROR is returned and nothing of the caller's is touched; that refusal comes before the handle is looked at. */
int CSAMI_DeviceReadSlices(CSADevArchive *a, const char *const *names, int nnames, const CSADevSlice *slices, void *const *ptrs,
                           const uint64_t *caps, uint32_t n, uint32_t flags, const CSAOptions *o, CSADevFile *files, CSADevReadStats *st,
                           CSADevStopStats *stop_stats, CSADevSliceStats *slice_stats);
/* host only, no GPU: the tasks CSAMI_DeviceReadSlices decodes for this selection and these slices (n of them, one per selected entry,
 * else -1), in the order it decodes them, with the strictness and the outputs of CSAMI_PlanDeviceStops: stops[i] is the task's stop
 * under CSAMI_DEV_STOP_EARLY.  *n_touched (may be NULL) is the number of touched fragments.  -1 also for what the read refuses in a
 * slice. */
int CSAMI_PlanDeviceSlices(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                           const CSADevSlice *slices, uint32_t n, uint64_t *bids, uint64_t *stops, uint64_t *raws, uint32_t cap,
                           uint32_t *n_tasks, uint32_t *n_touched);

/* ---- entries gathered from strided slices of the caller's buffers: a write that takes its bytes where they lie; not in the reference ----
 *
 * CSAMI_DeviceWriteFrom wants every entry as one contiguous range.  Here entry i's bytes are the bytes that slices[i] -- a
 * CSADevSlice exactly as CSAMI_DeviceReadSlices defines it: offset, run, stride, count; with count == 1 the stride is ignored --
 * selects out of the caller's buffer ptrs[i][0, sizes[i]), packed row after row: a rank that holds a full row-major matrix archives
 * its block of columns, one run out of every row, without a contiguous copy of it.  The archive is byte for byte what CSA_Add and
 * CSAMI_DeviceWriteFrom write for the packed bytes and the same options; the plan depends on sizes alone, so CSAMI_DeviceWritePlan
 * serves unchanged.  There is one write path: CSAMI_DeviceWriteFrom is this call with slices[i] = {0, esize_i, esize_i, 1} and
 * sizes[i] = esize_i.
 *
 * Refused with -1, nothing launched and *st and *gather_stats (each may be NULL) zeroed: everything CSAMI_DeviceWriteFrom refuses in
 * a table; slices == NULL or sizes == NULL with n_files > 0; a slice that the read refuses in an entry of sizes[i] bytes (run == 0
 * with count > 0, stride < run with count > 1, any product or sum that wraps, a last selected byte at or behind sizes[i]);
 * files[i].esize != run * count -- so count == 0 goes with esize == 0 and with nothing else, and ptrs[i] may be NULL there; a NULL
 * ptrs[i] with count > 0; and whatever CSAMI_CheckBuffers refuses over the HULLS [ptrs[i] + offset, + (count - 1) * stride + run)
 * against [arc, arc + arc_cap) with disjoint == 0.  Hulls may alias each other.  The other return values are CSAMI_DeviceWriteFrom's:
 * WRITE_ERROR for an archive that does not fit, CSA_TOO_MANY_FRAGMENTS, and CSCMI_DEVICE_ERROR without a visible device -- decided
 * before any argument is looked at, with nothing touched.
 *
 * Where a task is encoded.  A task that is one non-empty range of one entry, and whose range lies inside ONE RUN of that entry's
 * slice, is encoded where it lies (gather_stats->inplace_tasks); every other task with a byte in it is gathered into scratch of this
 * layer (gathered_tasks) -- decided with one division a range, not by walking rows.  The pieces of a fragment lie on the fixed
 * 16 KiB grid of the PACKED fragment.  A wave stays at most five launches of this layer, st->launches <= 5 * st->waves + 2: in a
 * wave with at least one piece gathered across a run border (periodic_pieces) the stored pieces, those of one contiguous source
 * included, go through k_frag_rows with one table of 56 bytes a piece; a wave without one runs k_frag_pieces over 24-byte pieces
 * exactly as CSAMI_DeviceWriteFrom always did.  st->upload_bytes counts whatever table was sent, and slot [0] of
 * CSAMI_DeviceWriteKernelMs holds the gather's time either way.  A periodic piece's table entry holds 32-bit quantities whatever
 * the run is; the stride is an address step and stays 64-bit.  A 16-byte unit of it whose packed bytes lie inside one run is two
 * aligned 16-byte loads funnel-shifted into one aligned 16-byte store; a unit across a run border is assembled byte by byte.  With
 * run < 16 every unit crosses a border: that is the slow path (profiles/archive_device_write_slices.md has its measured rate), and
 * no rate is promised for it.
 *
 * Safety contract.  Nothing outside an entry's hull is loaded, not even by an aligned 16-byte window.  Gap bytes inside the hull may
 * be loaded; they are never summed and never stored.  Nothing of the caller's is written.  The bus contract is CSAMI_DeviceWrite's,
 * with 56 bytes in the place of 24 for a stored piece of a wave that runs k_frag_rows: no file byte and no stream byte crosses.
 * Out of scope: updating an existing archive in place (CSAMI_DeviceUpdate writes a new one and reuses the streams of the unchanged
 * tasks), and the host paths (CSA_Add).  The way back -- a read into, and a comparison
 * against, a slice of a buffer -- is the next section. */
typedef struct CSADevGatherStats {
    uint64_t selected_bytes;    /* sum of run * count: the entries' bytes */
    uint64_t hull_bytes;        /* sum of the slices' hulls: (count - 1) * stride + run */
    uint64_t periodic_pieces;   /* pieces gathered across a run border */
    uint64_t plain_pieces;      /* pieces whose source is one contiguous range: gathered so, or summed where they lie */
    uint64_t gathered_tasks, inplace_tasks;   /* tasks with a byte in them: gathered into scratch / encoded where they lie */
} CSADevGatherStats;
int CSAMI_DeviceWriteSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices,
                            CSADevFile *files, uint32_t n_files, const char *arcname,
                            void *arc_dev, uint64_t arc_cap, const CSAOptions *o,
                            CSADevWriteStats *st, CSADevGatherStats *gather_stats);

/* ---- read into and compare against strided slices of the caller's buffers: the way back of CSAMI_DeviceWriteSlices; not in the reference ----
 *
 * CSAMI_DeviceReadInto and CSAMI_DeviceCompare want contiguous bytes on the caller's side.  Here the caller's side of entry i -- in the
 * order CSAMI_DevicePlan lists the entries -- is what slices[i], a CSADevSlice exactly as CSAMI_DeviceWriteSlices reads it, selects of
 * the caller's buffer ptrs[i][0, sizes[i]): packed byte p of the entry lives at buffer offset offset + (p / run) * stride + p % run;
 * with count == 1 the stride is ignored.  It is a slice of the BUFFER, not of the entry.  So a block of columns written from
 * t[:, c0:c1] is restored into, or verified against, t[:, c0:c1] where it lies, without a packed scratch copy and a second pass, and
 * eight ranks' column blocks are read into one full matrix by ONE call, through eight slices whose hulls interleave.  There is one
 * read path: CSAMI_DeviceReadInto is CSAMI_DeviceReadIntoSlices with slices[i] = {0, size_i, size_i, 1} and sizes[i] = caps[i], and
 * CSAMI_DeviceCompare is CSAMI_DeviceCompareSlices with slices[i] = {0, sizes[i], sizes[i], 1}.
 *
 * Reading.  Every sentence documented at CSAMI_DeviceReadInto and CSAMI_DeviceReadStop that does not speak of caps or of the
 * destination's shape holds: which tasks are decoded and how far (CSAMI_DEV_STOP_EARLY), that every selected fragment is summed
 * whole and verified, the return value, the clipping of a fragment to what its task produced, failed_frags, st->launches ==
 * 3 * st->waves and the read-back bound.  ptrs[i] == NULL (or ptrs == NULL: all of them): the entry is verified only and its slice
 * is not looked at.  run * count > size_i is allowed: the entry fills the first size_i packed positions and the rest is untouched.
 * run * count < size_i with a non-NULL pointer: WRITE_ERROR, nothing launched.  Gap bytes are never stored to, nor are bytes of
 * the hull behind packed position size_i, bytes that no delivered fragment covers, or anything outside the hull.
 * Refused with -1, nothing launched and *st, *stop_stats and *spread_stats (each may be NULL) zeroed: slices == NULL or sizes == NULL
 * with n > 0; n other than the plan's *n_files; for a non-NULL ptrs[i], a slice that the read refuses in an entry of sizes[i] bytes
 * (run == 0 with count > 0, stride < run with count > 1, any product or sum that wraps, a last selected byte at or behind sizes[i]);
 * and whatever CSAMI_CheckSlices(ptrs, sizes, slices, n, arc, arc_size, 1) refuses.  Without a visible device CSCMI_DEVICE_ERROR is
 * returned before any argument is looked at, with nothing touched.
 *
 * Comparing.  CSAMI_DeviceCompareSlices is CSAMI_DeviceCompare with entry i compared against the packed bytes of slices[i]:
 * CSA_DIFF_SIZE is set when run * count != size_i, and the compared size is then the smaller of the two; first_diff is a packed offset
 * in the entry; gap bytes are never compared and nothing of the caller's is written.  Hulls may alias each other, not the archive:
 * the check is CSAMI_CheckSlices with disjoint == 0.
 *
 * Kernels.  A fragment's pieces stay on the fixed 16 KiB grid of the decoded (packed) fragment, and a piece is planned as
 * CSAMI_DeviceWriteSlices plans it, with the roles of source and destination exchanged.  A wave stays three launches.  In a wave
 * with at least one piece whose side in the buffer crosses a run border (spread_stats->periodic_pieces) all pieces go through
 * k_frag_spread (k_frag_compare_rows when comparing) with one table of 56 bytes a piece; a wave without one runs k_frag_pieces
 * (k_frag_compare) over 24-byte pieces exactly as CSAMI_DeviceReadInto (CSAMI_DeviceCompare) always did.  Slot [1] of
 * CSAMI_DeviceKernelMs holds the time either way.  Every byte of the fragment is loaded once, in aligned 16-byte units, and summed as
 * k_frag_pieces sums it.  A unit whose 16 packed bytes fall in one run is stored as 16 bytes -- one store, four or sixteen, as the
 * destination's alignment allows -- or compared with two aligned 16-byte loads of the caller's, funnel-shifted, whose window is
 * checked against the hull: gap bytes may be loaded by the comparison; they are never compared.  A unit across a run border goes
 * byte by byte.  With run < 16 every unit crosses a border: that is the slow path (profiles/archive_device_spread.md), and no
 * rate is promised for it.  Nothing outside a hull is loaded or stored, not even by an aligned 16-byte window.
 * Out of scope: a slice of an entry into a slice of a buffer in one call, updating an archive in place (CSAMI_DeviceUpdate writes a
 * new archive beside the old one), and the host paths. */
typedef struct CSADevSpreadStats {
    uint64_t selected_bytes;    /* sum over the entries of the bytes delivered / compared: min(size_i, run * count) */
    uint64_t hull_bytes;        /* sum of the slices' hulls: (count - 1) * stride + run */
    uint64_t periodic_pieces;   /* pieces spread (or compared) across a run border */
    uint64_t plain_pieces;      /* pieces whose buffer side is one contiguous range, or that are summed only */
} CSADevSpreadStats;
/* host only, no GPU: CSAMI_CheckBuffers over slices.  It refuses what CSAMI_CheckBuffers refuses, about each HULL
 * [ptrs[i] + offset, + (count - 1) * stride + run) -- a hull that overlaps [excl, excl + excl_size) is refused even where only a gap
 * byte overlaps, as the write refuses it -- and a slice that the read refuses in a buffer of sizes[i] bytes; count == 0 selects
 * nothing and its pointer may be NULL.  *bad as there; ptrs, sizes or slices NULL with n > 0 refuses index 0.
 * With disjoint != 0 two hulls that overlap are accepted only where their SELECTED bytes provably do not meet, decided without
 * walking rows: both slices have the same stride S (a count == 1 slice takes the other's; two count == 1 slices that overlap are
 * refused), d = (address of B's period position 0 - address of A's) mod S, and d >= run_A and d + run_B <= S -- column blocks of one
 * matrix, a byte range inside one gap.  Any other overlapping pair refuses both indices.  The hulls are sorted by their start and
 * swept: n log n plus the number of overlapping pairs.  With disjoint == 0 nothing is checked between entries. */
int CSAMI_CheckSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, uint32_t n,
                      const void *excl, uint64_t excl_size, int disjoint, uint32_t *bad);
int CSAMI_DeviceReadIntoSlices(CSADevArchive *a, const char *const *names, int nnames, void *const *ptrs, const uint64_t *sizes,
                               const CSADevSlice *slices, uint32_t n, uint32_t flags, const CSAOptions *o, CSADevFile *files,
                               CSADevReadStats *st, CSADevStopStats *stop_stats, CSADevSpreadStats *spread_stats);
int CSAMI_DeviceCompareSlices(CSADevArchive *a, const char *const *names, int nnames, const void *const *ptrs, const uint64_t *sizes,
                              const CSADevSlice *slices, uint32_t n, uint32_t flags, const CSAOptions *o, CSADevFile *files,
                              CSADevDiff *diffs, CSADevReadStats *st, CSADevStopStats *stop_stats, CSADevSpreadStats *spread_stats);

/* ---- update: CSAMI_DeviceWriteSlices that copies the streams of unchanged tasks out of an archive already in HBM; not in the reference ----
 *
 * A state dict is written again and again, and most of its bytes are last time's.  A task stream is a pure function of the task's
 * bytes, `level` and the properties CSCEncProps_Init(min(dict_size, total), level) gives, and the plan depends on names and sizes
 * alone.  So where a task of the new plan has the composition and the bytes of a task of `base` -- a handle from CSAMI_DeviceOpen --
 * the stream in the base archive IS the stream the encoder would write, and it is copied, not encoded.
 *
 * Contract.  arc[0, archive_bytes) is byte for byte what CSAMI_DeviceWriteSlices writes for the same arguments whenever the reused
 * streams were written at the same `level` by this library or the reference.  The 10 property bytes do not record the level: that
 * the base was written at this call's level is the CALLER's to ensure.  Otherwise arc is a valid `.csa` that holds those streams.
 * Nothing of the caller's and nothing of the base is written; nothing outside a hull or the base buffer is loaded.
 *
 * Arguments are CSAMI_DeviceWriteSlices's and mean the same, refusals and return values included.  slices == NULL && sizes == NULL
 * means every entry whole, as CSAMI_DeviceWriteFrom builds it (only one of them NULL: -1).  base == NULL makes the call exactly
 * CSAMI_DeviceWriteSlices -- that call IS this one with base == NULL, so there is one write path.  Refused with -1, nothing launched
 * and all three statistics zeroed, besides what the write refuses: [arc, arc + arc_cap) overlapping the base's archive buffer.
 * Without a visible device CSCMI_DEVICE_ERROR is returned before any argument is looked at.
 *
 * Candidates (host; CSAMI_PlanDeviceUpdate is exactly this step over raw index bytes, as strict as CSAMI_PlanDeviceLayout).  A task
 * of the new plan is a candidate for base task b when its total is above zero and the set of its fragments (name, offset in the
 * entry, size, posblock), zero-size fragments included, equals the set of ALL fragments of the base index with bid b.  An entry
 * of that base task missing from the table, one more entry, another size or another split make the sets differ: CSA_UPD_NEW.
 * edate and eattr do not enter.  Found through one map from (name, offset) to the base's fragments, not by comparing tasks pairwise.
 * A candidate whose 10 property bytes in the base (read back, 10 bytes a candidate, in st->readback_bytes) are not what
 * CSCEnc_WriteProperties(CSCEncProps_Init(min(dict_size, total), level)) writes is CSA_UPD_PROPS.
 *
 * Check, default (verify).  The remaining candidates' base streams are decoded and compared with the caller's bytes by the machinery
 * of CSAMI_DeviceCompareSlices, in waves sized as CSAMI_DeviceRead sizes them; no task that is not a candidate is decoded.  A task
 * is reused when its stream decodes with rc 0, produces exactly the task's total, is consumed to its last byte and no compared
 * byte differs; else it is CSA_UPD_BASE_BAD or CSA_UPD_CHANGED.  A reused fragment's checksum in the new index is the sum taken in
 * this pass, not the base index's: a wrong checksum in the base neither blocks reuse nor survives it.
 *
 * Check, CSAMI_UPDATE_TRUST_SUMS.  Nothing is decoded.  Each candidate's fragments are summed where they lie in the caller's buffers
 * (k_frag_pieces, or k_frag_rows without a destination where a piece crosses a run border) and folded against the base index's
 * checksums; reused means every fragment's adler32 equals the base's.  THIS IS THE FORMAT'S OWN 32-BIT TEST AND NO MORE: two
 * contents of equal size and equal adler32 are taken for equal -- the archive then holds the OLD bytes under the new table -- and
 * the base's stream is trusted to be intact.  A candidate found CHANGED that is encoded where it lies keeps the checksums of this
 * pass and is not summed again.
 *
 * A check wave is three launches in either mode, update_stats->check_launches == 3 * check_waves: k_gather_extents (the property
 * bytes; in verify also the streams of more than one archive block), the compare kernel or the sum pass, and the fold.
 *
 * Write.  The waves run over consecutive ids as in the write; a reused task costs nothing in the budget and one slot of the width,
 * and skips gather and encode.  Its base extents, the property bytes in front, are placed by the wave's one k_gather_extents launch
 * together with the encoded streams, and its archive-block table is NOT the base index's: it comes from k_block_table over the
 * placed stream, so it is the canonical one whatever cut the base into blocks.  st->launches <= 5 * st->waves + 2 holds.  If that
 * walk finds a reused stream that does not end at its length the call returns -1 (in verify: unreachable for an intact decoder).
 * gather_stats and st->retries count encoded tasks only; st->tasks, frags, blocks, raw_bytes and archive_bytes mean what they mean
 * for the write.  tasks[i], i < min(task_cap, st->tasks), says what became of task i of the new plan.
 * Updating in place (arc inside the base buffer) is CSAMI_DeviceUpdateInPlace's.  Out of scope: reusing part of a task, and the host paths. */
#define CSAMI_UPDATE_TRUST_SUMS 1u
typedef struct CSADevUpdateTask { uint64_t base_bid; uint32_t status; uint32_t reserved; } CSADevUpdateTask;   /* per task of the NEW plan, in id order */
/* status */
#define CSA_UPD_REUSED   0u   /* the base archive's stream was copied; base_bid says which */
#define CSA_UPD_NEW      1u   /* no task of the base has this composition (base_bid = UINT64_MAX) */
#define CSA_UPD_PROPS    2u   /* same composition, other 10 property bytes under these options */
#define CSA_UPD_CHANGED  3u   /* same composition, a byte (or, with TRUST_SUMS, a sum) differs */
#define CSA_UPD_BASE_BAD 4u   /* verify only: the base task's stream has no decoder, fails, ends early, holds more than its raw size,
                                 or its decoder did not consume it to its last byte */
typedef struct CSADevUpdateStats {
    uint64_t candidates, reused_tasks, encoded_tasks;   /* candidates: what the host step found, before the property bytes */
    uint64_t reused_raw_bytes, reused_stream_bytes, encoded_raw_bytes;   /* stream bytes: as placed, property bytes included */
    uint64_t checked_bytes;      /* bytes of the caller's summed (TRUST_SUMS) or compared (verify) in the check phase */
    uint64_t decoded_bytes;      /* verify: sum of `produced` of the base decodes; 0 with TRUST_SUMS */
    uint64_t check_waves, check_launches, decode_launches;
    double check_kernel_ms, seconds_check;
} CSADevUpdateStats;
int CSAMI_DeviceUpdate(CSADevArchive *base, const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices,
                       CSADevFile *files, uint32_t n_files, const char *arcname, void *arc_dev, uint64_t arc_cap,
                       uint32_t flags, const CSAOptions *o, CSADevWriteStats *st, CSADevGatherStats *gather_stats,
                       CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap);
/* host only, no GPU: the candidate step.  base_bids[i], i < min(cap, *n_tasks): the base bid task i of the plan of `files` under o
 * is a candidate for, or UINT64_MAX.  -1 for an index CSAMI_PlanDeviceLayout refuses and a table CSAMI_DeviceWritePlan refuses;
 * CSA_TOO_MANY_FRAGMENTS as there. */
int CSAMI_PlanDeviceUpdate(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const CSADevFile *files, uint32_t n_files,
                           const CSAOptions *o, uint64_t *base_bids, uint32_t cap, uint32_t *n_tasks, uint32_t *n_candidates);

/* ---- fragment digests: a strong hash beside adler32, so that an update can trust and not decode; not in the reference ----
 *
 * CSAMI_UPDATE_TRUST_SUMS rests on the format's own 32-bit sum, and the `.csa` has to stay byte for byte `csarc a -t1`'s, so a
 * stronger hash cannot go into the archive.  It goes into a side table in HBM: one 32-byte digest per fragment of the index, in
 * INDEX ORDER -- the entries in byte-wise name order, the fragments of an entry as CSA_List reports them (offset order), zero-size
 * fragments included.  Every write and update can produce the table; the next update consumes it in the place of a decode.
 *
 * The digest of a fragment of n bytes is BLAKE2s-256 in tree mode, unkeyed, no salt, no personalisation: fan-out 0, maximal depth
 * 2, leaf length 16384, inner length 32, digest length 32.  L = max(1, ceil(n / 16384)) leaves; leaf i is the fragment's packed
 * bytes [16384 i, min(n, 16384 (i + 1))), hashed with node offset i, node depth 0 and the last-node flag on leaf L - 1 only; the root
 * is hashed over the L leaf digests, node offset 0, node depth 1, last-node flag set.  A fragment of size 0 is one empty leaf.
 * Python: hashlib.blake2s(leaf, digest_size=32, fanout=0, depth=2, leaf_size=16384, inner_size=32, node_offset=i, node_depth=0,
 * last_node=(i == L - 1)), and the same call over the leaf digests with node_depth=1, node_offset=0, last_node=True
 * (csc_amd.csa.fragment_digest).  The leaf grid is the 16 KiB grid of the piece tables.
 *
 * Kernels (csa_dev_digest.h, csa_dev_kernels.hip).  k_digest_leaves: one lane per leaf -- a leaf is a serial chain of up to 256
 * compressions, so the parallelism is across leaves -- over a table of 40 bytes a leaf.  A source is contiguous bytes at any
 * alignment, or the runs of a periodic slice, digested straight from the runs (no packed copy is made); nothing outside the
 * fragment's bytes is loaded, not even by an aligned window, and no gap byte.  k_digest_roots: one lane per fragment over its
 * leaves' digests; it stores the digest to the table and, where an expected table is given, compares the 32 bytes on the device.
 * One word a fragment is read back; no digest byte crosses the bus in either direction.  Both tables may have any alignment.
 * A call digests all its fragments in one leaf launch and one root launch, whatever the number of waves: ds->launches, never
 * st->launches -- every existing statistic is what it is without the tables.
 *
 * What CSAMI_UPDATE_TRUST_DIGESTS still trusts: that the base's streams are intact, as under CSAMI_UPDATE_TRUST_SUMS -- the table
 * speaks about the bytes the streams were made from, not about the streams; CSAMI_DeviceReadDigests checks them once -- and that
 * the base was written at this call's level. */
typedef struct CSADevDigest { uint8_t b[32]; } CSADevDigest;
typedef struct CSADevDigestStats {
    uint64_t frags, leaves, digested_bytes;   /* what the digest kernels ran over */
    uint64_t launches;                        /* theirs: two a pass */
    uint64_t mismatches;                      /* compared fragments whose digest differs from the expected table's */
    uint64_t first_mismatch;                  /* the lowest index, in the table this call writes (or would write), of such a fragment; UINT64_MAX: none */
    double kernel_ms;
} CSADevDigestStats;
#define CSAMI_UPDATE_TRUST_DIGESTS 2u
/* host only, no GPU: the fragments, and so the table entries, that a write of this table makes.  Refusals: CSAMI_DeviceWritePlan's. */
int CSAMI_DeviceWriteFragCount(const CSADevFile *files, uint32_t n_files, const char *arcname, const CSAOptions *o, uint64_t *n_frags);
/* The table a write of these entries would produce, with nothing written and nothing encoded.  Arguments and refusals are
 * CSAMI_DeviceWriteSlices's minus the archive (sizes == slices == NULL: every entry whole); -1 also where digests_out overlaps a
 * hull or is NULL with fragments to digest; digests_cap (entries) < the fragment count: WRITE_ERROR with nothing launched. */
int CSAMI_DeviceDigestSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, const CSADevFile *files,
                             uint32_t n_files, const char *arcname, const CSAOptions *o, CSADevDigest *digests_out, uint64_t digests_cap,
                             CSADevDigestStats *ds);
/* CSAMI_DeviceUpdate with the tables: CSAMI_DeviceUpdate IS this call with both tables NULL, so there stays one write path; with
 * base == NULL it is CSAMI_DeviceWriteSlices that also hands out the table.
 * digests_out (may be NULL; digests_cap entries): the table of the archive this call writes, always computed in this call from the
 * caller's bytes, never copied from the base table.  The archive bytes and every statistic of st, gather_stats and update_stats
 * are exactly what the call without it gives.
 * base_digests (may be NULL; n_base_digests entries): the table of `base`, as the call that wrote the base or
 * CSAMI_DeviceReadDigests handed it out.
 * CSAMI_UPDATE_TRUST_DIGESTS: nothing is decoded.  Each candidate's fragments are digested where they lie and compared on the device
 * with base_digests at the base fragments' index positions; reused means every fragment's digest is equal, else the task is
 * CSA_UPD_CHANGED.  The check waves are CSAMI_UPDATE_TRUST_SUMS's (the property bytes, the sum pass, the fold: the new index's
 * checksums of reused fragments are still sums taken in this call, not the base's), except that the base index's checksums decide
 * nothing.  ds->mismatches counts the candidates' fragments whose digest differs.
 * Refused with -1, nothing launched and all statistics zeroed, besides what CSAMI_DeviceUpdate refuses: both trust flags;
 * TRUST_DIGESTS with base_digests == NULL; base and base_digests given and n_base_digests other than the base index's fragment
 * count; either table overlapping arc, the base buffer, a caller's hull or the other table.  digests_cap < the plan's fragment
 * count returns WRITE_ERROR before any launch. */
int CSAMI_DeviceUpdateDigests(CSADevArchive *base, const CSADevDigest *base_digests, uint64_t n_base_digests,
                              const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices,
                              CSADevFile *files, uint32_t n_files, const char *arcname, void *arc_dev, uint64_t arc_cap,
                              uint32_t flags, const CSAOptions *o, CSADevWriteStats *st, CSADevGatherStats *gather_stats,
                              CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap,
                              CSADevDigest *digests_out, uint64_t digests_cap, CSADevDigestStats *ds);
/* `csarc t` of the whole archive (no selection) that also writes the table of the decoded fragments: how an archive that comes from
 * disk enters the chain, and how a base's streams are checked once.  It is CSAMI_DeviceRead with dst == NULL, wave for wave, with a
 * digest pass over each wave's delivered fragments (and one over the zero-size fragments, which no task holds); a fragment none
 * of whose bytes was delivered is neither digested nor compared, as it is not summed.  digests_out may be NULL (compare only).
 * expect (may be NULL): a table of the archive's fragment count; every digested fragment is compared with it, mismatches are counted
 * in ds, and for the return value, st->verify_failures and the entry's failed fragments a mismatch counts exactly as a failed
 * checksum of that fragment does (a fragment that fails both counts once).  -1 with nothing launched: a NULL, a table overlapping
 * the archive or the other table; digests_cap < the archive's fragment count: WRITE_ERROR with nothing launched. */
int CSAMI_DeviceReadDigests(CSADevArchive *a, const CSAOptions *o, CSADevDigest *digests_out, uint64_t digests_cap,
                            const CSADevDigest *expect, CSADevReadStats *st, CSADevDigestStats *ds);
/* HIP-event milliseconds of this thread's last digesting call by kernel: [0] k_digest_leaves, [1] k_digest_roots; ds->kernel_ms is their sum */
void CSAMI_DeviceDigestKernelMs(double ms[2]);

/* ---- the update in place: the new archive takes the base's place in the caller's buffer ----
 * CSAMI_DeviceUpdateDigests without a second buffer: `base` was opened at the first byte of a buffer of buf_cap bytes (buf_cap >= the
 * base's size), and on return 0 buf[0, st->archive_bytes) is byte for byte what CSAMI_DeviceUpdateDigests writes into a separate
 * buffer for the same arguments.  Every other argument means what it means there -- flags, refusals and the three check modes
 * (verify, CSAMI_UPDATE_TRUST_SUMS, CSAMI_UPDATE_TRUST_DIGESTS) included --, with [base's first byte, + buf_cap) in the place of
 * both the base buffer and arc: no hull and neither digest table may meet it.  -1 also for base == NULL and buf_cap < the base's size.
 * tasks[], update_stats, gather_stats, ds and digests_out are that call's; st is that call's except for launches, waves,
 * kernel_ms, upload_bytes, readback_bytes and the times.  st->launches <= 5 * st->waves + 2 + ceil(reused tasks / 2048): a wave
 * with a task to encode is at most three launches of gather, sums and fold, one k_block_table and one k_gather_extents that
 * compacts its streams into held memory; the reused streams are one k_gather_extents (only where a base stream lies in more than
 * one extent) and one k_block_table per 2048 of them; the final placement is one k_gather_extents.  The moves are ms->launches, at
 * most three.
 * On success the handle describes the new archive exactly as CSAMI_DeviceOpen(buf, st->archive_bytes) would: the next read or
 * update on it needs no reopen.
 * EVERY REFUSAL COMES BEFORE THE FIRST STORE INTO THE BUFFER: bad arguments, a failed plan, -1 for a reused stream whose
 * block-table walk does not end at its length, and WRITE_ERROR where header, streams and index do not fit buf_cap.  After any of
 * these the buffer is byte for byte the base and the handle still describes it.  The order that gives this: the check waves and
 * the encode waves only read the base, and the encoded streams are held in scratch (ms->held_stream_bytes at its peak) until every
 * size is known; then the reused streams move inside the buffer (k_move_extents) and the rest is placed.
 * ONCE THE FIRST MOVE HAS BEEN LAUNCHED ONLY CSCMI_DEVICE_ERROR CAN COME BACK, AND THEN THE BUFFER IS LOST: it holds neither the
 * base nor the new archive, and the handle must be closed. */
typedef struct CSADevMoveStats {
    uint64_t moves, moved_bytes;              /* after dropping src == dst and coalescing neighbours of one shift */
    uint64_t parked_moves, parked_bytes;      /* of those: copied to scratch before the left phase, placed from there at the end */
    uint64_t held_stream_bytes;               /* encoded streams kept in scratch until placement, at its peak */
    uint64_t launches;                        /* this layer's: park, left, right */
    double kernel_ms;
} CSADevMoveStats;
int CSAMI_DeviceUpdateInPlace(CSADevArchive *base, uint64_t buf_cap,
                              const CSADevDigest *base_digests, uint64_t n_base_digests,
                              const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices,
                              CSADevFile *files, uint32_t n_files, const char *arcname,
                              uint32_t flags, const CSAOptions *o, CSADevWriteStats *st, CSADevGatherStats *gather_stats,
                              CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap,
                              CSADevDigest *digests_out, uint64_t digests_cap, CSADevDigestStats *ds, CSADevMoveStats *ms);
/* HIP-event milliseconds of this thread's last CSAMI_DeviceUpdateInPlace by launch: [0] the park copy, [1] k_move_extents' left
 * phase, [2] its right phase; ms->kernel_ms is their sum */
void CSAMI_DeviceMoveKernelMs(double ms[3]);

/* YYYYMMDDHHMMSS <-> time_t, csa_common.cpp:3-39 */
int64_t CSA_DecimalTime(int64_t unix_seconds);
int64_t CSA_UnixTime(int64_t decimal_date);

#ifdef __cplusplus
}
#endif
#endif /* CSA_MI355X_H_ */
