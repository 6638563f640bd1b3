// csc_host.cpp -- host side of libcsc_mi355x.so: the reference's C API (csc_enc.h) served by
// the gfx950 kernels of csc_kernels.hip.
//
// What stays on the host (SURVEY.md section 3.1 puts the device boundary inside
// CSCEncoder::Compress): the user callbacks (always on the calling thread), the 2 MiB read loop
// (csc_enc.cpp:160-191) and the RC/BC block framing (csc_memio.cpp:83-108).  Everything that
// touches the data -- analyzer, run segmentation over its per-block verdicts, filters, match
// finder, parser, model, range/bit coder -- runs in HIP kernels on state that lives in HBM.
// There is NO CPU fallback: without a HIP device CSCEnc_Create fails loudly and returns NULL.
#include <hip/hip_runtime.h>
#include <chrono>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/csc_mi355x.h"
#include "csc_device.h"
#include "csc_enc_frame.h"
#include "csc_tables.h"

namespace cscmi {
hipError_t upload_tables();
void launch_frame_blocks(const FrameItem *items, FrameJob *jobs, FrameStatus *status, uint32_t nstreams, hipStream_t st);   // csc_enc_frame.hip
void launch_init_state(EncState *S, hipStream_t st);
void launch_analyze(EncState *S, uint32_t chunk_size, const double *ent_coef, hipStream_t st);
void launch_encode_runs(int parser, EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena, hipStream_t st);
void launch_encode_eof(EncState *S, hipStream_t st);
void launch_encode_runs_multi(int parser, uint32_t nstreams, EncState *const *states, const RunDesc *const *runs,
                              const uint32_t *nruns, const uint32_t *reset, hipStream_t st);
#ifdef CSCMI_STAGE_TEST
void launch_stage_filter(EncState *S, uint32_t kind, uint32_t size, uint32_t chn, uint32_t *result, hipStream_t st);
#endif
hipStream_t pooled_stream(int device);
void pooled_stream_release(int device, hipStream_t s);
}  // namespace cscmi

using namespace cscmi;

namespace {

constexpr uint32_t kMagicEnc = 0x43534345;           // "CSCE"

void *def_alloc(void *, size_t n) { return malloc(n); }   // csc_default_alloc.cpp:5-17
void def_free(void *, void *a) { free(a); }
ISzAlloc g_default_alloc = {def_alloc, def_free};

#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t err__ = (call);                                                                \
        if (err__ != hipSuccess) {                                                                \
            fprintf(stderr, "csc-mi355x: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(err__), \
                    __FILE__, __LINE__);                                                          \
            return CSCMI_DEVICE_ERROR;                                                            \
        }                                                                                         \
    } while (0)

// Filters::MakeWordTree, csc_filters.cpp:87-111: node numbering follows insertion order
void build_trie(uint16_t *next, uint8_t *sym)
{
    memset(next, 0, sizeof(uint16_t) * 300 * 26);
    memset(sym, 0, 300);
    uint32_t nodes = 1;
    uint8_t code = 0x82;
    for (int w = 0; w < 122; w++) {
        uint32_t pos = 0;
        for (const char *p = kWords[w]; *p; p++) {
            uint32_t idx = (uint32_t)(*p - 'a');
            if (next[pos * 26 + idx]) pos = next[pos * 26 + idx];
            else { next[pos * 26 + idx] = (uint16_t)nodes; pos = nodes; nodes++; }
        }
        sym[pos] = code++;
    }
}


// Per-handle resources that do not depend on the stream's content are recycled: creating a handle
// costs a pinned allocation, a stream and four events otherwise, and an archive job creates one handle
// per task (hundreds).  HostRes = pinned staging slab + HIP stream + events, keyed by (device, size);
// DevSlab = the ONE device allocation all of a handle's HBM state is carved from, keyed by
// (device, size) and zero-filled again on every reuse (the reference's determinism condition).
struct HostRes {
    int device;
    size_t hsize;
    uint8_t *hslab;
    uint8_t *h_in;              // lazily allocated: only CSCEnc_Encode / CSCMI_EncodeHostChunk stage input on the host
    hipStream_t stream;
    hipEvent_t ev[2];           // created on first use (host_events): a handle that is only ever driven through a batch launch records none
    hipEvent_t ev_an[2];
    bool have_events;
};
struct DevSlab { int device; size_t size; void *p; };

std::mutex g_cache_mu;
std::vector<HostRes *> g_host_cache;
std::vector<DevSlab> g_dev_cache;
size_t g_dev_cache_bytes = 0;
constexpr size_t kHostCacheMax = 4096;            // entries (256 B pinned each; coder blocks are read back through the calling thread's buffer, thread_pinned)
constexpr size_t kDevCacheMaxBytes = 48ull << 30;

}  // namespace

// Streams are shared: creating one costs ~4 ms on this runtime (tools/gpu_setup_probe.py), an archive job has thousands of handles
// alive at once, and a handle's own stream only carries its set-up, its single-handle calls and its EOF -- batch calls run on the
// lead handle's stream.  Up to kStreamPool non-blocking streams per device, handed out least-used first, created when every
// existing one has a user, never destroyed.  Handles that share a stream stay correct (every call waits for its own work; it may
// wait for a neighbour's too): a host that drives more than kStreamPool handles from threads of its own loses overlap, not bytes.
namespace cscmi {
namespace {
constexpr int kStreamPool = 16;
struct StreamPool { hipStream_t s[kStreamPool]; uint32_t users[kStreamPool]; int n; };
StreamPool g_streams[64];
std::mutex g_streams_mu;
}
hipStream_t pooled_stream(int device)
{
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(g_streams_mu);
    StreamPool &p = g_streams[device];
    int best = -1;
    for (int i = 0; i < p.n; i++) if (best < 0 || p.users[i] < p.users[best]) best = i;
    if ((best < 0 || p.users[best] > 0) && p.n < kStreamPool) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess) { best = p.n++; p.s[best] = st; p.users[best] = 0; }
        else (void)hipGetLastError();
    }
    if (best < 0) return nullptr;
    p.users[best]++;
    return p.s[best];
}
void pooled_stream_release(int device, hipStream_t s)
{
    if (device < 0 || device >= 64 || !s) return;
    std::lock_guard<std::mutex> lk(g_streams_mu);
    StreamPool &p = g_streams[device];
    for (int i = 0; i < p.n; i++) if (p.s[i] == s) { if (p.users[i]) p.users[i]--; return; }
}
}  // namespace cscmi

namespace {

void host_res_destroy(HostRes *r)
{
    if (!r) return;
    if (r->hslab) (void)hipHostFree(r->hslab);
    if (r->h_in) (void)hipHostFree(r->h_in);
    for (auto &e : r->ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : r->ev_an) if (e) (void)hipEventDestroy(e);
    if (r->stream) pooled_stream_release(r->device, r->stream);
    delete r;
}

HostRes *host_res_get(int device, size_t hsize)
{
    HostRes *r = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (size_t i = 0; i < g_host_cache.size(); i++)
            if (g_host_cache[i]->device == device && g_host_cache[i]->hsize == hsize) {
                r = g_host_cache[i];
                g_host_cache.erase(g_host_cache.begin() + i);
                break;
            }
    }
    bool ok = true;
    if (!r) {
        r = new HostRes();
        memset(r, 0, sizeof(*r));
        r->device = device; r->hsize = hsize;
        ok = hipHostMalloc((void **)&r->hslab, hsize, hipHostMallocDefault) == hipSuccess;
    }
    r->stream = ok ? pooled_stream(device) : nullptr;      // (a recycled entry holds none while it sits in the cache)
    if (!ok || !r->stream) { host_res_destroy(r); return nullptr; }
    return r;
}

hipError_t host_events(HostRes *r)
{
    if (r->have_events) return hipSuccess;
    for (auto &e : r->ev) if (!e) { hipError_t err = hipEventCreate(&e); if (err != hipSuccess) return err; }
    for (auto &e : r->ev_an) if (!e) { hipError_t err = hipEventCreate(&e); if (err != hipSuccess) return err; }
    r->have_events = true;
    return hipSuccess;
}

void host_res_put(HostRes *r)
{
    if (!r) return;
    pooled_stream_release(r->device, r->stream);
    r->stream = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        if (g_host_cache.size() < kHostCacheMax) { g_host_cache.push_back(r); return; }
    }
    host_res_destroy(r);
}

void dev_cache_trim()
{
    std::vector<DevSlab> drop;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        drop.swap(g_dev_cache);
        g_dev_cache_bytes = 0;
    }
    for (DevSlab &d : drop) (void)hipFree(d.p);
}

void *dev_slab_get(int device, size_t size)
{
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (size_t i = 0; i < g_dev_cache.size(); i++)
            if (g_dev_cache[i].device == device && g_dev_cache[i].size == size) {
                void *p = g_dev_cache[i].p;
                g_dev_cache.erase(g_dev_cache.begin() + i);
                g_dev_cache_bytes -= size;
                return p;
            }
    }
    void *p = nullptr;
    if (hipMalloc(&p, size) == hipSuccess) return p;
    (void)hipGetLastError();
    dev_cache_trim();                              // give the cached slabs back and try once more
    if (hipMalloc(&p, size) == hipSuccess) return p;
    return nullptr;
}

void dev_slab_put(int device, size_t size, void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        if (g_dev_cache_bytes + size <= kDevCacheMaxBytes) {
            g_dev_cache.push_back(DevSlab{device, size, p});
            g_dev_cache_bytes += size;
            return;
        }
    }
    (void)hipFree(p);
}

// per device, once: the constant tables of the kernels + the two tables built on the host -- the word trie of the dictionary filter
// (next: u16[7800], sym: u8[300]) and log2(diffNum-2)-0.6 for diffNum 6..15 (csc_analyzer.cpp:223).  Never freed.
struct DevTables { uint8_t *trie; double *coef; bool ready; };
DevTables g_dev_tables[64];
std::mutex g_dev_tables_mu;
hipError_t device_tables(int device, DevTables &out)
{
    if (device < 0 || device >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_dev_tables_mu);
    DevTables &t = g_dev_tables[device];
    if (!t.ready) {
        hipError_t err = upload_tables();
        if (err != hipSuccess) return err;
        std::vector<uint8_t> trie(300 * 26 * 2 + 320, 0);
        build_trie((uint16_t *)trie.data(), trie.data() + 300 * 26 * 2);
        double coef[16] = {0};
        for (int d = 6; d < 16; d++) coef[d - 6] = log((double)d - 2) / log((double)2) - 0.6;
        uint8_t *p = nullptr;
        const size_t trie_bytes = (trie.size() + 255) & ~(size_t)255;
        if ((err = hipMalloc((void **)&p, trie_bytes + sizeof(coef))) != hipSuccess) return err;
        if ((err = hipMemcpy(p, trie.data(), trie.size(), hipMemcpyHostToDevice)) != hipSuccess
            || (err = hipMemcpy(p + trie_bytes, coef, sizeof(coef), hipMemcpyHostToDevice)) != hipSuccess) { (void)hipFree(p); return err; }
        t.trie = p; t.coef = (double *)(p + trie_bytes); t.ready = true;
    }
    out = t;
    return hipSuccess;
}

struct EncInstance {
    uint32_t magic;
    ISzAlloc *alloc;
    ISeqOutStream *os;
    CSCProps props;
    int device;
    hipStream_t stream;
    EncState *d_state;
    EncState h;                 // host mirror of the configuration + device pointers
    double *d_entcoef;
    uint8_t *d_trie;            // next (u16[7800]) + sym (u8[300])
#ifdef CSCMI_STAGE_TEST
    uint32_t *d_result;         // CSCST_Filter's result word
#endif
    void *dslab;                // everything above and in `h` is carved from this one allocation
    size_t dsize;
    HostRes *res;               // stream, events and the pinned slab the pointers below point into
    // pinned staging
    uint8_t *h_in;
    uint32_t *h_small;
    hipEvent_t *ev;             // res->ev
    hipEvent_t *ev_an;          // res->ev_an
    // accounting
    int64_t outsize;            // GetCompressedSize, csc_encoder_main.cpp:174
    CSCMIStats stats;
    int parser;
};
// Per-thread resources, recycled through process-wide free lists: a thread that ends hands them back (its thread_local holder's
// destructor makes no HIP call -- it may run while the runtime shuts down), the next thread that needs one takes it over.  So
// short-lived worker threads do not accumulate pinned memory, streams or device tables.
//  * PinBuf: the pinned buffer coder blocks are read back through -- one handle's (drain_arena: a chunk's blocks, or the few bytes
//    of an EOF) and a batch's (drain_batch).  Grown on demand to what is actually read (power of two, >= 256 KiB), so a
//    CSCEnc_Encode_Flush pins no arena-sized buffer and a handle pins none at all.
//  * BatchArgs: argument arrays of the multi-stream launch ([4 * kMaxBatch] pointer-sized words: states, run lists, run counts,
//    reset flags), one set per calling thread and device, + the {bytes, error} pair of every stream of a batch.
struct PinBuf { uint8_t *p = nullptr; size_t cap = 0; };
struct BatchArgs {
    int device = -1; void **d = nullptr; void **h = nullptr;
    uint32_t *small = nullptr;
};
std::mutex g_thread_res_mu;
std::vector<PinBuf> g_pin_free;
std::vector<BatchArgs> g_batch_free;
struct ThreadRes {
    PinBuf pin;
    BatchArgs batch;
    ~ThreadRes()
    {
        std::lock_guard<std::mutex> lk(g_thread_res_mu);
        if (pin.p) g_pin_free.push_back(pin);
        if (batch.d) g_batch_free.push_back(batch);
    }
};
thread_local ThreadRes t_res;
#define t_batch (t_res.batch)
constexpr int kMaxBatch = 2048;
constexpr size_t kBatchPool = 64ull << 20;       // most a batch reads back per wait, unless one stream's arena alone is larger (tiny csc_blocksize: arena_bytes)
constexpr size_t kPinMin = 256 * 1024;

// the calling thread's pinned read-back buffer, at least `need` bytes (nullptr: allocation failed)
uint8_t *thread_pinned(size_t need)
{
    PinBuf &b = t_res.pin;
    if (b.cap >= need) return b.p;
    PinBuf take;
    {
        std::lock_guard<std::mutex> lk(g_thread_res_mu);
        if (b.p) { g_pin_free.push_back(b); b = PinBuf(); }
        size_t best = g_pin_free.size();
        for (size_t i = 0; i < g_pin_free.size(); i++)
            if (g_pin_free[i].cap >= need && (best == g_pin_free.size() || g_pin_free[i].cap < g_pin_free[best].cap)) best = i;
        if (best < g_pin_free.size()) { take = g_pin_free[best]; g_pin_free.erase(g_pin_free.begin() + best); }
        else if (g_pin_free.size() > 8) {        // nothing fits and the list is long: give the smallest back to the system
            size_t sm = 0;
            for (size_t i = 1; i < g_pin_free.size(); i++) if (g_pin_free[i].cap < g_pin_free[sm].cap) sm = i;
            (void)hipHostFree(g_pin_free[sm].p);
            g_pin_free.erase(g_pin_free.begin() + sm);
        }
    }
    if (!take.p) {
        size_t cap = kPinMin;
        while (cap < need) cap <<= 1;
        if (hipHostMalloc((void **)&take.p, cap, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        take.cap = cap;
    }
    b = take;
    return b.p;
}

void free_device(EncInstance *e)
{
    (void)hipSetDevice(e->device);
    if (e->res) (void)hipStreamSynchronize(e->res->stream);
    dev_slab_put(e->device, e->dsize, e->dslab);
    host_res_put(e->res);
    e->dslab = nullptr; e->res = nullptr; e->stream = nullptr;
}

// MemIO::WriteBlock, csc_memio.cpp:83-108: flag byte, [3-byte BE size], payload -- 2-3 Write calls
int write_block(EncInstance *e, const uint8_t *buf, uint32_t size, uint32_t rc1bc0)
{
    uint8_t fb = (uint8_t)(rc1bc0 << 7);
    if (size == e->props.csc_blocksize) fb |= (1 << 6);
    if (e->os->Write(e->os, &fb, 1) != 1) return -1;
    if (size != e->props.csc_blocksize) {
        uint8_t sb[3] = {(uint8_t)(size >> 16), (uint8_t)(size >> 8), (uint8_t)size};
        if (e->os->Write(e->os, sb, 3) != 3) return -1;
    }
    if (size && e->os->Write(e->os, buf, size) != size) return -1;
    return 0;
}

// hand the coder blocks of one chunk (a host copy of the stream's arena) to the user's stream, in the order they were finished
int write_arena(EncInstance *e, const uint8_t *h_arena, uint32_t used)
{
    for (uint32_t off = 0; off < used;) {
        const ArenaRec *rec = (const ArenaRec *)(h_arena + off);
        e->outsize += rec->size;
        e->stats.output_bytes += rec->size;
        if (write_block(e, h_arena + off + 16, rec->size, rec->kind) < 0) return WRITE_ERROR;
        off += 16 + ((rec->size + 15) & ~15u);
    }
    return 0;
}

// Bytes of output arena a chunk can need.  A chunk of raw_blocksize bytes is budgeted B = 3 * raw_blocksize + 1 MiB of coded bytes, as
// it always was.  emit_block (csc_kernels.hip) stores them as records of 16 + round16(size) bytes: full blocks of size == bsize while
// a coder buffer fills -- at most B / bsize of them, each 16 + pad bytes over its payload, pad = round16(bsize) - bsize -- and the two
// blocks of Coder::Flush, of any size up to bsize, each at most 16 + 15 bytes over its payload.  So
//     cap = B + (B / bsize) * (16 + pad) + 2 * 31
// which is B + 1.8 KiB at the default 64 KiB blocks and 32 B at bsize 1.  With raw_blocksize and bsize below 16 MiB (CSCEnc_Create
// refuses the rest) this stays below 2^31, inside the device's 32-bit arena offsets.
uint32_t arena_bytes(uint32_t raw_blocksize, uint32_t bsize)
{
    const uint64_t B = 3ull * raw_blocksize + kMB;
    const uint64_t pad = ((bsize + 15u) & ~15u) - bsize;
    return (uint32_t)(B + B / bsize * (16 + pad) + 2 * 31);
}

int report_device_error(uint32_t err)
{
    // anything else is the watchdog of a many-wavefront form (d4_spin, bt_spin, hp_spin; ERR_QUEUE_STALL): the value says which wait gave up
    fprintf(stderr, "csc-mi355x: device encoder error 0x%x (%s)\n", err,
            err == ERR_ARENA_FULL ? "output arena exhausted" : err == ERR_BAD_TYPE ? "bad block type" : "parse wavefronts lost step");
    return CSCMI_DEVICE_ERROR;
}

// read the finished coder blocks of this chunk back and hand them to the user's stream
int drain_arena(EncInstance *e, bool timed)
{
    HIPCHK(hipMemcpyAsync(e->h_small, &e->d_state->arena_used, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (timed && hipEventElapsedTime(&ms, e->ev[0], e->ev[1]) == hipSuccess) e->stats.encode_kernel_ms += ms;
    uint32_t used = e->h_small[0], err = e->h_small[1];
    if (err != ERR_NONE) return report_device_error(err);
    uint8_t *pin = nullptr;
    if (used) {
        pin = thread_pinned(used);
        if (!pin) { fprintf(stderr, "csc-mi355x: pinned read-back buffer of %u bytes failed\n", used); return CSCMI_DEVICE_ERROR; }
        HIPCHK(hipMemcpyAsync(pin, e->h.arena, used, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return write_arena(e, pin, used);
}

// CSCEncoder::Compress, csc_encoder_main.cpp:85-147, with the data work on the device: chunk_begin uploads the chunk and
// launches the analyzer (no wait), then ONE encode launch per chunk.  The chunk's blocks are walked by the encode kernel itself
// (seg_next, csc_kernels_blocks.inc): typing, duplicate-block checks and run formation need no host round trip.
int chunk_begin(EncInstance *e, const void *src, size_t size, bool on_device, hipStream_t st = nullptr)
{
    if (size == 0 || size > e->props.raw_blocksize) return -1;
    HIPCHK(hipSetDevice(e->device));
    const bool timed = st == nullptr;                // (a batch queues every stream's analyzer on the lead's stream: not timed one by one)
    if (!st) st = e->stream;
    HIPCHK(hipMemcpyAsync(e->h.inbuf, src, size, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if ((e->props.DLTFilter + e->props.EXEFilter + e->props.TXTFilter) != 0) {   // csc_encoder_main.cpp:27-31
        if (timed) HIPCHK(hipEventRecord(e->ev_an[0], st));
        launch_analyze(e->d_state, (uint32_t)size, e->d_entcoef, st);
        HIPCHK(hipGetLastError());
        if (timed) HIPCHK(hipEventRecord(e->ev_an[1], st));
    }
    return 0;
}

int encode_chunk(EncInstance *e, const void *src, size_t size, bool on_device)
{
    if (size == 0) return 0;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(host_events(e->res));
    int rc = chunk_begin(e, src, size, on_device);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[0], e->stream));
    launch_encode_runs(e->parser, e->d_state, nullptr, kSelfSegment | (uint32_t)size, 1u, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], e->stream));
    e->stats.encode_launches++;
    e->stats.chunks++;
    e->stats.input_bytes += size;
    rc = drain_arena(e, true);
    float ms = 0;
    if ((e->props.DLTFilter + e->props.EXEFilter + e->props.TXTFilter) != 0 && hipEventElapsedTime(&ms, e->ev_an[0], e->ev_an[1]) == hipSuccess)
        e->stats.analyze_kernel_ms += ms;
    return rc;
}

// the calling thread's launch tables + read-back pool, on `device`
int batch_args_ready(int device)
{
    if (t_batch.device == device) return 0;
    {
        std::lock_guard<std::mutex> lk(g_thread_res_mu);
        if (t_batch.d) { g_batch_free.push_back(t_batch); t_batch = BatchArgs(); }
        for (size_t i = 0; i < g_batch_free.size(); i++)
            if (g_batch_free[i].device == device) { t_batch = g_batch_free[i]; g_batch_free.erase(g_batch_free.begin() + i); return 0; }
    }
    BatchArgs b;
    auto fail = [&](hipError_t err) {
        fprintf(stderr, "csc-mi355x: batch tables: %s\n", hipGetErrorString(err));
        if (b.d) (void)hipFree(b.d);
        if (b.h) (void)hipHostFree(b.h);
        if (b.small) (void)hipHostFree(b.small);
        return CSCMI_DEVICE_ERROR;
    };
    hipError_t err;
    if ((err = hipMalloc((void **)&b.d, sizeof(void *) * 4 * kMaxBatch)) != hipSuccess) return fail(err);
    if ((err = hipHostMalloc((void **)&b.h, sizeof(void *) * 4 * kMaxBatch, hipHostMallocDefault)) != hipSuccess) return fail(err);
    if ((err = hipHostMalloc((void **)&b.small, sizeof(uint32_t) * 2 * kMaxBatch, hipHostMallocDefault)) != hipSuccess) return fail(err);
    b.device = device;
    t_batch = b;
    return 0;
}

// Read the coder blocks of hs[i] (every i with skip == nullptr || skip[i] != 0) back and hand them to the users' streams, in handle
// order: the {bytes, error} pairs of all streams with one wait, then the arenas packed into the thread's pinned pool, one wait per
// pool-full.  All copies on `st`, the stream the kernels that filled the arenas were launched on.
int drain_batch(int n, CSCEncHandle *hs, const size_t *skip, hipStream_t st)
{
    uint32_t *sm = t_batch.small;
    for (int i = 0; i < n; i++) {
        if (skip && !skip[i]) continue;
        EncInstance *e = (EncInstance *)hs[i];
        HIPCHK(hipMemcpyAsync(sm + 2 * i, &e->d_state->arena_used, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    int rc = 0;
    for (int i = 0; i < n; i++) {
        if (skip && !skip[i]) continue;
        if (sm[2 * i + 1] != ERR_NONE) rc = report_device_error(sm[2 * i + 1]);
    }
    if (rc) return rc;
    // the pool: what this batch reads back (a round's worth at most), not a fixed 64 MiB -- a CSCMI_FlushBatch needs a few KiB
    size_t want = 0, biggest = 0;
    for (int i = 0; i < n; i++) {
        if (skip && !skip[i]) continue;
        const size_t used = sm[2 * i];
        want += (used + 255) & ~(size_t)255;
        if (used > biggest) biggest = used;
    }
    if (want > kBatchPool) want = kBatchPool;
    if (want < biggest) want = biggest;
    if (!want) return 0;
    uint8_t *pool = thread_pinned(want);
    if (!pool) { fprintf(stderr, "csc-mi355x: pinned read-back pool of %zu bytes failed\n", want); return CSCMI_DEVICE_ERROR; }
    const size_t pool_cap = t_res.pin.cap;
    std::vector<size_t> at((size_t)n, 0);
    for (int i = 0; i < n;) {
        size_t off = 0;
        int j = i;
        for (; j < n; j++) {
            if (skip && !skip[j]) continue;
            const size_t used = sm[2 * j];
            if (off + used > pool_cap) break;
            at[j] = off;
            if (used) HIPCHK(hipMemcpyAsync(pool + off, ((EncInstance *)hs[j])->h.arena, used, hipMemcpyDeviceToHost, st));
            off += (used + 255) & ~(size_t)255;
        }
        HIPCHK(hipStreamSynchronize(st));
        for (int k = i; k < j; k++) {
            if (skip && !skip[k]) continue;
            int r = write_arena((EncInstance *)hs[k], pool + at[k], sm[2 * k]);
            if (r && !rc) rc = r;
        }
        i = j;
    }
    return rc;
}

}  // namespace

// =============================================================================================
extern "C" {

int CSCMI_DeviceCheck(void)
{
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess || n <= 0) {
        fprintf(stderr, "csc-mi355x: no HIP device visible (%s); this library has no CPU fallback\n",
                err == hipSuccess ? "device count 0" : hipGetErrorString(err));
        return CSCMI_DEVICE_ERROR;
    }
    return 0;
}

// CSCEncProps_Init, csc_enc.cpp:16-97 (pure host arithmetic; the 10 KiB head-room, the hash-bit
// classes and the per-level overrides are part of the format's de-facto contract)
void CSCEncProps_Init(CSCProps *p, uint32_t dict_size, int level)
{
    dict_size += 10 * kKB;
    if (dict_size < 32 * kKB) dict_size = 32 * kKB;
    if (dict_size > 1024 * kMB) dict_size = 1024 * kMB;
    p->dict_size = dict_size;
    level = level < 1 ? 1 : (level > 5 ? 5 : level);
    p->DLTFilter = p->TXTFilter = p->EXEFilter = 1;
    p->csc_blocksize = 64 * kKB;
    p->raw_blocksize = 2 * kMB;
    uint32_t hbits = dict_size < kMB ? 19 : dict_size <= 4 * kMB ? 20 : dict_size <= 16 * kMB ? 21
                   : dict_size <= 64 * kMB ? 22 : dict_size <= 256 * kMB ? 23 : 24;
    while (((uint32_t)1 << hbits) > dict_size) hbits--;
    if (dict_size <= 16 * kMB) p->bt_size = dict_size;
    else if (dict_size <= 64 * kMB) p->bt_size = (dict_size - 16 * kMB) / 2 + 16 * kMB;
    else if (dict_size <= 256 * kMB) p->bt_size = (dict_size - 64 * kMB) / 4 + 40 * kMB;
    else p->bt_size = (dict_size - 256 * kMB) / 8 + 88 * kMB;
    p->good_len = 32;
    p->hash_bits = (uint8_t)hbits;
    p->bt_hash_bits = (uint8_t)(hbits + 1);
    struct { uint8_t width, mode, good; int dbits; } lv[5] = {
        {1, 2, 32, +1}, {8, 2, 24, -1}, {2, 3, 16, +1}, {8, 3, 24, -1}, {0, 3, 48, 0}};
    const auto &L = lv[level - 1];
    p->hash_width = L.width; p->lz_mode = L.mode; p->good_len = L.good;
    p->hash_bits = (uint8_t)(p->hash_bits + L.dbits);
    if (level < 5) p->bt_size = 0;          // levels 1-4 leave bt_cyc as the caller had it (:57-84)
    else p->bt_cyc = 32;
    if (p->bt_size == p->dict_size) p->hash_width = 0;
}

void CSCEnc_WriteProperties(const CSCProps *props, uint8_t *s, int full)   // csc_enc.cpp:145-158
{
    (void)full;
    uint32_t d = (uint32_t)props->dict_size;
    s[0] = (uint8_t)(d >> 24); s[1] = (uint8_t)(d >> 16); s[2] = (uint8_t)(d >> 8); s[3] = (uint8_t)d;
    s[4] = (uint8_t)(props->csc_blocksize >> 16); s[5] = (uint8_t)(props->csc_blocksize >> 8); s[6] = (uint8_t)props->csc_blocksize;
    s[7] = (uint8_t)(props->raw_blocksize >> 16); s[8] = (uint8_t)(props->raw_blocksize >> 8); s[9] = (uint8_t)props->raw_blocksize;
}

uint64_t CSCEnc_EstMemUsage(const CSCProps *p)   // csc_enc.cpp:99-112 (same 32-bit intermediate arithmetic)
{
    uint64_t ret = p->dict_size;
    ret += p->csc_blocksize * 2;
    if (p->bt_size) ret += (uint64_t)(uint32_t)((1u << p->bt_hash_bits) + 2 * p->bt_size) * sizeof(uint32_t);
    if (p->hash_width) ret += (uint64_t)(int64_t)(int)(p->hash_width * (1 << p->hash_bits)) * sizeof(uint32_t);
    ret += 80 * kKB * sizeof(uint32_t);
    ret += 256 * 256 * sizeof(uint32_t) * 2;
    ret += 2 * kMB;
    return ret;
}

CSCEncHandle CSCEnc_Create(const CSCProps *props, ISeqOutStream *outstream, ISzAlloc *alloc)   // csc_enc.cpp:114-133
{
    if (alloc == NULL) alloc = &g_default_alloc;
    if (CSCMI_DeviceCheck() != 0) return NULL;
    // (enc_props_ok below restates this refusal for CSCMI_EncodeDeviceBatch, which must tell it from a device failure: keep the two in step)
    if (props->csc_blocksize == 0 || props->csc_blocksize >= 16 * kMB || props->raw_blocksize == 0
        || props->raw_blocksize >= 16 * kMB || props->hash_width > 32
        || (props->lz_mode != 1 && props->lz_mode != 2 && props->lz_mode != 3)
        || (props->hash_width && (props->hash_bits < 1 || props->hash_bits > 28))
        || (props->bt_size && props->bt_hash_bits && (props->bt_hash_bits > 28))) {
        fprintf(stderr, "csc-mi355x: unsupported CSCProps\n");
        return NULL;
    }

    EncInstance *e = (EncInstance *)alloc->Alloc(alloc, sizeof(EncInstance));
    if (!e) return NULL;
    memset(e, 0, sizeof(*e));
    e->magic = kMagicEnc; e->alloc = alloc; e->os = outstream; e->props = *props;
    e->parser = props->lz_mode == 3 ? 3 : 2;
    {   // hash-table-only configuration (levels 1-4): the specialised kernels (bit 4 of the launch kind)
        bool bt = props->bt_hash_bits && props->bt_size;
        bool ht = props->hash_bits && props->hash_width;
        if (!bt && ht && props->hash_width <= 9) e->parser |= 4;
        // level-3 geometry: the pipeline form of the advanced parser (csc_kernels_dp4.inc)
        if ((e->parser & 4) && props->lz_mode == 3 && props->hash_width <= 2 && props->good_len >= 2 && props->good_len <= 16) e->parser |= 8;
        // level-5 geometry -- binary tree, no bucket, advanced parser: the inserter form (csc_kernels_bt.inc)
        if (bt && !ht && props->lz_mode == 3 && props->bt_cyc <= 32) e->parser |= 16;
        // lazy / greedy parser over a bucket of up to eight (levels 1, 2): the inserter form (csc_kernels_hp.inc)
        if ((e->parser & 4) && props->lz_mode != 3 && props->hash_width <= 8) e->parser |= 32;
    }
    bool ok = hipGetDevice(&e->device) == hipSuccess;
    // each process/thread may sit on another device: the constant tables are per device
    DevTables dt = {nullptr, nullptr, false};
    if (ok) ok = device_tables(e->device, dt) == hipSuccess;

    EncState &h = e->h;
    // LZ::Init / MatchFinder::Init geometry, csc_lz.cpp:15-33, csc_mf.cpp:45-106
    uint32_t wnd = (uint32_t)(props->dict_size > 0xFFFFFFFFull ? 0xFFFFFFFFull : props->dict_size);
    if (wnd < 32 * kKB) wnd = 32 * kKB;
    if (wnd > 1024 * kMB) wnd = 1024 * kMB;
    h.wnd_size = wnd;
    h.vld_rge = wnd - kMinBlock - 4;
    h.bsize = props->csc_blocksize; h.raw_blocksize = props->raw_blocksize;
    h.ht_bits = props->hash_bits; h.ht_width = props->hash_width;
    h.bt_bits = props->bt_hash_bits; h.bt_size = props->bt_size;
    if (!h.bt_bits || !h.bt_size) h.bt_bits = h.bt_size = 0;
    if (!h.ht_bits || !h.ht_width) h.ht_bits = h.ht_width = 0;
    h.lz_mode = props->lz_mode; h.lz_good_len = props->good_len;
    h.lz_bt_cyc = props->bt_cyc; h.lz_ht_cyc = props->hash_width;
    h.mf_size = (uint64_t)kHT2Size + kHT3Size + ((uint64_t)h.ht_width << h.ht_bits);
    if (h.bt_bits) h.mf_size += ((uint64_t)1 << h.bt_bits) + (uint64_t)h.bt_size * 2;
    h.arena_cap = arena_bytes(props->raw_blocksize, props->csc_blocksize);
    h.filt_flags = (props->DLTFilter ? 1u : 0u) | (props->TXTFilter ? 2u : 0u) | (props->EXEFilter ? 4u : 0u);

    // ---- one device slab, zero-filled: memset(wnd_, 0, ..) csc_lz.cpp:50, the tables csc_mf.cpp:73, and the
    // coder buffers, which the reference reads before writing (App. C #1)
    size_t doff = 0;
    auto dtake = [&](size_t bytes) { size_t o = doff; doff += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_wnd = dtake((size_t)wnd + 256), o_mf = dtake((h.mf_size + 64) * sizeof(uint32_t));
    const size_t o_plit = dtake(256 * 256 * sizeof(uint32_t)), o_pdelta = dtake(256 * 256 * sizeof(uint32_t));
    const size_t o_rc = dtake((size_t)h.bsize + 64), o_bc = dtake((size_t)h.bsize + 64);
    const size_t o_in = dtake((size_t)h.raw_blocksize + 256), o_swap = dtake(4 * (size_t)h.raw_blocksize + 512);
    const size_t o_arena = dtake((size_t)h.arena_cap + 64), o_binfo = dtake(sizeof(BlockInfo) * kMaxBlocksPerChunk);
#ifdef CSCMI_STAGE_TEST
    const size_t o_result = dtake(256);                                 // CSCST_Filter's result word
#endif
    const size_t o_undo = dtake(h.bt_bits ? kBtUndoBytes : 0);          // (its own region: the filter scratch can be smaller than the log when raw_blocksize is)
    const size_t o_state = dtake(sizeof(EncState));
    e->dsize = doff;
    // ---- one pinned slab
    size_t hoff = 0;
    auto htake = [&](size_t bytes) { size_t o = hoff; hoff += (bytes + 255) & ~(size_t)255; return o; };
    const size_t p_small = htake(64);

    if (ok) { e->res = host_res_get(e->device, hoff); ok = e->res != nullptr; }
    if (ok) { e->dslab = dev_slab_get(e->device, e->dsize); ok = e->dslab != nullptr; }
    if (ok) {
        e->stream = e->res->stream; e->ev = e->res->ev; e->ev_an = e->res->ev_an;
        uint8_t *D = (uint8_t *)e->dslab, *H = e->res->hslab;
        h.wnd = D + o_wnd; h.mfbuf = (uint32_t *)(D + o_mf); h.p_lit = (uint32_t *)(D + o_plit); h.p_delta = (uint32_t *)(D + o_pdelta);
        h.rc_buf = D + o_rc; h.bc_buf = D + o_bc; h.inbuf = D + o_in; h.swapbuf = D + o_swap; h.arena = D + o_arena;
        h.bt_undo = h.bt_bits ? D + o_undo : nullptr;
        h.binfo = (BlockInfo *)(D + o_binfo); e->d_trie = dt.trie;
        e->d_entcoef = dt.coef; e->d_state = (EncState *)(D + o_state);
#ifdef CSCMI_STAGE_TEST
        e->d_result = (uint32_t *)(D + o_result);
#endif
        e->h_in = e->res->h_in;
        e->h_small = (uint32_t *)(H + p_small);
        ok = hipMemsetAsync(e->dslab, 0, e->dsize, e->stream) == hipSuccess;
    }
    hipStream_t st = e->stream;
    if (!ok) {
        fprintf(stderr, "csc-mi355x: device allocation failed (%s)\n", hipGetErrorString(hipGetLastError()));
        free_device(e);
        alloc->Free(alloc, e);
        return NULL;
    }
    uint64_t cpos = 0;
    h.ht2 = h.mfbuf + cpos; cpos += kHT2Size;
    h.ht3 = h.mfbuf + cpos; cpos += kHT3Size;
    if (h.ht_width) { h.ht6 = h.mfbuf + cpos; cpos += (uint64_t)h.ht_width << h.ht_bits; } else h.ht6 = nullptr;
    if (h.bt_bits) { h.bt_head = h.mfbuf + cpos; cpos += (uint64_t)1 << h.bt_bits; h.bt_nodes = h.mfbuf + cpos; }
    else { h.bt_head = nullptr; h.bt_nodes = nullptr; }
    h.trie_next = (const uint16_t *)e->d_trie;
    h.trie_sym = e->d_trie + 300 * 26 * 2;

    ok = hipMemcpyAsync(e->d_state, &h, sizeof(EncState), hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        launch_init_state(e->d_state, st);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(st) == hipSuccess;   // (`h` may change once this returns)
    if (!ok) {
        fprintf(stderr, "csc-mi355x: device initialisation failed (%s)\n", hipGetErrorString(hipGetLastError()));
        free_device(e);
        alloc->Free(alloc, e);
        return NULL;
    }
    return (CSCEncHandle)e;
}

void CSCEnc_Destroy(CSCEncHandle p)   // csc_enc.cpp:135-143
{
    EncInstance *e = (EncInstance *)p;
    if (!e || e->magic != kMagicEnc) return;
    free_device(e);
    e->magic = 0;
    ISzAlloc *a = e->alloc;
    a->Free(a, e);
}

int CSCMI_EncodeHostChunk(CSCEncHandle p, const void *host_ptr, size_t size)
{
    return encode_chunk((EncInstance *)p, host_ptr, size, false);
}
int CSCMI_EncodeDeviceChunk(CSCEncHandle p, const void *device_ptr, size_t size)
{
    return encode_chunk((EncInstance *)p, device_ptr, size, true);
}

// Many independent streams (the archiver's -p / per-extension tasks, csarc.cpp:532-557) advanced by one
// chunk each with ONE kernel launch: one workgroup per stream.  hs[i] encodes sizes[i] bytes at
// device_ptrs[i]; the Write callbacks of all handles run on this thread, in handle order.
int CSCMI_EncodeDeviceChunkBatch(int n, CSCEncHandle *hs, const void *const *device_ptrs, const size_t *sizes)
{
    if (n <= 0) return 0;
    if (n > kMaxBatch) return -1;
    EncInstance *lead = (EncInstance *)hs[0];
    HIPCHK(hipSetDevice(lead->device));
    { int r = batch_args_ready(lead->device); if (r) return r; }
    HIPCHK(host_events(lead->res));
    void **const d_batch = t_batch.d, **const h_batch = t_batch.h;
    int rc = 0;
    static const bool trace = getenv("CSCMI_BATCH_TRACE") != nullptr;      // development: one line per call on stderr
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto tms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_begin = tnow();
    // every stream walks its chunk itself: upload + analyzer per stream, then ONE launch per kernel flavour, one workgroup a stream
    for (int i = 0; i < n && !rc; i++) {
        if (!sizes[i]) continue;
        EncInstance *e = (EncInstance *)hs[i];
        if (e->stats.chunks == 0 && e->stream != lead->stream) HIPCHK(hipStreamSynchronize(e->stream));   // (its state was initialised on its own stream)
        rc = chunk_begin(e, device_ptrs[i], sizes[i], true, lead->stream);
    }
    if (rc) return rc;
    for (int parser = 2; parser <= 63; parser++) {
        if ((parser & 3) < 2) continue;
        uint32_t m = 0;
        EncState **st = (EncState **)h_batch;
        const RunDesc **rl = (const RunDesc **)(h_batch + kMaxBatch);
        uint32_t *cnt = (uint32_t *)(h_batch + 2 * kMaxBatch);
        uint32_t *rst = (uint32_t *)(h_batch + 3 * kMaxBatch);
        for (int i = 0; i < n; i++) {
            EncInstance *e = (EncInstance *)hs[i];
            if (!sizes[i] || e->parser != parser) continue;
            st[m] = e->d_state; rl[m] = nullptr; cnt[m] = kSelfSegment | (uint32_t)sizes[i]; rst[m] = 1u;
            m++;
        }
        if (!m) continue;
        HIPCHK(hipMemcpyAsync(d_batch, h_batch, sizeof(void *) * 4 * kMaxBatch, hipMemcpyHostToDevice, lead->stream));
        HIPCHK(hipEventRecord(lead->ev[0], lead->stream));
        launch_encode_runs_multi(parser, m, (EncState *const *)d_batch, (const RunDesc *const *)(d_batch + kMaxBatch),
                                 (const uint32_t *)(d_batch + 2 * kMaxBatch), (const uint32_t *)(d_batch + 3 * kMaxBatch), lead->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(lead->ev[1], lead->stream));
        HIPCHK(hipStreamSynchronize(lead->stream));          // (the pointer tables are reused by the next flavour)
        float ms = 0;
        if (hipEventElapsedTime(&ms, lead->ev[0], lead->ev[1]) == hipSuccess) lead->stats.encode_kernel_ms += ms;
        lead->stats.encode_launches++;
    }
    const auto t_dr = tnow();
    for (int i = 0; i < n; i++) {
        if (!sizes[i]) continue;
        EncInstance *e = (EncInstance *)hs[i];
        e->stats.chunks++;
        e->stats.input_bytes += sizes[i];
    }
    rc = drain_batch(n, hs, sizes, lead->stream);
    if (trace) fprintf(stderr, "batch trace: %d streams, kernels walk their chunks: launches %.1f ms, drain %.1f ms\n", n, tms(t_begin, t_dr), tms(t_dr, tnow()));
    return rc;
}

// CSCEnc_Encode, csc_enc.cpp:160-191: exactly one Read of raw_blocksize per chunk; a short read
// IS the chunk; Progress after every chunk, return value ignored.
int CSCEnc_Encode(CSCEncHandle p, ISeqInStream *is, ICompressProgress *progress)
{
    EncInstance *e = (EncInstance *)p;
    int ret = 0;
    uint64_t insize = 0;
    if (!e->h_in) {   // pinned staging for the caller's Read, kept with the recycled host resources
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipHostMalloc((void **)&e->res->h_in, e->props.raw_blocksize, hipHostMallocDefault));
        e->h_in = e->res->h_in;
    }
    for (;;) {
        size_t size = e->props.raw_blocksize;
        ret = is->Read(is, e->h_in, &size);
        if (ret >= 0 && size) {
            insize += size;
            ret = encode_chunk(e, e->h_in, size, false);
            if (progress) progress->Progress(progress, insize, (uint64_t)e->outsize);
        } else if (ret < 0) {
            ret = READ_ERROR;
        }
        if (ret < 0 || size == 0) break;
    }
    return ret;
}

// CSCEnc_Encode_Flush, csc_enc.cpp:193-203: WriteEOF (EncodeInt(SIG_EOF)) + Coder::Flush
int CSCEnc_Encode_Flush(CSCEncHandle p)
{
    EncInstance *e = (EncInstance *)p;
    HIPCHK(hipSetDevice(e->device));
    launch_encode_eof(e->d_state, e->stream);
    HIPCHK(hipGetLastError());
    return drain_arena(e, false);
}

// CSCEnc_Encode_Flush for many handles of one device: every EOF kernel queued on one stream, one wait, the last blocks handed to
// the users' streams in handle order.  (2048 task streams of the archiver: one round trip instead of 2048.)
int CSCMI_FlushBatch(int n, CSCEncHandle *hs)
{
    if (n <= 0) return 0;
    EncInstance *lead = (EncInstance *)hs[0];
    HIPCHK(hipSetDevice(lead->device));
    for (int i = 0; i < n; i += kMaxBatch) {
        const int m = n - i < kMaxBatch ? n - i : kMaxBatch;
        { int r = batch_args_ready(lead->device); if (r) return r; }
        for (int k = 0; k < m; k++) {
            EncInstance *e = (EncInstance *)hs[i + k];
            if (e->device != lead->device) return -1;
            launch_encode_eof(e->d_state, lead->stream);
        }
        HIPCHK(hipGetLastError());
        int r = drain_batch(m, hs + i, nullptr, lead->stream);
        if (r) return r;
    }
    return 0;
}

// Not in the reference: whole inputs that lie in device memory encoded into streams that lie in device memory, n at once -- the
// mirror image of CSCMI_DecodeDeviceBatch.  Per-stream state is a CSCEnc_Create handle without an output stream (so a recycled
// slab is initialised exactly as CSCEnc_Create initialises it) that goes back to the caches when the call ends.  A round is what
// CSCMI_EncodeDeviceChunkBatch queues -- chunk_begin for every live stream, one encode launch per kernel flavour -- and then, in
// place of drain_batch, ONE launch of k_frame_blocks (csc_enc_frame.hip) that frames every stream's arena into its destination
// under the dst_cap rule.  The last round queues k_encode_eof for every stream and frames again.  The host reads back one
// FrameStatus {error, rc, produced} per live stream per round, 16 bytes, and nothing else: no coder block crosses the bus.
static bool enc_props_ok(const CSCProps *props)      // CSCEnc_Create's refusal, restated (a note there points here): the two change together
{
    return !(props->csc_blocksize == 0 || props->csc_blocksize >= 16 * kMB || props->raw_blocksize == 0
             || props->raw_blocksize >= 16 * kMB || props->hash_width > 32
             || (props->lz_mode != 1 && props->lz_mode != 2 && props->lz_mode != 3)
             || (props->hash_width && (props->hash_bits < 1 || props->hash_bits > 28))
             || (props->bt_size && props->bt_hash_bits && (props->bt_hash_bits > 28)));
}

int CSCMI_EncodeDeviceBatch(int n, CSCMIDevEncode *jobs, CSCMIDevEncodeStats *stats)
{
    if (stats) { stats->launches = stats->rounds = stats->readback_bytes = 0; stats->kernel_ms = 0; }
    if (n <= 0) return 0;
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    { int r = batch_args_ready(device); if (r) return r; }
    void **const d_batch = t_batch.d, **const h_batch = t_batch.h;
    hipStream_t st = pooled_stream(device);
    if (!st) return CSCMI_DEVICE_ERROR;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};       // [0], [1] around an encode or a framing launch, [2], [3] around the flush kernels
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess || hipEventCreate(&ev[2]) != hipSuccess
        || hipEventCreate(&ev[3]) != hipSuccess) {
        for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
        pooled_stream_release(device, st);
        return CSCMI_DEVICE_ERROR;
    }
    static const bool trace = getenv("CSCMI_BATCH_TRACE") != nullptr;      // development: one line per call on stderr
    double frame_ms = 0, all_ms = 0;
    uint64_t launches = 0, rounds = 0, readback = 0;
    for (int i = 0; i < n; i++) { jobs[i].produced = 0; jobs[i].rc = CSCMI_DEVICE_ERROR; }
    struct Slot { int job; EncInstance *e; uint64_t chunks; bool live; };
    int dev_rc = 0, next = 0;
    while (next < n && !dev_rc) {
        // a group: as many of the remaining jobs as the free device memory (and what the slab cache holds) can carry, kMaxBatch at most
        std::vector<Slot> grp;
        size_t free_b = 0, total_b = 0, used = 0, cached = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { dev_rc = CSCMI_DEVICE_ERROR; break; }
        { std::lock_guard<std::mutex> lk(g_cache_mu); cached = g_dev_cache_bytes; }
        const size_t room = (free_b + cached) / 8 * 7;
        for (; next < n && grp.size() < (size_t)kMaxBatch; next++) {
            CSCMIDevEncode &job = jobs[next];
            if (!enc_props_ok(&job.props)) { job.rc = CSCMI_NO_ENCODER; continue; }
            EncInstance *e = (EncInstance *)CSCEnc_Create(&job.props, nullptr, nullptr);
            if (!e) {
                if (!grp.empty()) break;                       // this group first; the job is tried again with its memory back
                continue;                                      // (rc stays CSCMI_DEVICE_ERROR; the other jobs proceed)
            }
            if (!grp.empty() && used + e->dsize > room) { CSCEnc_Destroy(e); break; }
            used += e->dsize;
            const uint64_t raw = job.props.raw_blocksize;
            grp.push_back(Slot{next, e, ((uint64_t)job.src_size + raw - 1) / raw, true});
        }
        if (grp.empty()) continue;
        const size_t m = grp.size();
        // device: the job records (they persist across the rounds), the round's items and its status array; pinned: their host sides
        uint8_t *d_mem = nullptr, *h_mem = nullptr;
        const size_t per = sizeof(FrameJob) + sizeof(FrameItem) + sizeof(FrameStatus);
        bool ok = hipMalloc((void **)&d_mem, per * m) == hipSuccess && hipHostMalloc((void **)&h_mem, per * m, hipHostMallocDefault) == hipSuccess;
        FrameJob *d_jobs = (FrameJob *)d_mem, *h_jobs = (FrameJob *)h_mem;
        FrameItem *d_items = (FrameItem *)(d_mem + sizeof(FrameJob) * m), *h_items = (FrameItem *)(h_mem + sizeof(FrameJob) * m);
        FrameStatus *d_status = (FrameStatus *)(d_mem + (sizeof(FrameJob) + sizeof(FrameItem)) * m);
        FrameStatus *h_status = (FrameStatus *)(h_mem + (sizeof(FrameJob) + sizeof(FrameItem)) * m);
        uint64_t max_chunks = 0;
        if (ok) {
            for (size_t k = 0; k < m; k++) {
                const CSCMIDevEncode &job = jobs[grp[k].job];
                h_jobs[k] = FrameJob{(uint8_t *)job.dst, (uint64_t)job.dst_cap, 0, 0, 0};
                if (grp[k].chunks > max_chunks) max_chunks = grp[k].chunks;
            }
            ok = hipMemcpyAsync(d_jobs, h_jobs, sizeof(FrameJob) * m, hipMemcpyHostToDevice, st) == hipSuccess;
        }
        std::vector<size_t> in_round;
        // frame what the round's kernels left in the arenas of `in_round`, read the status array back, retire what has ended
        auto frame_round = [&]() -> bool {
            const size_t c = in_round.size();
            if (!c) return true;
            for (size_t k = 0; k < c; k++) h_items[k] = FrameItem{grp[in_round[k]].e->d_state, (uint32_t)in_round[k], 0};
            bool good = hipMemcpyAsync(d_items, h_items, sizeof(FrameItem) * c, hipMemcpyHostToDevice, st) == hipSuccess
                     && hipEventRecord(ev[0], st) == hipSuccess;
            if (good) {
                launch_frame_blocks(d_items, d_jobs, d_status, (uint32_t)c, st);
                good = hipGetLastError() == hipSuccess && hipEventRecord(ev[1], st) == hipSuccess;
            }
            good = good && hipMemcpyAsync(h_status, d_status, sizeof(FrameStatus) * c, hipMemcpyDeviceToHost, st) == hipSuccess
                        && hipStreamSynchronize(st) == hipSuccess;
            float ms = 0;
            good = good && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess;
            if (!good) return false;
            launches++; readback += sizeof(FrameStatus) * c; frame_ms += ms; all_ms += ms;
            for (size_t k = 0; k < c; k++) {
                Slot &s = grp[in_round[k]];
                CSCMIDevEncode &job = jobs[s.job];
                job.produced = (size_t)h_status[k].produced;
                if (h_status[k].error != ERR_NONE) {               // (rc stays CSCMI_DEVICE_ERROR)
                    if (h_status[k].error == kFrameErrArena) fprintf(stderr, "csc-mi355x: device encoder error 0x%x (a coder block record does not lie inside the arena)\n", kFrameErrArena);
                    else (void)report_device_error(h_status[k].error);
                    s.live = false;
                }
                else if (h_status[k].rc != 0) { job.rc = h_status[k].rc; s.live = false; }
            }
            return true;
        };
        for (uint64_t r = 0; r < max_chunks && ok; r++) {
            in_round.clear();
            for (size_t k = 0; k < m && ok; k++) {
                Slot &s = grp[k];
                if (!s.live || r >= s.chunks) continue;
                const CSCMIDevEncode &job = jobs[s.job];
                const uint64_t raw = job.props.raw_blocksize, off = r * raw;
                const size_t size = (size_t)(job.src_size - off < raw ? job.src_size - off : raw);
                ok = chunk_begin(s.e, (const uint8_t *)job.src + off, size, true, st) == 0;
                in_round.push_back(k);
            }
            // one launch per kernel flavour, one workgroup a stream: as CSCMI_EncodeDeviceChunkBatch queues them
            for (int parser = 2; parser <= 63 && ok; parser++) {
                if ((parser & 3) < 2) continue;
                uint32_t c = 0;
                EncState **sp = (EncState **)h_batch;
                const RunDesc **rl = (const RunDesc **)(h_batch + kMaxBatch);
                uint32_t *cnt = (uint32_t *)(h_batch + 2 * kMaxBatch);
                uint32_t *rst = (uint32_t *)(h_batch + 3 * kMaxBatch);
                for (size_t k : in_round) {
                    const Slot &s = grp[k];
                    if (s.e->parser != parser) continue;
                    const CSCMIDevEncode &job = jobs[s.job];
                    const uint64_t raw = job.props.raw_blocksize, off = r * raw;
                    sp[c] = s.e->d_state; rl[c] = nullptr; rst[c] = 1u;
                    cnt[c] = kSelfSegment | (uint32_t)(job.src_size - off < raw ? job.src_size - off : raw);
                    c++;
                }
                if (!c) continue;
                ok = hipMemcpyAsync(d_batch, h_batch, sizeof(void *) * 4 * kMaxBatch, hipMemcpyHostToDevice, st) == hipSuccess
                  && hipEventRecord(ev[0], st) == hipSuccess;
                if (ok) {
                    launch_encode_runs_multi(parser, c, (EncState *const *)d_batch, (const RunDesc *const *)(d_batch + kMaxBatch),
                                             (const uint32_t *)(d_batch + 2 * kMaxBatch), (const uint32_t *)(d_batch + 3 * kMaxBatch), st);
                    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev[1], st) == hipSuccess
                      && hipStreamSynchronize(st) == hipSuccess;          // (the pointer tables are reused by the next flavour)
                }
                float ms = 0;
                if (ok && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) all_ms += ms;
                launches++;
            }
            ok = ok && frame_round();
            rounds++;
        }
        if (ok) {                                              // CSCEnc_Encode_Flush for every stream that still lives
            in_round.clear();
            ok = hipEventRecord(ev[2], st) == hipSuccess;      // one event pair around all the flush kernels: they run back to back on `st`
            for (size_t k = 0; k < m && ok; k++) {
                if (!grp[k].live) continue;
                launch_encode_eof(grp[k].e->d_state, st);
                launches++;
                in_round.push_back(k);
            }
            ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev[3], st) == hipSuccess && frame_round();
            float ms = 0;
            if (ok && !in_round.empty() && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) all_ms += ms;   // (frame_round has waited for the stream)
            rounds++;
            if (ok) for (size_t k : in_round) if (grp[k].live) jobs[grp[k].job].rc = 0;
        }
        if (!ok) dev_rc = CSCMI_DEVICE_ERROR;
        (void)hipStreamSynchronize(st);
        if (d_mem) (void)hipFree(d_mem);
        if (h_mem) (void)hipHostFree(h_mem);
        for (const Slot &s : grp) CSCEnc_Destroy(s.e);
    }
    for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    pooled_stream_release(device, st);
    if (stats) { stats->launches = launches; stats->rounds = rounds; stats->readback_bytes = readback; stats->kernel_ms = all_ms; }
    if (trace) fprintf(stderr, "encode-device trace: %d jobs, %llu rounds, %llu launches, kernels %.3f ms of which framing %.3f ms, read back %llu bytes\n",
                       n, (unsigned long long)rounds, (unsigned long long)launches, all_ms, frame_ms, (unsigned long long)readback);
    return dev_rc;
}

void CSCMI_GetStats(CSCEncHandle p, CSCMIStats *out)
{
    EncInstance *e = (EncInstance *)p;
    KernelStats ks;
    memset(&ks, 0, sizeof(ks));
    (void)hipSetDevice(e->device);
    if (hipMemcpy(&ks, &e->d_state->stats, sizeof(ks), hipMemcpyDeviceToHost) == hipSuccess) {
        e->stats.find_match_calls = ks.find_match_calls; e->stats.slide_positions = ks.slide_positions;
        e->stats.bt_steps = ks.bt_steps; e->stats.literals = ks.literals; e->stats.matches = ks.matches;
    }
    *out = e->stats;
}

#ifdef CSCMI_STAGE_TEST
// Test-only entry points (tests/stage/libcsc_stage.so -- the same sources built with -DCSCMI_STAGE_TEST; the product library does
// not have them): the analyzer kernel and the three forward filters on a caller-supplied buffer, one stage at a time.

// out: 7 words per 8 KiB block: type, bpb, dlt_bpb[5] (csc_analyzer.cpp:184-239, :166-182)
int CSCST_Analyze(CSCEncHandle p, const void *host, size_t size, uint32_t *out)
{
    EncInstance *e = (EncInstance *)p;
    if (!e || size == 0 || size > e->props.raw_blocksize) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->h.inbuf, host, size, hipMemcpyHostToDevice, e->stream));
    const uint32_t nblk = ((uint32_t)size + kMinBlock - 1) / kMinBlock;
    HIPCHK(hipMemsetAsync(e->h.binfo, 0xEE, sizeof(BlockInfo) * nblk, e->stream));
    launch_analyze(e->d_state, (uint32_t)size, e->d_entcoef, e->stream);
    HIPCHK(hipGetLastError());
    BlockInfo *bi = (BlockInfo *)thread_pinned(sizeof(BlockInfo) * nblk);
    if (!bi) return CSCMI_DEVICE_ERROR;
    HIPCHK(hipMemcpyAsync(bi, e->h.binfo, sizeof(BlockInfo) * nblk, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (uint32_t b = 0; b < nblk; b++) {
        out[b * 7] = bi[b].type; out[b * 7 + 1] = bi[b].bpb;
        for (int k = 0; k < 5; k++) out[b * 7 + 2 + k] = bi[b].dlt_bpb[k];
    }
    return 0;
}

// kind 0 Forward_E89, 1 Foward_Dict (*result = its return value), 2 Forward_Delta with `chn` channels; buf is transformed in place
int CSCST_Filter(CSCEncHandle p, int kind, void *buf, size_t size, uint32_t chn, uint32_t *result)
{
    EncInstance *e = (EncInstance *)p;
    if (!e || size == 0 || size > e->props.raw_blocksize) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->h.inbuf, buf, size, hipMemcpyHostToDevice, e->stream));
    launch_stage_filter(e->d_state, (uint32_t)kind, (uint32_t)size, chn, e->d_result, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(buf, e->h.inbuf, size, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(e->h_small, e->d_result, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (result) *result = e->h_small[0];
    return 0;
}
// the match finder's position counter (EncState::pos; MatchFinder::Init leaves it at vld_rge_ over zeroed tables): a start close to
// 0xFFFFFFF0 brings the renormalisation of csc_mf.cpp:108-114 within reach of a test.  Right after CSCEnc_Create.
int CSCST_SetPos(CSCEncHandle p, uint32_t pos)
{
    EncInstance *e = (EncInstance *)p;
    if (!e) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(&e->d_state->pos, &pos, sizeof(pos), hipMemcpyHostToDevice));
    return 0;
}
#endif   // CSCMI_STAGE_TEST

#ifdef CSCMI_TIMERS
// development aids (tools/gpu_timers.py, tools/gpu_trace.py): only in the -DCSCMI_TIMERS build, never in the product library
void CSCMI_DebugTimers(CSCEncHandle p, uint64_t *out16)
{
    EncInstance *e = (EncInstance *)p;
    KernelStats ks;
    memset(&ks, 0, sizeof(ks));
    (void)hipSetDevice(e->device);
    (void)hipMemcpy(&ks, &e->d_state->stats, sizeof(ks), hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; i++) out16[i] = ks.tm[i];
}

void CSCMI_DebugSetMask(CSCEncHandle p, uint64_t mask)      // csc_kernels_dp4.inc: D5DBG
{
    EncInstance *e = (EncInstance *)p;
    (void)hipSetDevice(e->device);
    (void)hipMemcpy(&e->d_state->stats.trace[63][0], &mask, sizeof(mask), hipMemcpyHostToDevice);
}

void CSCMI_DebugTrace(CSCEncHandle p, uint64_t *out768)
{
    EncInstance *e = (EncInstance *)p;
    static KernelStats ks;
    memset(&ks, 0, sizeof(ks));
    (void)hipSetDevice(e->device);
    (void)hipMemcpy(&ks, &e->d_state->stats, sizeof(ks), hipMemcpyDeviceToHost);
    memcpy(out768, ks.trace, sizeof(ks.trace));
}
#endif   // CSCMI_TIMERS

}  // extern "C"
