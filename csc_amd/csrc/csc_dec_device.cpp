// csc_dec_device.cpp -- CSCDec_* of libcsc_mi355x.so served by k_decode_run (csc_dec_kernels.hip).
//
// The host thread owns the callbacks and the block framing, the GPU owns the stream state and all
// decoding work:
//   * MemIO::ReadBlock (csc_memio.cpp:5-81) is reproduced here read for read: when the kernel reports
//     that it ran out of RC (or BC) bytes, blocks are read from the ISeqInStream -- flag byte, optional
//     3-byte size, ONE Read for the payload -- until one of the wanted kind turns up; every block read
//     on the way is uploaded to its ring on the device, which is the reference's queue of the
//     "other" kind.
//   * CSCDec_Decode (csc_dec.cpp:740-777) loops over Decompress calls; each is one or more launches
//     of the resumable kernel; the decoded run is copied back and handed to ISeqOutStream::Write.
//   * CSCMI_DecodeDeviceBatch is the path without callbacks: streams that lie in device memory, raw bytes that stay
//     there; block reader and run delivery are in the kernel (k_decode_dev*), the host only relaunches live streams.
//     CSCMI_DecodeDeviceBatchStop is the same call with a stop position per stream (DecState::stop_at, DEC_STOPPED).
// No CPU decoding path exists in this library.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/csc_mi355x.h"
#include "csc_device.h"
#include "csc_tables.h"

namespace cscmi {
void launch_decode_init(DecState *D, hipStream_t st);
void launch_decode_run(DecState *D, hipStream_t st);
void launch_decode_run_multi(DecState *const *states, uint32_t n, hipStream_t st);
void launch_decode_dev(DecState *const *states, DecState *first, uint32_t n, hipStream_t st);
hipStream_t pooled_stream(int device);                     // csc_host.cpp
void pooled_stream_release(int device, hipStream_t s);
}
using namespace cscmi;

namespace {

constexpr uint32_t kMagicDec = 0x43534344;   // "CSCD"

void *def_alloc(void *, size_t n) { return malloc(n); }
void def_free(void *, void *a) { free(a); }
ISzAlloc g_default_alloc = {def_alloc, def_free};

// A decoder's device state is ONE allocation (zero-filled on every use) and its pinned staging ONE allocation;
// both, and the HIP stream, are recycled through a per-process cache keyed by (device, sizes): an archive reader
// creates one decoder per task.
struct DecRes {
    int device;
    size_t dsize, hsize;
    uint8_t *dslab, *hslab;
    hipStream_t stream;
};
std::mutex g_dec_mu;
std::vector<DecRes *> g_dec_cache;
size_t g_dec_cache_bytes = 0;
constexpr size_t kDecCacheMaxBytes = 32ull << 30;
// CSCMI_DecodeDeviceBatch: output a launch delivers per stream before it returns (a few MiB = a second or two of kernel time at the
// 2.4-5.5 MB/s a stream decodes at; not tuned by measurement: profiles/decode_device.md), streams a group
constexpr uint64_t kDevLaunchBytes = 4ull << 20;
constexpr size_t kDevGroupMax = 1024;

void dec_res_destroy(DecRes *r)
{
    if (!r) return;
    if (r->dslab) (void)hipFree(r->dslab);
    if (r->hslab) (void)hipHostFree(r->hslab);
    if (r->stream) cscmi::pooled_stream_release(r->device, r->stream);
    delete r;
}
void dec_cache_trim()
{
    std::vector<DecRes *> drop;
    {
        std::lock_guard<std::mutex> lk(g_dec_mu);
        drop.swap(g_dec_cache);
        g_dec_cache_bytes = 0;
    }
    for (DecRes *r : drop) dec_res_destroy(r);
}
DecRes *dec_res_get(int device, size_t dsize, size_t hsize)
{
    {
        std::lock_guard<std::mutex> lk(g_dec_mu);
        for (size_t i = 0; i < g_dec_cache.size(); i++) {
            DecRes *r = g_dec_cache[i];
            if (r->device == device && r->dsize == dsize && r->hsize == hsize) {
                g_dec_cache.erase(g_dec_cache.begin() + i);
                g_dec_cache_bytes -= dsize;
                r->stream = cscmi::pooled_stream(device);      // (a recycled entry holds none while it sits in the cache)
                if (!r->stream) { dec_res_destroy(r); return nullptr; }
                return r;
            }
        }
    }
    DecRes *r = new DecRes();
    memset(r, 0, sizeof(*r));
    r->device = device; r->dsize = dsize; r->hsize = hsize;
    bool ok = (r->stream = cscmi::pooled_stream(device)) != nullptr;     // shared, csc_host.cpp: creating a stream costs ~4 ms here
    if (ok && hipMalloc((void **)&r->dslab, dsize) != hipSuccess) {
        (void)hipGetLastError();
        dec_cache_trim();                                  // give cached slabs back and try once more
        ok = hipMalloc((void **)&r->dslab, dsize) == hipSuccess;
    }
    ok = ok && hipHostMalloc((void **)&r->hslab, hsize, hipHostMallocDefault) == hipSuccess;
    if (!ok) { dec_res_destroy(r); return nullptr; }
    return r;
}
void dec_res_put(DecRes *r)
{
    if (!r) return;
    cscmi::pooled_stream_release(r->device, r->stream);
    r->stream = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_dec_mu);
        if (g_dec_cache_bytes + r->dsize <= kDecCacheMaxBytes && g_dec_cache.size() < 1024) {
            g_dec_cache.push_back(r);
            g_dec_cache_bytes += r->dsize;
            return;
        }
    }
    dec_res_destroy(r);
}

size_t dec_cache_bytes()
{
    std::lock_guard<std::mutex> lk(g_dec_mu);
    return g_dec_cache_bytes;
}

// where a decoder's pieces lie in its device slab and its pinned slab (both sizes are the resource cache's key)
struct DecLayout {
    size_t o_wnd, o_plit, o_out, o_swap, o_q0, o_q1, o_qs0, o_qs1, o_ua, o_uv, o_words, o_state, dsize;
    size_t p_read, p_block, p_out, hsize;
};
bool dec_props_ok(const CSCProps *props)   // csc_dec.cpp:697-700
{
    if (props->dict_size > 1024 * kMB || props->dict_size < 32 * kKB) return false;
    return props->csc_blocksize != 0 && props->raw_blocksize != 0;
}
// fills the configuration words of `h` from the properties and returns the layout that goes with them
DecLayout dec_layout(const CSCProps *props, DecState &h)
{
    h.wnd_size = (uint32_t)props->dict_size; h.bsize = props->csc_blocksize; h.raw_blocksize = props->raw_blocksize;
    h.qslots = 2 * (props->raw_blocksize / props->csc_blocksize + 1) + 16;
    DecLayout l;
    size_t doff = 0, hoff = 0;
    auto dtake = [&](size_t bytes) { size_t o = doff; doff += (bytes + 255) & ~(size_t)255; return o; };
    auto htake = [&](size_t bytes) { size_t o = hoff; hoff += (bytes + 255) & ~(size_t)255; return o; };
    l.o_wnd = dtake((size_t)h.wnd_size + 256); l.o_plit = dtake(2 * 65536 * sizeof(uint32_t));
    l.o_out = dtake((size_t)h.raw_blocksize + 256); l.o_swap = dtake(2 * (size_t)h.raw_blocksize + 256);
    l.o_q0 = dtake((size_t)h.qslots * h.bsize + 256); l.o_q1 = dtake((size_t)h.qslots * h.bsize + 256);
    l.o_qs0 = dtake(sizeof(uint32_t) * h.qslots); l.o_qs1 = dtake(sizeof(uint32_t) * h.qslots);
    l.o_ua = dtake(sizeof(uint32_t) * kDecUndoCap); l.o_uv = dtake(sizeof(uint32_t) * kDecUndoCap);
    l.o_words = dtake(sizeof(kWords)); l.o_state = dtake(sizeof(DecState));
    l.p_read = htake(sizeof(DecState)); l.p_block = htake(h.bsize); l.p_out = htake(h.raw_blocksize);
    l.dsize = doff; l.hsize = hoff;
    return l;
}
// the device pointers of `h` inside slab D, and the stream's start phase
void dec_place(DecState &h, uint8_t *D, const DecLayout &l)
{
    h.wnd = D + l.o_wnd; h.p_lit = (uint32_t *)(D + l.o_plit); h.out = D + l.o_out; h.swap = D + l.o_swap;
    h.q[0] = D + l.o_q0; h.q[1] = D + l.o_q1; h.qsize[0] = (uint32_t *)(D + l.o_qs0); h.qsize[1] = (uint32_t *)(D + l.o_qs1);
    h.undo_addr = (uint32_t *)(D + l.o_ua); h.undo_val = (uint32_t *)(D + l.o_uv);
    h.words = D + l.o_words;
    h.p_delta = h.p_lit + 65536;
    h.phase = DEC_PH_PRIME0;
}

struct DecInstance {
    uint32_t magic;
    DecRes *res;
    ISzAlloc *alloc;
    ISeqInStream *is;
    int device;
    hipStream_t stream;
    DecState *d_state;
    DecState h;               // host mirror: configuration + device pointers
    DecState *h_read;         // pinned read-back of the whole (small) state
    uint8_t *h_block;         // pinned staging for one block
    uint8_t *h_out;           // pinned decoded run
    uint32_t *h_qsize[2];     // host mirrors of the ring slot sizes
    uint32_t avail[2], taken[2];
    uint64_t consumed_view;   // GetCompressedSize as of the last launch
};

void free_all(DecInstance *x)
{
    (void)hipSetDevice(x->device);
    if (x->res) { (void)hipStreamSynchronize(x->res->stream); dec_res_put(x->res); }
    free(x->h_qsize[0]); free(x->h_qsize[1]);
    x->magic = 0;
    ISzAlloc *a = x->alloc;
    a->Free(a, x);
}

// MemIO::ReadBlock for a block that is not queued yet (csc_memio.cpp:17-79): read stream blocks until one of
// `kind` (1 RC, 0 BC) arrives; each block read goes to the device ring of its own kind.
int read_block(DecInstance *x, int kind)
{
    for (;;) {
        uint8_t fb, sb[3];
        size_t n = 1;
        x->is->Read(x->is, &fb, &n);
        if (n != 1) return -1;
        uint32_t cur = x->h.bsize;
        if (!((fb >> 6) & 1)) {
            n = 3;
            x->is->Read(x->is, sb, &n);
            if (n != 3) return -1;
            cur = ((uint32_t)sb[0] << 16) + ((uint32_t)sb[1] << 8) + sb[2];
        }
        if (!cur || cur > x->h.bsize) return -1;
        n = cur;
        x->is->Read(x->is, x->h_block, &n);       // ONE Read per payload; a short one is an error (:47-50)
        if (n != cur) return -1;
        int k2 = (fb >> 7) & 1;
        if (x->avail[k2] - x->taken[k2] >= x->h.qslots) {
            fprintf(stderr, "csc-mi355x: decoder block ring overflow\n");
            return -1;
        }
        uint32_t slot = x->avail[k2] % x->h.qslots;
        if (hipMemcpy(x->h.q[k2] + (size_t)slot * x->h.bsize, x->h_block, cur, hipMemcpyHostToDevice) != hipSuccess) return -1;
        x->h_qsize[k2][slot] = cur;
        x->avail[k2]++;
        if (k2 == kind) return 0;
    }
}

// run the kernel until the current Decompress call is complete; returns 0 / error code, *size = run length
int decompress(DecInstance *x, uint32_t *size)
{
    *size = 0;
    for (;;) {
        // publish what has been uploaded so far
        for (int k = 0; k < 2; k++)
            if (hipMemcpyAsync(x->h.qsize[k], x->h_qsize[k], sizeof(uint32_t) * x->h.qslots, hipMemcpyHostToDevice, x->stream) != hipSuccess) return CSCMI_DEVICE_ERROR;
        if (hipMemcpyAsync(&x->d_state->avail[0], x->avail, sizeof(x->avail), hipMemcpyHostToDevice, x->stream) != hipSuccess) return CSCMI_DEVICE_ERROR;
        launch_decode_run(x->d_state, x->stream);
        if (hipGetLastError() != hipSuccess) return CSCMI_DEVICE_ERROR;
        if (hipMemcpyAsync(x->h_read, x->d_state, offsetof(DecState, probs), hipMemcpyDeviceToHost, x->stream) != hipSuccess) return CSCMI_DEVICE_ERROR;
        if (hipStreamSynchronize(x->stream) != hipSuccess) return CSCMI_DEVICE_ERROR;
        const DecState &r = *x->h_read;
        x->taken[0] = r.taken[0]; x->taken[1] = r.taken[1];
        x->consumed_view = r.consumed + r.rd[0] + r.rd[1];
        switch (r.status) {
        case DEC_DONE:
            *size = r.out_size;
            return 0;
        case DEC_NEED_RC:
        case DEC_NEED_BC:
            if (read_block(x, r.status == DEC_NEED_RC ? 1 : 0) < 0)
                return r.phase == DEC_PH_PRIME ? -1 : READ_ERROR;     // csc_dec.cpp:669-671 vs :17-18
            break;
        case DEC_ERR_MINUS1: return -1;
        default: return DECODE_ERROR;
        }
    }
}

}  // namespace

extern "C" {

void CSCDec_ReadProperties(CSCProps *props, uint8_t *s)   // csc_dec.cpp:733-738
{
    props->dict_size = ((uint32_t)s[0] << 24) + ((uint32_t)s[1] << 16) + ((uint32_t)s[2] << 8) + s[3];
    props->csc_blocksize = ((uint32_t)s[4] << 16) + ((uint32_t)s[5] << 8) + s[6];
    props->raw_blocksize = ((uint32_t)s[7] << 16) + ((uint32_t)s[8] << 8) + s[9];
}

CSCDecHandle CSCDec_Create(const CSCProps *props, ISeqInStream *instream, ISzAlloc *alloc)   // csc_dec.cpp:692-720
{
    if (alloc == NULL) alloc = &g_default_alloc;
    if (!dec_props_ok(props)) return NULL;
    if (CSCMI_DeviceCheck() != 0) return NULL;
    DecInstance *x = (DecInstance *)alloc->Alloc(alloc, sizeof(DecInstance));
    if (!x) return NULL;
    memset(x, 0, sizeof(*x));
    x->magic = kMagicDec; x->alloc = alloc; x->is = instream;
    DecState &h = x->h;
    bool ok = hipGetDevice(&x->device) == hipSuccess;
    // one device slab (zero-filled) and one pinned slab
    const DecLayout l = dec_layout(props, h);
    if (ok) { x->res = dec_res_get(x->device, l.dsize, l.hsize); ok = x->res != nullptr; }
    if (ok) {
        uint8_t *D = x->res->dslab, *H = x->res->hslab;
        x->stream = x->res->stream;
        dec_place(h, D, l);
        x->d_state = (DecState *)(D + l.o_state);
        x->h_read = (DecState *)(H + l.p_read); x->h_block = H + l.p_block; x->h_out = H + l.p_out;
        ok = hipMemsetAsync(D, 0, l.dsize, x->stream) == hipSuccess
          && hipMemcpyAsync(D + l.o_words, kWords, sizeof(kWords), hipMemcpyHostToDevice, x->stream) == hipSuccess;
    }
    x->h_qsize[0] = (uint32_t *)calloc(h.qslots, sizeof(uint32_t));
    x->h_qsize[1] = (uint32_t *)calloc(h.qslots, sizeof(uint32_t));
    ok = ok && x->h_qsize[0] && x->h_qsize[1];
    if (ok) {
        ok = hipMemcpyAsync(x->d_state, &h, sizeof(DecState), hipMemcpyHostToDevice, x->stream) == hipSuccess;
        if (ok) {
            launch_decode_init(x->d_state, x->stream);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(x->stream) == hipSuccess;
        }
    }
    // CSCDecoder::Init already reads the first RC and BC block (csc_dec.cpp:336-337)
    if (!ok || read_block(x, 1) < 0 || read_block(x, 0) < 0) {
        if (!ok) fprintf(stderr, "csc-mi355x: decoder device allocation failed\n");
        free_all(x);
        return NULL;
    }
    return (CSCDecHandle)x;
}

void CSCDec_Destroy(CSCDecHandle p)   // csc_dec.cpp:722-731
{
    DecInstance *x = (DecInstance *)p;
    if (x && x->magic == kMagicDec) free_all(x);
}

int CSCDec_Decode(CSCDecHandle p, ISeqOutStream *os, ICompressProgress *progress)   // csc_dec.cpp:740-777
{
    DecInstance *x = (DecInstance *)p;
    if (hipSetDevice(x->device) != hipSuccess) return CSCMI_DEVICE_ERROR;
    int ret = 0;
    uint64_t outsize = 0;
    for (;;) {
        uint32_t size = 0;
        ret = decompress(x, &size);
        if (ret == 0) outsize += size;
        if (progress) progress->Progress(progress, x->consumed_view, outsize);
        if (size == 0 || ret < 0) break;
        if (hipMemcpy(x->h_out, x->h.out, size, hipMemcpyDeviceToHost) != hipSuccess) { ret = CSCMI_DEVICE_ERROR; break; }
        size_t wrote = os->Write(os, x->h_out, size);
        if (wrote == CSC_WRITE_ABORT) break;
        if (wrote < size) { ret = WRITE_ERROR; break; }
    }
    return ret;
}

#ifdef CSCMI_TIMERS
// development aid (section timers): only in the -DCSCMI_TIMERS build, never in the product library
void CSCMI_DebugDecTimers(CSCDecHandle p, uint64_t *out16)
{
    DecInstance *x = (DecInstance *)p;
    (void)hipMemcpy(out16, (const uint8_t *)x->d_state + offsetof(DecState, dbg), 16 * sizeof(uint64_t), hipMemcpyDeviceToHost);
}
#endif

// Not in the reference: CSCDec_Decode for n independent handles at once (the tasks of an archive).  Every round
// is ONE launch of k_decode_run_multi -- workgroup b advances stream b until it needs a block or has completed a
// Decompress call -- followed, per stream and on this thread, by exactly the callbacks CSCDec_Decode would make:
// the block reads MemIO::ReadBlock does for that stream, or the Write of its decoded run.  rcs[i] receives what
// CSCDec_Decode(hs[i], oss[i], NULL) would have returned.  Returns 0, or CSCMI_DEVICE_ERROR if the GPU side failed.
int CSCMI_DecodeBatch(int n, CSCDecHandle *hs, ISeqOutStream *const *oss, int *rcs)
{
    if (n <= 0) return 0;
    DecInstance *lead = (DecInstance *)hs[0];
    if (hipSetDevice(lead->device) != hipSuccess) return CSCMI_DEVICE_ERROR;
    hipStream_t st = lead->stream;
    DecState **d_list = nullptr, **h_list = nullptr;
    if (hipMalloc((void **)&d_list, sizeof(DecState *) * n) != hipSuccess) return CSCMI_DEVICE_ERROR;
    if (hipHostMalloc((void **)&h_list, sizeof(DecState *) * n, hipHostMallocDefault) != hipSuccess) { (void)hipFree(d_list); return CSCMI_DEVICE_ERROR; }
    std::vector<int> live;
    for (int i = 0; i < n; i++) { rcs[i] = 0; live.push_back(i); }
    int dev_rc = 0;
    while (!live.empty() && !dev_rc) {
        bool ok = true;
        for (size_t k = 0; k < live.size() && ok; k++) {
            DecInstance *x = (DecInstance *)hs[live[k]];
            for (int q = 0; q < 2 && ok; q++)
                ok = hipMemcpyAsync(x->h.qsize[q], x->h_qsize[q], sizeof(uint32_t) * x->h.qslots, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(&x->d_state->avail[0], x->avail, sizeof(x->avail), hipMemcpyHostToDevice, st) == hipSuccess;
            h_list[k] = x->d_state;
        }
        ok = ok && hipMemcpyAsync(d_list, h_list, sizeof(DecState *) * live.size(), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            launch_decode_run_multi(d_list, (uint32_t)live.size(), st);
            ok = hipGetLastError() == hipSuccess;
        }
        for (size_t k = 0; k < live.size() && ok; k++) {
            DecInstance *x = (DecInstance *)hs[live[k]];
            ok = hipMemcpyAsync(x->h_read, x->d_state, offsetof(DecState, probs), hipMemcpyDeviceToHost, st) == hipSuccess;
        }
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) { dev_rc = CSCMI_DEVICE_ERROR; break; }
        // decoded runs back in one go
        for (int i : live) {
            DecInstance *x = (DecInstance *)hs[i];
            const DecState &r = *x->h_read;
            if (r.status == DEC_DONE && r.out_size)
                ok = ok && hipMemcpyAsync(x->h_out, x->h.out, r.out_size, hipMemcpyDeviceToHost, st) == hipSuccess;
        }
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) { dev_rc = CSCMI_DEVICE_ERROR; break; }
        std::vector<int> next;
        for (int i : live) {
            DecInstance *x = (DecInstance *)hs[i];
            const DecState &r = *x->h_read;
            x->taken[0] = r.taken[0]; x->taken[1] = r.taken[1];
            x->consumed_view = r.consumed + r.rd[0] + r.rd[1];
            bool keep = false;
            switch (r.status) {
            case DEC_DONE:
                if (r.out_size) {                                           // csc_dec.cpp:760-771
                    size_t wrote = oss[i]->Write(oss[i], x->h_out, r.out_size);
                    if (wrote == CSC_WRITE_ABORT) break;
                    if (wrote < r.out_size) { rcs[i] = WRITE_ERROR; break; }
                    keep = true;
                }
                break;
            case DEC_NEED_RC:
            case DEC_NEED_BC:
                if (read_block(x, r.status == DEC_NEED_RC ? 1 : 0) < 0) rcs[i] = r.phase == DEC_PH_PRIME ? -1 : READ_ERROR;
                else keep = true;
                break;
            case DEC_ERR_MINUS1: rcs[i] = -1; break;
            default: rcs[i] = DECODE_ERROR;
            }
            if (keep) next.push_back(i);
        }
        live.swap(next);
    }
    (void)hipFree(d_list);
    (void)hipHostFree(h_list);
    return dev_rc;
}

// Not in the reference: whole streams that lie in device memory decoded into device memory, n at once.  The block reader
// (csc_dec_blocks.h) and the delivery of every run are in the kernel (k_decode_dev*), so a round is: the list of live streams up,
// ONE launch, the small states back -- no payload and no run crosses the bus, and no callback is made.  A launch ends when its
// stream does or after opts->launch_bytes of output (kDevLaunchBytes by default), which bounds kernel time; the host relaunches
// what is still live.  jobs[i].rc / produced / dst are what CSCDec_Create + CSCDec_Decode give over a reader of src and a writer
// that refuses the run which would pass dst_cap (include/csc_mi355x.h).
int CSCMI_DecodeDeviceBatch(int n, CSCMIDevDecode *jobs, const CSCMIDevDecodeOpts *opts, CSCMIDevDecodeStats *stats)
{
    if (stats) { stats->launches = stats->rounds = 0; stats->kernel_ms = 0; }   // (this call zeroes them even where no device is visible)
    return CSCMI_DecodeDeviceBatchStop(n, jobs, NULL, opts, stats);
}

// The same with a stop position per stream (stop_at == NULL, or UINT64_MAX for a stream: none): the writer wants the first
// stop_at[i] bytes and answers CSC_WRITE_ABORT once it has them.  The rule is the kernel's (decode_stream<true>): the run that
// crosses the position is delivered clipped to it, and no run -- nor the end-of-stream signal -- is decoded behind it; a stopped
// stream leaves the live list like one that has ended, so it is not launched again.
int CSCMI_DecodeDeviceBatchStop(int n, CSCMIDevDecode *jobs, const uint64_t *stop_at, const CSCMIDevDecodeOpts *opts,
                                CSCMIDevDecodeStats *stats)
{
    if (n > 0 && CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;           // nothing of the caller's is touched
    if (stats) { stats->launches = stats->rounds = 0; stats->kernel_ms = 0; }
    if (n <= 0) return 0;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return CSCMI_DEVICE_ERROR;
    uint64_t budget64 = opts && opts->launch_bytes ? opts->launch_bytes : kDevLaunchBytes;
    const uint32_t launch_budget = budget64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)budget64;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) (void)hipEventDestroy(ev[0]);
        return CSCMI_DEVICE_ERROR;
    }
    for (int i = 0; i < n; i++) { jobs[i].produced = 0; jobs[i].consumed = 0; jobs[i].rc = CSCMI_DEVICE_ERROR; }
    struct Slot { int job; DecRes *res; DecState *d_state, *h_read; };
    int dev_rc = 0, next = 0;
    while (next < n && !dev_rc) {
        // a group: as many of the remaining jobs as the free device memory (and what the resource cache holds) can carry
        std::vector<Slot> grp;
        size_t free_b = 0, total_b = 0, used = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { dev_rc = CSCMI_DEVICE_ERROR; break; }
        const size_t room = (free_b + dec_cache_bytes()) / 8 * 7;
        hipStream_t st = nullptr;
        for (; next < n && grp.size() < kDevGroupMax && !dev_rc; next++) {
            CSCMIDevDecode &job = jobs[next];
            // where CSCDec_Create refuses before it reads (an empty source is its first read failing)
            if (!dec_props_ok(&job.props) || job.src_size == 0 || job.src == NULL) { job.rc = CSCMI_NO_DECODER; continue; }
            DecState h;
            memset(&h, 0, sizeof(h));
            const DecLayout l = dec_layout(&job.props, h);
            if (!grp.empty() && used + l.dsize > room) break;
            DecRes *r = dec_res_get(device, l.dsize, l.hsize);
            if (!r) {
                if (!grp.empty()) break;                     // this group first; the job is tried again with its memory back
                fprintf(stderr, "csc-mi355x: decoder device allocation failed\n");
                continue;                                      // (rc stays CSCMI_DEVICE_ERROR; the other jobs proceed)
            }
            used += l.dsize;
            if (!st) st = r->stream;
            uint8_t *D = r->dslab;
            dec_place(h, D, l);
            h.src = (const uint8_t *)job.src; h.src_size = job.src_size; h.src_pos = 0;
            h.dst = (uint8_t *)job.dst; h.dst_cap = job.dst_cap; h.produced = 0;
            h.stop_at = stop_at ? stop_at[next] : UINT64_MAX;
            h.launch_budget = launch_budget;
            Slot s = {next, r, (DecState *)(D + l.o_state), (DecState *)(r->hslab + l.p_read)};
            *s.h_read = h;                                     // (pinned: the upload below reads it when the stream gets there)
            bool ok = hipMemsetAsync(D, 0, l.dsize, st) == hipSuccess
                   && hipMemcpyAsync(D + l.o_words, kWords, sizeof(kWords), hipMemcpyHostToDevice, st) == hipSuccess
                   && hipMemcpyAsync(s.d_state, s.h_read, sizeof(DecState), hipMemcpyHostToDevice, st) == hipSuccess;
            if (ok) { launch_decode_init(s.d_state, st); ok = hipGetLastError() == hipSuccess; }
            grp.push_back(s);
            if (!ok) dev_rc = CSCMI_DEVICE_ERROR;
        }
        DecState **d_list = nullptr, **h_list = nullptr;
        std::vector<size_t> live;
        for (size_t k = 0; k < grp.size(); k++) live.push_back(k);
        if (!grp.empty() && !dev_rc) {
            if (hipMalloc((void **)&d_list, sizeof(DecState *) * grp.size()) != hipSuccess
                || hipHostMalloc((void **)&h_list, sizeof(DecState *) * grp.size(), hipHostMallocDefault) != hipSuccess) dev_rc = CSCMI_DEVICE_ERROR;
        }
        while (!live.empty() && !dev_rc) {
            for (size_t k = 0; k < live.size(); k++) h_list[k] = grp[live[k]].d_state;
            bool ok = hipMemcpyAsync(d_list, h_list, sizeof(DecState *) * live.size(), hipMemcpyHostToDevice, st) == hipSuccess
                   && hipEventRecord(ev[0], st) == hipSuccess;
            if (ok) {
                launch_decode_dev(d_list, h_list[0], (uint32_t)live.size(), st);
                ok = hipGetLastError() == hipSuccess && hipEventRecord(ev[1], st) == hipSuccess;
            }
            for (size_t k = 0; k < live.size() && ok; k++) {
                const Slot &s = grp[live[k]];
                ok = hipMemcpyAsync(s.h_read, s.d_state, offsetof(DecState, probs), hipMemcpyDeviceToHost, st) == hipSuccess;
            }
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            float ms = 0;
            ok = ok && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess;
            if (!ok) { dev_rc = CSCMI_DEVICE_ERROR; break; }
            if (stats) { stats->launches++; stats->rounds++; stats->kernel_ms += ms; }
#ifdef CSCMI_TIMERS
            fprintf(stderr, "csc-mi355x: decode launch: %zu streams, %.3f ms\n", live.size(), ms);      // (development build only)
#endif
            std::vector<size_t> keep;
            for (size_t k : live) {
                const Slot &s = grp[k];
                const DecState &r = *s.h_read;
                CSCMIDevDecode &job = jobs[s.job];
                job.produced = (size_t)r.produced;
                job.consumed = (size_t)r.src_pos;
                switch (r.status) {
                case DEC_DONE: keep.push_back(k); break;                  // the launch budget: more to come
                case DEC_END: job.rc = 0; break;
                case DEC_STOPPED: job.rc = 0; break;                      // the caller has the bytes it asked for
                case DEC_ERR_MINUS1: job.rc = -1; break;
                case DEC_ERR_READ: job.rc = READ_ERROR; break;
                case DEC_ERR_WRITE: job.rc = WRITE_ERROR; break;
                case DEC_NO_DECODER: job.rc = CSCMI_NO_DECODER; break;
                default: job.rc = DECODE_ERROR;
                }
            }
            live.swap(keep);
        }
        if (st) (void)hipStreamSynchronize(st);
        if (d_list) (void)hipFree(d_list);
        if (h_list) (void)hipHostFree(h_list);
        for (const Slot &s : grp) dec_res_put(s.res);
    }
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return dev_rc;
}

}  // extern "C"
