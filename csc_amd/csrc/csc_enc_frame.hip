// csc_enc_frame.hip -- k_frame_blocks: the coder blocks a round of encode kernels left in the streams' arenas, framed into the
// callers' device destinations (CSCMI_EncodeDeviceBatch, csc_host.cpp).  What write_arena / write_block do on the host over
// Write callbacks, without the arena crossing the bus: one 256-thread workgroup per stream; one lane walks the dependent chain of
// records (frame_walk, csc_enc_frame.h -- each offset needs the previous size) kFrameBatch at a time into an LDS table and
// applies the dst_cap rule while it walks, so the table ends at the refused Write; the whole workgroup then copies the batch:
// 16-byte loads from the arena, 16-byte stores shifted into place, byte stores for a payload's head and tail and for the header.
#include <hip/hip_runtime.h>

#include "csc_device.h"
#include "csc_enc_frame.h"

namespace cscmi {

constexpr uint32_t kFrameThreads = 256;

__global__ __launch_bounds__(kFrameThreads) void k_frame_blocks(const FrameItem *items, FrameJob *jobs, FrameStatus *status)
{
    __shared__ FrameRec tab[kFrameBatch];
    __shared__ FrameCursor cur;
    __shared__ uint32_t cnt;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const EncState *S = items[b].state;
    FrameJob *J = jobs + items[b].job;
    // (every thread reads the same words: the branches below are uniform)
    const int32_t rc0 = J->rc;
    const uint32_t err = S->error, used = S->arena_used, bsize = S->bsize;
    const uint64_t cap = J->dst_cap;
    uint8_t *const dst = J->dst;
    const uint8_t *const arena = S->arena;
    if (rc0 != 0 || err != ERR_NONE) {              // a stream that has ended is skipped; a kernel error ends it here
        if (tid == 0) {
            if (rc0 == 0) J->rc = kFrameDeviceError;
            FrameStatus s = {rc0 != 0 ? 0u : err, rc0 != 0 ? rc0 : kFrameDeviceError, J->produced};
            status[b] = s;
        }
        return;
    }
    if (tid == 0) { cur.arena_pos = 0; cur.error = 0; cur.produced = J->produced; cur.rc = 0; }
    for (;;) {
        __syncthreads();                            // the table's readers of the last batch are done; `cur` is set
        if (tid == 0)
            cnt = frame_walk([&](uint32_t off) { return *(const uint32_t *)(arena + off); }, used, bsize, cap, &cur, kFrameBatch,
                             [&](uint32_t i, const FrameRec &r) { tab[i] = r; });
        __syncthreads();
        const uint32_t n = cnt;
        for (uint32_t r = 0; r < n; r++) {
            const FrameRec rec = tab[r];
            if (tid == 32) frame_put_header(dst, rec);
            if (rec.size) frame_copy(dst + rec.dst_off + rec.hdr, arena + rec.arena_off, rec.size, tid, kFrameThreads);
        }
        if (n < kFrameBatch) break;
    }
    if (tid == 0) {                                 // (its own LDS writes; every other thread is past the last barrier)
        const int32_t rc = cur.error ? kFrameDeviceError : cur.rc;
        J->produced = cur.produced;
        J->rc = rc;
        FrameStatus s = {cur.error, rc, cur.produced};
        status[b] = s;
    }
}

void launch_frame_blocks(const FrameItem *items, FrameJob *jobs, FrameStatus *status, uint32_t nstreams, hipStream_t st)
{
    if (!nstreams) return;
    hipLaunchKernelGGL(k_frame_blocks, dim3(nstreams), dim3(kFrameThreads), 0, st, items, jobs, status);
}

}  // namespace cscmi
