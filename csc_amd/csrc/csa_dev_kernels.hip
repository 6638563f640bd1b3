// csa_dev_kernels.hip -- the three kernels of the device-resident archive read (CSAMI_DeviceRead, csa_dev_archive.cpp): per wave
// of tasks one launch of each, whatever the number of tasks and fragments.  All three are bandwidth-bound: a byte is loaded once and
// stored at most once, in 16-byte accesses wherever the two ends allow it (csa_dev_read.h: copy_sum).  The device-resident write
// (CSAMI_DeviceWrite) runs the same three the other way round -- fragments gathered and summed, streams placed -- and one more.
// k_frag_pieces<false> is also the adler32 of CSA_Add's fragments and of CSAMI_Adler32Device (csa_archive.cpp):
//
//   k_gather_extents      one workgroup per <= 64 KiB piece of an archive block: the blocks of a task, which interleave with other
//                         tasks' in an archive written by several workers (AsyncArchiveReader, csa_io.h:466-542), go back to back
//                         into the task's gathered stream; the 10 property bytes of every task go to the wave's property table
//   k_frag_pieces<STORE>  one workgroup per <= 16 KiB piece of a fragment: adler32's A and B over it, and with STORE the bytes to
//                         their place in the caller's buffer in the same pass (AsyncFileWriter, csa_io.h:274-408)
//                         (a piece without a destination -- an entry CSAMI_DeviceReadInto only verifies -- is summed and not stored)
//   k_frag_fold           one lane per fragment: its pieces folded in order and compared with the index's checksum
//   k_frag_compare        k_frag_pieces<true> for CSAMI_DeviceCompare: the piece against the caller's bytes instead of onto them --
//                         two loads in the place of a load and a store -- and the first differing index beside the sums
//   k_frag_fold_diff      k_frag_fold, and the fragment's first differing offset from its pieces'
//   k_frag_slices         k_frag_pieces<true> for CSAMI_DeviceReadSlices: a piece is still summed whole, and the bytes of it that its
//                         entry's slice selects -- all, none, or the runs of a periodic pattern -- go to their packed places
//   k_frag_rows           k_frag_pieces<true> for CSAMI_DeviceWriteSlices, the transpose of k_frag_slices: a piece's destination is
//                         contiguous and its source is the runs of a periodic pattern in the caller's buffer (or one range of it);
//                         without a destination it is the sum-only pass of CSAMI_DeviceUpdate's check
//   k_frag_spread         k_frag_pieces<true> for CSAMI_DeviceReadIntoSlices, the transpose of k_frag_rows: a piece's source is contiguous
//                         and its destination is the runs of a periodic pattern in the caller's buffer (or one range of it, or none)
//   k_frag_compare_rows   k_frag_compare for CSAMI_DeviceCompareSlices: the piece against such rows instead of one range
//   k_block_table         one lane per task stream of a wave (write only): the archive-block table AsyncWriter would have made of
//                         the encoder's Write calls (csa_io.h:145-201), read off the stream's framing (csa_dev_write.h)
//   k_digest_leaves       one LANE per <= 16 KiB leaf of a fragment: its BLAKE2s tree-mode leaf digest (csa_dev_digest.h) -- a leaf is a
//                         serial chain of up to 256 compressions, so the parallelism is across leaves
//   k_digest_roots        one lane per fragment: the root over its leaves' digests, stored to the digest table and compared with an
//                         expected table where one is given; one word a fragment is all the host reads back
//   k_move_extents        one workgroup per <= 32 KiB chunk of a move INSIDE the archive buffer (CSAMI_DeviceUpdateInPlace): memmove for a
//                         whole move list in one launch -- a chunk into registers, a flag, a wait for the chunks whose sources its
//                         destination meets, the stores (csa_dev_move.h)
//
// Every address in the tables was validated by the host before the launch; a workgroup touches src[0, len) and dst[0, len) of its
// piece and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csa_dev_read.h"
#include "csa_dev_write.h"
#include "csa_dev_digest.h"
#include "csa_dev_move.h"

using namespace csadev;

__global__ __launch_bounds__(kThreads) void k_gather_extents(const CopyPiece *pieces, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const CopyPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    copy_sum<true, false>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
}

// the workgroup's a and b added up and stored as its piece's sums
__device__ inline void store_sums(uint64_t a, uint64_t b, PieceSums *out)
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    __shared__ uint64_t red[2 * (kThreads / 64)];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        PieceSums s = {0, 0};
        for (uint32_t w = 0; w < kThreads / 64; w++) { s.a += red[2 * w]; s.b += red[2 * w + 1]; }
        *out = s;
    }
}

template <bool STORE>
__global__ __launch_bounds__(kThreads) void k_frag_pieces(const CopyPiece *pieces, PieceSums *out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const CopyPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    if (STORE && pc.dst == nullptr) copy_sum<false, true>(nullptr, pc.src, pc.len, threadIdx.x, kThreads, a, b);   // (the same for the whole workgroup)
    else copy_sum<STORE, true>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    store_sums(a, b, out + blockIdx.x);
}

// the workgroup's a and b added up, and its smallest differing index, stored as its piece's (len: the piece's, where no thread saw one)
__device__ inline void store_sums_first(uint64_t a, uint64_t b, uint32_t first, uint32_t len, PieceSums *out, uint32_t *first_out)
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        const uint32_t f = __shfl_down(first, off, 64);
        first = f < first ? f : first;
    }
    __shared__ uint64_t red[2 * (kThreads / 64)];
    __shared__ uint32_t redf[kThreads / 64];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; redf[wave] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        PieceSums s = {0, 0};
        uint32_t f = len;
        for (uint32_t w = 0; w < kThreads / 64; w++) { s.a += red[2 * w]; s.b += red[2 * w + 1]; f = redf[w] < f ? redf[w] : f; }
        *out = s;
        *first_out = f;
    }
}

// k_frag_pieces<true> with two loads in the place of a load and a store: the piece's first `cmp` bytes against the caller's
// (compare_piece, csa_dev_read.h), and the smallest differing index of the workgroup reduced the way the sums are
__global__ __launch_bounds__(kThreads) void k_frag_compare(const CopyPiece *pieces, PieceSums *out, uint32_t *first_out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const CopyPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    uint32_t first;
    compare_piece(pc.src, pc.dst, pc.len, pc.dst ? pc.cmp : 0u, threadIdx.x, kThreads, a, b, first);
    store_sums_first(a, b, first, pc.len, out + blockIdx.x, first_out + blockIdx.x);
}

// k_frag_pieces<true> for CSAMI_DeviceReadSlices: a piece that lies inside one run of its entry's slice, or holds no selected byte, is
// copy_sum's as there; any other is summed whole and stored in part (slice_sum, csa_dev_read.h).  Which of the three: the same for
// the whole workgroup.
__global__ __launch_bounds__(kThreads) void k_frag_slices(const SlicePiece *pieces, PieceSums *out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const SlicePiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    if (pc.stride) slice_sum(pc, threadIdx.x, kThreads, a, b);
    else if (pc.dst == nullptr) copy_sum<false, true>(nullptr, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    else copy_sum<true, true>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    store_sums(a, b, out + blockIdx.x);
}

// k_frag_pieces<true> for CSAMI_DeviceWriteSlices: a piece whose packed bytes lie inside one run of its entry's slice is copy_sum's
// as there; any other is gathered across the run borders (gather_sum, csa_dev_write.h).  A piece without a destination
// (CSAMI_DeviceUpdate's check against the base's checksums) is summed and not stored, as in k_frag_pieces<true>.  Which of the four:
// the same for the whole workgroup.
__global__ __launch_bounds__(kThreads) void k_frag_rows(const GatherPiece *pieces, PieceSums *out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const GatherPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    if (pc.dst == nullptr) {
        if (pc.stride) gather_sum<kGPlantNone, false>(pc, threadIdx.x, kThreads, a, b);
        else copy_sum<false, true>(nullptr, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    } else if (pc.stride) gather_sum(pc, threadIdx.x, kThreads, a, b);
    else copy_sum<true, true>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    store_sums(a, b, out + blockIdx.x);
}

// k_frag_pieces<true> for CSAMI_DeviceReadIntoSlices: a piece whose packed bytes go to one range of the caller's buffer, or to none, is
// copy_sum's as there; any other is spread across the run borders (spread_sum, csa_dev_read.h).  Which of the three: the same for
// the whole workgroup.
__global__ __launch_bounds__(kThreads) void k_frag_spread(const SpreadPiece *pieces, PieceSums *out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const SpreadPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    if (pc.stride) spread_sum(pc, threadIdx.x, kThreads, a, b);
    else if (pc.dst == nullptr) copy_sum<false, true>(nullptr, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    else copy_sum<true, true>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
    store_sums(a, b, out + blockIdx.x);
}

// k_frag_compare for CSAMI_DeviceCompareSlices: a piece whose compared bytes lie in one range of the caller's buffer, or that is
// summed only, is compare_piece's as there; any other is compared across the run borders (compare_rows, csa_dev_read.h).
__global__ __launch_bounds__(kThreads) void k_frag_compare_rows(const SpreadPiece *pieces, PieceSums *out, uint32_t *first_out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const SpreadPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    uint32_t first;
    if (pc.stride) compare_rows(pc, threadIdx.x, kThreads, a, b, first);
    else compare_piece(pc.src, pc.dst, pc.len, pc.dst ? pc.cmp : 0u, threadIdx.x, kThreads, a, b, first);
    store_sums_first(a, b, first, pc.len, out + blockIdx.x, first_out + blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void k_frag_fold(const FragFold *frags, const PieceSums *sums, FragResult *out, uint32_t nfrags)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nfrags) return;
    const FragFold f = frags[i];
    const PieceSums *s = sums + f.first;
    FragResult r;
    r.adler = fold_pieces([s](uint32_t k) { return s[k]; }, f.npieces, f.size);
    r.ok = r.adler == f.checksum ? 1u : 0u;
    out[i] = r;
}

__global__ __launch_bounds__(kThreads) void k_frag_fold_diff(const FragFold *frags, const PieceSums *sums, const uint32_t *firsts, FragDiff *out,
                                                             uint32_t nfrags)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nfrags) return;
    const FragFold f = frags[i];
    const PieceSums *s = sums + f.first;
    const uint32_t *d = firsts + f.first;
    FragDiff r;
    r.adler = fold_pieces([s](uint32_t k) { return s[k]; }, f.npieces, f.size);
    r.ok = r.adler == f.checksum ? 1u : 0u;
    r.first = fold_first([d](uint32_t k) { return d[k]; }, f.npieces, f.size);
    out[i] = r;
}

// A launch is made even for an empty table (one workgroup that returns at once), so that a wave is always the same three launches.
void launch_gather_extents(const void *pieces, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_gather_extents, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const CopyPiece *)pieces, npieces);
}

void launch_frag_pieces(const void *pieces, void *sums, uint32_t npieces, bool store, hipStream_t st)
{
    if (store) hipLaunchKernelGGL(k_frag_pieces<true>, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const CopyPiece *)pieces, (PieceSums *)sums, npieces);
    else hipLaunchKernelGGL(k_frag_pieces<false>, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const CopyPiece *)pieces, (PieceSums *)sums, npieces);
}

void launch_frag_compare(const void *pieces, void *sums, void *firsts, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_compare, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const CopyPiece *)pieces, (PieceSums *)sums, (uint32_t *)firsts, npieces);
}

void launch_frag_slices(const void *pieces, void *sums, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_slices, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const SlicePiece *)pieces, (PieceSums *)sums, npieces);
}

void launch_frag_rows(const void *pieces, void *sums, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_rows, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const GatherPiece *)pieces, (PieceSums *)sums, npieces);
}

void launch_frag_spread(const void *pieces, void *sums, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_spread, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const SpreadPiece *)pieces, (PieceSums *)sums, npieces);
}

void launch_frag_compare_rows(const void *pieces, void *sums, void *firsts, uint32_t npieces, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_compare_rows, dim3(npieces ? npieces : 1), dim3(kThreads), 0, st, (const SpreadPiece *)pieces, (PieceSums *)sums, (uint32_t *)firsts, npieces);
}

void launch_frag_fold(const void *frags, const void *sums, void *out, uint32_t nfrags, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_fold, dim3(nfrags ? (nfrags + kThreads - 1) / kThreads : 1), dim3(kThreads), 0, st,
                       (const FragFold *)frags, (const PieceSums *)sums, (FragResult *)out, nfrags);
}

void launch_frag_fold_diff(const void *frags, const void *sums, const void *firsts, void *out, uint32_t nfrags, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_fold_diff, dim3(nfrags ? (nfrags + kThreads - 1) / kThreads : 1), dim3(kThreads), 0, st,
                       (const FragFold *)frags, (const PieceSums *)sums, (const uint32_t *)firsts, (FragDiff *)out, nfrags);
}

// One workgroup for the wave: lane t walks tasks t, t + 256, ... -- a step is one coder block, a few dependent byte loads, so the
// longest stream sets the time whatever the width -- into its own slots of `scratch`; then the tables go back to back, in task
// order, into `sizes`, so that the host reads back the blocks there are and not the slots there might have been.
__global__ __launch_bounds__(kTableThreads) void k_block_table(const BlockTableJob *jobs, uint32_t njobs, uint64_t *scratch,
                                                               BlockTableRes *res, uint64_t *sizes)
{
    __shared__ uint32_t start[kTableMaxJobs];
    for (uint32_t k = threadIdx.x; k < njobs; k += kTableThreads) {
        const BlockTableJob j = jobs[k];
        const uint8_t *s = j.stream;
        uint64_t *out = scratch + j.first;
        BlockTableRes r;
        r.status = block_table([s](uint64_t i) { return (uint32_t)s[i]; }, j.produced, j.bsize, j.max_blocks,
                               [out](uint32_t i, uint64_t size) { out[i] = size; }, &r.nblocks);
        res[k] = r;
        start[k] = r.nblocks < j.max_blocks ? r.nblocks : j.max_blocks;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < njobs; k++) { const uint32_t n = start[k]; start[k] = at; at += n; }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < njobs; k += kTableThreads) {
        const BlockTableJob j = jobs[k];
        const uint32_t nb = res[k].nblocks < j.max_blocks ? res[k].nblocks : j.max_blocks;
        for (uint32_t i = 0; i < nb; i++) sizes[start[k] + i] = scratch[j.first + i];
    }
}

void launch_block_table(const void *jobs, uint32_t njobs, void *scratch, void *res, void *sizes, hipStream_t st)
{
    hipLaunchKernelGGL(k_block_table, dim3(1), dim3(kTableThreads), 0, st, (const BlockTableJob *)jobs, njobs, (uint64_t *)scratch,
                       (BlockTableRes *)res, (uint64_t *)sizes);
}

// One lane per leaf.  The chaining value, one message block and the working vector live in registers (no scratch); a lane loads
// its own 64-byte blocks, 16 KiB from its neighbours'.
__global__ __launch_bounds__(kDigestThreads) void k_digest_leaves(const DigestLeaf *leaves, DigestWords *out, uint32_t nleaves)
{
    const uint32_t i = blockIdx.x * kDigestThreads + threadIdx.x;
    if (i >= nleaves) return;
    const DigestLeaf lf = leaves[i];
    DigestWords d;
    digest_leaf(lf, d);
    out[i] = d;
}

__global__ __launch_bounds__(kDigestThreads) void k_digest_roots(const DigestFrag *frags, const DigestWords *leaves, uint8_t *out, const uint8_t *expect,
                                                                 uint32_t *differs, uint32_t nfrags)
{
    const uint32_t i = blockIdx.x * kDigestThreads + threadIdx.x;
    if (i >= nfrags) return;
    differs[i] = digest_root(frags[i], leaves, out, expect);
}

void launch_digest_leaves(const void *leaves, void *out, uint32_t nleaves, hipStream_t st)
{
    hipLaunchKernelGGL(k_digest_leaves, dim3(nleaves ? (nleaves + kDigestThreads - 1) / kDigestThreads : 1), dim3(kDigestThreads), 0, st,
                       (const DigestLeaf *)leaves, (DigestWords *)out, nleaves);
}

void launch_digest_roots(const void *frags, const void *leaves, void *out, const void *expect, void *differs, uint32_t nfrags, hipStream_t st)
{
    hipLaunchKernelGGL(k_digest_roots, dim3(nfrags ? (nfrags + kDigestThreads - 1) / kDigestThreads : 1), dim3(kDigestThreads), 0, st,
                       (const DigestFrag *)frags, (const DigestWords *)leaves, (uint8_t *)out, (const uint8_t *)expect, (uint32_t *)differs, nfrags);
}

// memmove for a move list (csa_dev_move.h: the plan, the order, the thread's loads and stores).  `state` is one block the launcher
// zeroes: the ticket counter, the error word, two words of padding, then one flag a chunk.
//
// A workgroup draws its ticket with one atomic add when it starts, and the ticket -- not blockIdx -- selects its chunk.  It loads
// the whole chunk into registers, every wave waits for its loads, and behind the barrier one lane sets the chunk's flag: a global,
// agent-scope atomic store.  What crosses workgroups is that flag alone, and what it orders is a write after a read: no byte one
// workgroup stores is loaded by another in this launch (a load window may hold such bytes; the funnel shift drops them), so there
// is no payload to release or acquire.  Then the lanes of the first wave poll the flags lo..hi of its chunk, lane-strided, relaxed
// and agent-scope, with s_sleep between sweeps; behind a second barrier the workgroup stores.
//
// Progress, whatever the residency: a workgroup waits only for tickets LOWER than its own.  A lower ticket was drawn by a workgroup
// that had started before this one drew its own, so it is running, and between its start and its flag there is no wait at all:
// the flag store needs nothing from anyone.  So every flag a workgroup polls is set after a bounded time, whether one workgroup is
// resident or all of them.  Nothing here waits for a higher ticket, there is no grid barrier and no cooperative launch.
//
// Every spin is bounded all the same: at kMoveSpins sweeps the workgroup sets the error word (its ticket + 1) and leaves without
// storing.  The host reads the word back and returns CSCMI_DEVICE_ERROR: a mistake in the plan fails a test and holds no card.
constexpr uint32_t kMoveSpins = 1u << 22;       // sweeps of >= 512 clocks each: about a second, a million times what a flag takes

__global__ __launch_bounds__(kThreads) void k_move_extents(const MoveChunk *chunks, uint32_t nchunks, uint8_t *buf, uint64_t cap, uint32_t *state)
{
    __shared__ uint32_t s_ticket, s_go;
    if (threadIdx.x == 0) s_ticket = __hip_atomic_fetch_add(state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t ticket = s_ticket;
    if (ticket >= nchunks) return;                                       // (the same for the whole workgroup)
    const MoveChunk c = chunks[ticket];
    uint32_t *flags = state + kMoveStateWords;
    MoveRegs r;
    move_load(c, buf, buf, buf + cap, threadIdx.x, kThreads, r);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flags + ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < 64) {
        bool go = true;
        if (c.lo != kMoveNone) {
            for (uint32_t spins = 0;; spins++) {
                bool set = true;
                for (uint32_t j = c.lo + threadIdx.x; j <= c.hi; j += 64)
                    set = set && __hip_atomic_load(flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (__all(set)) break;
                if (spins >= kMoveSpins) { go = false; break; }          // (uniform: __all's result and the counter are)
                __builtin_amdgcn_s_sleep(8);
            }
        }
        if (threadIdx.x == 0) {
            s_go = go;
            if (!go) __hip_atomic_store(state + 1, ticket + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (!s_go) return;
    move_store(c, buf, threadIdx.x, kThreads, r);
}

// the state block zeroed, then the launch: one workgroup a chunk
void launch_move_extents(const void *chunks, uint32_t nchunks, void *buf, uint64_t cap, void *state, size_t state_bytes, hipStream_t st)
{
    (void)hipMemsetAsync(state, 0, state_bytes, st);
    hipLaunchKernelGGL(k_move_extents, dim3(nchunks ? nchunks : 1), dim3(kThreads), 0, st, (const MoveChunk *)chunks, nchunks, (uint8_t *)buf, cap,
                       (uint32_t *)state);
}
