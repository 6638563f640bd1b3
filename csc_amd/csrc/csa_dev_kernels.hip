// csa_dev_kernels.hip -- the three kernels of the device-resident archive read (CSAMI_DeviceRead, csa_archive.cpp): per wave of
// tasks one launch of each, whatever the number of tasks and fragments.  All three are bandwidth-bound: a byte is loaded once and
// stored at most once, in 16-byte accesses wherever the two ends allow it (csa_dev_read.h: copy_sum).
//
//   k_gather_extents      one workgroup per <= 64 KiB piece of an archive block: the blocks of a task, which interleave with other
//                         tasks' in an archive written by several workers (AsyncArchiveReader, csa_io.h:466-542), go back to back
//                         into the task's gathered stream; the 10 property bytes of every task go to the wave's property table
//   k_frag_pieces<STORE>  one workgroup per <= 16 KiB piece of a fragment: adler32's A and B over it, and with STORE the bytes to
//                         their place in the caller's buffer in the same pass (AsyncFileWriter, csa_io.h:274-408)
//   k_frag_fold           one lane per fragment: its pieces folded in order and compared with the index's checksum
//
// Every address in the tables was validated by the host before the launch; a workgroup touches src[0, len) and dst[0, len) of its
// piece and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csa_dev_read.h"

using namespace csadev;

__global__ __launch_bounds__(kThreads) void k_gather_extents(const CopyPiece *pieces, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const CopyPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    copy_sum<true, false>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
}

template <bool STORE>
__global__ __launch_bounds__(kThreads) void k_frag_pieces(const CopyPiece *pieces, PieceSums *out, uint32_t npieces)
{
    if (blockIdx.x >= npieces) return;
    const CopyPiece pc = pieces[blockIdx.x];
    uint64_t a = 0, b = 0;
    copy_sum<STORE, true>(pc.dst, pc.src, pc.len, threadIdx.x, kThreads, a, b);
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
        out[blockIdx.x] = s;
    }
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

void launch_frag_fold(const void *frags, const void *sums, void *out, uint32_t nfrags, hipStream_t st)
{
    hipLaunchKernelGGL(k_frag_fold, dim3(nfrags ? (nfrags + kThreads - 1) / kThreads : 1), dim3(kThreads), 0, st,
                       (const FragFold *)frags, (const PieceSums *)sums, (FragResult *)out, nfrags);
}
