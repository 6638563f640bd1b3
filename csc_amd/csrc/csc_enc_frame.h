// csc_enc_frame.h -- the block framing of a libcsc stream on the way OUT, MemIO::WriteBlock (csc_memio.cpp:83-108) restated
// over a byte range with a capacity instead of an ISeqOutStream.  Compiles for the host (plain C++:
// tests/test_encode_device_host.py runs tests/model/enc_frame_model.cpp with g++) and for the device (k_frame_blocks,
// csc_enc_frame.hip); csc_host.cpp's write_block / write_arena is the same walk over Write callbacks.
//
// The encode kernels leave a chunk's finished coder blocks in the stream's arena as (ArenaRec, payload padded to 16)*, in the
// order they were finished.  A block becomes two or three Write calls:
//   flag byte: bit 7 = kind (1 range-coder block, 0 bit-coder block), bit 6 = "payload is exactly csc_blocksize bytes";
//   without bit 6 the payload size, 3 bytes big-endian; then the payload, unless it is empty.
// The cap rule: a Write is all or nothing; the first one that would take the total past dst_cap ends the stream with
// WRITE_ERROR and nothing after it is written -- not even a later, smaller Write that would fit (csc_coder.cpp:60-62,99-100
// throw at the first short WriteBlock).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSCMI_FHD __host__ __device__ inline
#else
#define CSCMI_FHD inline
#endif

namespace cscmi {

constexpr uint32_t kFrameBatch = 64;            // records the walk hands to the copy at a time (the kernel's LDS table)
constexpr int32_t kFrameWriteError = -97;       // WRITE_ERROR, csc_common.h:14
constexpr int32_t kFrameDeviceError = -95;      // CSCMI_DEVICE_ERROR, include/csc_mi355x.h
constexpr uint32_t kFrameErrArena = 0x4652;     // FrameCursor::error: a record that does not lie inside arena_used (never written by the encode kernels)

// What CSCMI_EncodeDeviceBatch keeps on the device for a group of jobs (csc_host.cpp), and what k_frame_blocks gets and gives:
struct EncState;
struct FrameJob {          // one per job, persists across the rounds of the call
    uint8_t *dst;
    uint64_t dst_cap;
    uint64_t produced;     // bytes framed so far
    int32_t rc;            // 0 while the stream lives; WRITE_ERROR / CSCMI_DEVICE_ERROR end it
    uint32_t pad;
};
struct FrameItem {         // one per workgroup of a launch: the stream and its job record
    const EncState *state;
    uint32_t job, pad;
};
struct FrameStatus {       // one per workgroup of a launch: ALL the host reads back of a round (16 bytes a stream)
    uint32_t error;        // EncState::error of the round's encode kernel, or kFrameErrArena
    int32_t rc;
    uint64_t produced;
};

// one block of a batch: where its payload lies in the arena, where its header goes in dst, and what of it fits
struct FrameRec {
    uint32_t arena_off;    // the payload's first byte in the arena (a multiple of 16)
    uint32_t size;         // payload bytes to copy: the block's, or 0 where the payload is empty or was refused
    uint32_t hdr;          // header bytes to store at dst_off: 1 (flag), 4 (flag + size); the payload goes behind them
    uint32_t hdr_bytes;    // the header, first byte in bits 0-7
    uint64_t dst_off;
};

struct FrameCursor {
    uint32_t arena_pos;    // next record
    uint32_t error;        // 0 or kFrameErrArena
    uint64_t produced;     // bytes of all Write calls accepted so far
    int32_t rc;            // 0, or WRITE_ERROR once a Write was refused
};

// Walk up to `max` records from c->arena_pos on.  ld(off) returns the 32-bit word at arena offset `off` (a multiple of 4, below
// arena_used); put(i, rec) stores table entry i.  Returns the entries made; fewer than `max` means the arena is consumed or the
// walk has ended (c->rc / c->error).  An entry is made for every block of which at least the flag byte fits.
template <class Load, class Put>
CSCMI_FHD uint32_t frame_walk(Load ld, uint32_t arena_used, uint32_t bsize, uint64_t dst_cap, FrameCursor *c, uint32_t max, Put put)
{
    uint32_t n = 0;
    while (n < max && c->rc == 0 && c->error == 0 && c->arena_pos < arena_used) {
        const uint32_t off = c->arena_pos;
        if (arena_used - off < 16) { c->error = kFrameErrArena; break; }
        const uint32_t kind = ld(off) & 1u, size = ld(off + 4);
        if (size > 0xFFFFFFu || arena_used - off - 16 < ((size + 15) & ~15u)) { c->error = kFrameErrArena; break; }
        if (c->produced + 1 > dst_cap) { c->rc = kFrameWriteError; break; }          // Write 1: the flag byte
        FrameRec r;
        r.arena_off = off + 16; r.size = 0; r.hdr = 1; r.dst_off = c->produced;
        r.hdr_bytes = (kind << 7) | (size == bsize ? 0x40u : 0u);
        c->produced += 1;
        if (size != bsize) {                                                          // Write 2: the size
            if (c->produced + 3 > dst_cap) c->rc = kFrameWriteError;
            else {
                r.hdr = 4;
                r.hdr_bytes |= ((size >> 16) & 0xFFu) << 8 | ((size >> 8) & 0xFFu) << 16 | (size & 0xFFu) << 24;
                c->produced += 3;
            }
        }
        if (c->rc == 0 && size) {                                                     // Write 3: the payload
            if (c->produced + size > dst_cap) c->rc = kFrameWriteError;
            else { r.size = size; c->produced += size; }
        }
        put(n, r);
        n++;
        c->arena_pos = off + 16 + ((size + 15) & ~15u);
    }
    return n;
}

struct alignas(16) FrameVec { uint32_t w[4]; };

// Thread `tid` of `nthreads`: its share of copying src[0, n) to dst[0, n).  src is 16-byte aligned and readable up to n rounded
// up to 16; dst has any alignment.  Up to 15 head bytes bring dst to a 16-byte line and up to 15 tail bytes end the payload: those
// are byte stores.  Everything between is 16-byte stores of source words shifted into place.  Nothing outside dst[0, n) is stored.
CSCMI_FHD void frame_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t tid, uint32_t nthreads)
{
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = (n - head) & 15u;
    if (tid < head) dst[tid] = src[tid];
    // (the tail from the far end of the workgroup: the head's lanes are busy)
    if (nthreads - 1 - tid < tail) { const uint32_t k = head + 16 * units + (nthreads - 1 - tid); dst[k] = src[k]; }
    const FrameVec *s16 = (const FrameVec *)src;
    FrameVec *d16 = (FrameVec *)(dst + head);
    const uint32_t sw = head >> 2, sb = 8 * (head & 3u);      // unit i is source bytes [16 i + head, 16 i + head + 16)
    for (uint32_t i = tid; i < units; i += nthreads) {
        const FrameVec a = s16[i];
        FrameVec o = a;
        if (head) {                                            // (unit i full and head > 0: vector i + 1 begins inside the payload)
            const FrameVec b = s16[i + 1];
            const uint32_t t0 = (sw & 2u) ? a.w[2] : a.w[0], t1 = (sw & 2u) ? a.w[3] : a.w[1], t2 = (sw & 2u) ? b.w[0] : a.w[2],
                           t3 = (sw & 2u) ? b.w[1] : a.w[3], t4 = (sw & 2u) ? b.w[2] : b.w[0], t5 = (sw & 2u) ? b.w[3] : b.w[1];
            const uint32_t u0 = (sw & 1u) ? t1 : t0, u1 = (sw & 1u) ? t2 : t1, u2 = (sw & 1u) ? t3 : t2, u3 = (sw & 1u) ? t4 : t3,
                           u4 = (sw & 1u) ? t5 : t4;
            o.w[0] = (uint32_t)((((uint64_t)u1 << 32) | u0) >> sb);
            o.w[1] = (uint32_t)((((uint64_t)u2 << 32) | u1) >> sb);
            o.w[2] = (uint32_t)((((uint64_t)u3 << 32) | u2) >> sb);
            o.w[3] = (uint32_t)((((uint64_t)u4 << 32) | u3) >> sb);
        }
        d16[i] = o;
    }
}

// the header of table entry r, from ONE thread: 1 or 4 byte stores
CSCMI_FHD void frame_put_header(uint8_t *dst, const FrameRec &r)
{
    for (uint32_t k = 0; k < r.hdr; k++) dst[r.dst_off + k] = (uint8_t)(r.hdr_bytes >> (8 * k));
}

}  // namespace cscmi
