// csc_dec_blocks.h -- the block framing of a libcsc stream, MemIO::ReadBlock (csc_memio.cpp:17-79) restated over a
// byte range instead of an ISeqInStream.  Compiles for the host (plain C++: tests/test_decode_device_host.py runs it
// with g++) and for the device (k_decode_dev*, csc_dec_kernels.hip); csc_dec_device.cpp's read_block is the same
// walk over Read callbacks.
//
//   flag byte: bit 7 = kind (1 range-coder block, 0 bit-coder block), bit 6 = "payload is exactly csc_blocksize bytes";
//   without bit 6 a 3-byte big-endian payload size follows; then the payload.
// Refused: a header or payload cut short, size 0, size > csc_blocksize, a full ring of the block's kind.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSCMI_HD __host__ __device__ inline
#else
#define CSCMI_HD inline
#endif

namespace cscmi {

struct DecBlock {
    uint32_t kind, size;
    uint64_t payload;      // offset of the payload's first byte
};

// The block whose flag byte sits at `pos`.  `ld(offset)` returns one source byte and is only ever asked for offsets
// below `src_size`.  0 and *b, or -1 (refusal).
template <class Load>
CSCMI_HD int dec_block_at(Load ld, uint64_t src_size, uint64_t pos, uint32_t bsize, DecBlock *b)
{
    if (pos >= src_size) return -1;
    const uint32_t fb = ld(pos);
    pos++;
    uint32_t cur = bsize;
    if (!((fb >> 6) & 1)) {
        if (src_size - pos < 3) return -1;
        cur = (ld(pos) << 16) + (ld(pos + 1) << 8) + ld(pos + 2);
        pos += 3;
    }
    if (!cur || cur > bsize) return -1;
    if (src_size - pos < cur) return -1;
    b->kind = (fb >> 7) & 1;
    b->size = cur;
    b->payload = pos;
    return 0;
}

// Blocks are read from *pos on until one of `kind` has arrived; each goes to the ring of its own kind:
// put(block, slot) stores it.  avail0 / avail1 (blocks queued so far, BC / RC) move on, taken0 / taken1 are the
// decoder's.  0, or -1 with *pos at the refused block.
template <class Load, class Put>
CSCMI_HD int dec_read_block(Load ld, uint64_t src_size, uint64_t *pos, uint32_t bsize, uint32_t kind, uint32_t qslots,
                            uint32_t *avail0, uint32_t *avail1, uint32_t taken0, uint32_t taken1, Put put)
{
    for (;;) {
        DecBlock b;
        if (dec_block_at(ld, src_size, *pos, bsize, &b) < 0) return -1;
        const uint32_t av = b.kind ? *avail1 : *avail0, tk = b.kind ? taken1 : taken0;
        if (av - tk >= qslots) return -1;
        put(b, av % qslots);
        if (b.kind) *avail1 = av + 1; else *avail0 = av + 1;
        *pos = b.payload + b.size;
        if (b.kind == kind) return 0;
    }
}

}  // namespace cscmi
