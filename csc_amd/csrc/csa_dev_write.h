// csa_dev_write.h -- the device-resident archive write (CSAMI_DeviceWrite, include/csa_mi355x.h) below the host planner: a task's
// archive-block table, taken from the framed stream where it lies.  Compiles for the host (plain C++:
// tests/test_archive_device_write_host.py runs tests/model/csa_dev_write_model.cpp with g++ and the sanitizers) and for the device
// (k_block_table, csa_dev_kernels.hip), so the model runs the text the kernel runs.  Its second half is the piece of
// CSAMI_DeviceWriteSlices whose source is periodic (k_frag_rows; gather_reduce, gather_sum and their model are described there).
//
// What the reference does here: the encoder hands its output to AsyncArchiveWriter through ISeqOutStream::Write, and the writer
// coalesces those calls into archive blocks (AsyncWriter::Write / flush, csa_io.h:145-201; Finish, :596-603):
//     if (cur + size > cap) { flush what is there; cap = max(1 MiB, size); }   append
// so the table depends on the SIZES of the Write calls alone.  The file path gets them from the callbacks (BlockSink::put,
// csa_archive.cpp); a stream framed on the device (CSCMI_EncodeDeviceBatch) made no callback, but the sizes can be read back off
// its framing (MemIO::WriteBlock, csc_memio.cpp:83-108; csc_enc_frame.h):
//     10                      the property bytes (csa_worker.cpp:38-42)
//     per coder block:  1     the flag byte; bit 6 = "the payload is exactly csc_blocksize bytes"
//                       3     without bit 6: the payload size, big-endian
//                       size  the payload, unless it is empty
//
// The template parameter PLANT switches one deliberate mistake on (0: none).  The product instantiates 0 only; the model runs each
// of the others and has to see it caught by a named case.
#pragma once
#include <stdint.h>

#include "csa_dev_read.h"

namespace csadev {

constexpr uint64_t kArcBlockCap = 1048576;      // csa_io.h:158
constexpr uint32_t kPropBytes = 10;             // CSC_PROP_SIZE
constexpr uint32_t kTableThreads = 256;         // the one workgroup of k_block_table
constexpr uint32_t kTableMaxJobs = 2048;        // tasks of one k_block_table launch (= the most streams of a wave)

enum WritePlant { kWPlantNone = 0, kWPlantFlushAtEqual = 1, kWPlantPropsLeftOut = 2, kWPlantBit6FromField = 3 };
enum TableStatus { kTableOk = 0, kTableCut = 1, kTableFull = 2 };     // kTableCut: the walk does not end at `produced`

struct BlockTableJob {     // one task of k_block_table
    const uint8_t *stream; // the framed stream AFTER its property bytes
    uint64_t produced;     // its bytes
    uint32_t bsize;        // csc_blocksize of its props
    uint32_t max_blocks;   // entries this task may store
    uint64_t first;        // its first entry in the scratch table
};
struct BlockTableRes { uint32_t nblocks, status; };       // per task, all the host reads back besides the sizes themselves

// entries a task of `produced` stream bytes can need: every block flushed before the end holds more than 1 MiB - bsize bytes (a
// Write of the encoder's is at most bsize long), and the end flushes one more
CSADEV_FHD uint64_t table_bound(uint64_t produced, uint32_t bsize)
{
    const uint64_t least = bsize < kArcBlockCap ? kArcBlockCap - bsize : 1;
    return produced / least + 2;
}

// AsyncWriter::Write over sizes alone; put(k, size) stores block k
template <int PLANT = kWPlantNone>
struct Coalescer {
    uint64_t cur = 0, cap = kArcBlockCap;
    uint32_t n = 0, max_blocks = 0;
    bool full = false;
    template <class Put>
    CSADEV_FHD void flush(Put put)
    {
        if (!cur) return;
        if (n < max_blocks) put(n, cur); else full = true;
        n++;
        cur = 0;
    }
    template <class Put>
    CSADEV_FHD void write(uint64_t size, Put put)
    {
        if (PLANT == kWPlantFlushAtEqual ? cur + size >= cap : cur + size > cap) {
            flush(put);
            cap = size > kArcBlockCap ? size : kArcBlockCap;
        }
        cur += size;
    }
};

// The block table of one task: ld(i) returns byte i of the stream, i < produced -- no other byte is asked for.  Returns the status;
// *nblocks is the number of blocks the stream has (of which min(*nblocks, max_blocks) were stored).
template <int PLANT = kWPlantNone, class Load, class Put>
CSADEV_FHD uint32_t block_table(Load ld, uint64_t produced, uint32_t bsize, uint32_t max_blocks, Put put, uint32_t *nblocks)
{
    Coalescer<PLANT> co;
    co.max_blocks = max_blocks;
    uint32_t status = kTableOk;
    if (PLANT != kWPlantPropsLeftOut) co.write(kPropBytes, put);
    uint64_t pos = 0;
    while (pos < produced) {
        const uint32_t flag = ld(pos);
        pos += 1;
        co.write(1, put);
        uint64_t size = bsize;
        if (!(flag & 0x40u) || PLANT == kWPlantBit6FromField) {
            if (produced - pos < 3) { status = kTableCut; break; }
            size = (uint64_t)ld(pos) << 16 | (uint64_t)ld(pos + 1) << 8 | (uint64_t)ld(pos + 2);
            pos += 3;
            co.write(3, put);
        }
        if (size) {
            if (produced - pos < size) { status = kTableCut; break; }
            pos += size;
            co.write(size, put);
        }
    }
    co.flush(put);
    *nblocks = co.n;
    if (status == kTableOk && co.full) status = kTableFull;
    return status;
}

// ---- entries gathered from strided slices of the caller's buffers (CSAMI_DeviceWriteSlices): the transpose of slice_sum ----
//
// An entry's bytes are what a checked Slice selects of a buffer, packed row after row: packed byte p lies at buffer offset
// offset + (p / run) * stride + p % run.  The pieces of a fragment stay on the fixed kFragPiece grid of the PACKED fragment
// (fold_pieces needs it), so a piece's destination is contiguous and its source is the tail of one run, a gap and the head of the
// next -- or, where run is small, many of them.  gather_whole and gather_reduce are the host planner's; gather_sum is the
// workgroup's (tests/model/csa_dev_gather_model.cpp is their model).  With run < 16 every 16-byte unit crosses a run border and is
// assembled byte by byte: that is the slow path, and no rate is promised for it.

enum GatherPlant {
    kGPlantNone = 0, kGPlantBorderLate = 1, kGPlantPhaseDropped = 2, kGPlantStraddleContiguous = 3, kGPlantRowNotAdvanced = 4,
    kGPlantWindowPastHull = 5,
    // the form that only sums (tests/model/csa_dev_sum_only_model.cpp)
    kGPlantSumTailDropped = 6, kGPlantSumStillStores = 7
};

struct GatherPiece {       // one workgroup of k_frag_rows
    const uint8_t *src;    // stride == 0: the piece's one contiguous source (copy_sum<true, true>, as a CopyPiece);
                           // else the address of period position 0, inside the hull (what lies in front of `phase` is not loaded)
    uint8_t *dst;          // the piece's contiguous destination; NULL: the piece is summed, not stored
    uint64_t stride;       // periodic: the address step from one run to the next, >= run
    uint32_t len;          // <= kFragPiece
    uint32_t phase;        // periodic: byte i of the piece is period position pos = phase + i; row = pos / run, r = pos % run; it lies
    uint32_t run;          //           at src + row * stride + r
    uint32_t pad;
    const uint8_t *lo, *hi;   // periodic: the slice's hull [lo, hi): all that a load window may touch
};

// The packed bytes [at, at + size), size > 0, of a checked slice (at + size <= run * count): true if they lie inside one run, and
// *src is then the buffer offset of the first.  One division, no walk over the rows.
CSADEV_FHD bool gather_whole(const Slice &s, uint64_t at, uint64_t size, uint64_t *src)
{
    const uint64_t k0 = at / s.run, r0 = at - k0 * s.run;
    *src = s.offset + k0 * s.stride + r0;
    return s.run - r0 >= size;
}

struct GatherCut { uint64_t src, stride; uint32_t phase, run; };

// The piece [at, at + len) of the packed bytes, 0 < len <= kFragPiece, under a checked slice: true if it lies inside one run (c.src
// is the buffer offset of its first byte, the rest of c is 0).  Else c is the GatherPiece's phase, run and stride, and c.src the
// buffer offset of period position 0.  A piece sees at most kFragPiece packed bytes, so whatever the 64-bit run is it sees the same
// as under a run cut to kFragPiece -- the run it begins in from its front, since what lies before the piece is not seen, the next
// one from its back: run' = min(run, kFragPiece) and stride' = stride - (run - run'), so phase + len < 2^16 and every division of
// gather_sum is one of 32-bit quantities.  The stride is an address step and stays 64-bit.  Patterns that fit are left as they are.
CSADEV_FHD bool gather_reduce(const Slice &s, uint64_t at, uint32_t len, GatherCut &c)
{
    c = GatherCut{0, 0, 0, 0};
    if (gather_whole(s, at, len, &c.src)) return true;
    const uint64_t k0 = at / s.run, r0 = at - k0 * s.run;
    const uint64_t cut = s.run > kFragPiece ? s.run - kFragPiece : 0;        // (r0 > cut: fewer than len bytes are left of the run)
    c.src = s.offset + k0 * s.stride + cut;
    c.stride = s.stride - cut;
    c.run = (uint32_t)(s.run - cut);
    c.phase = (uint32_t)(r0 - cut);
    return false;
}

// Thread `tid` of `nthreads`: its share of a periodic piece.  The anchor is the destination: up to 15 head bytes bring it to a
// 16-byte line and up to 15 tail bytes end the piece, byte by byte; between them every unit is one aligned 16-byte store.  A unit
// whose 16 packed bytes lie inside one run is loaded as load_unit loads (load_window: the window is checked against the HULL, so gap
// bytes may be loaded; they are never summed and never stored); a unit across a run border is assembled row segment by row
// segment, byte by byte.  The sums are over packed positions, as one piece of len bytes: exactly copy_sum<true, true>'s over the
// packed bytes.  No division in the unit loop: a thread's (row, r) advances by the workgroup's step, 16 * nthreads packed
// positions, with one carry.
//
// STORE == false (CSAMI_DeviceUpdate's check of a piece against the base's checksum; k_frag_rows with dst == NULL): the piece is
// summed and nothing is stored -- pc.dst is not looked at.  There is no destination to anchor on, so the 16-byte units begin at
// the piece's packed position 0 (no head, up to 15 tail bytes); a unit's load window is still checked against the hull.  The sums
// are those of the storing form, whatever its destination's alignment.
template <int PLANT = kGPlantNone, bool STORE = true>
CSADEV_FHD void gather_sum(const GatherPiece &pc, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b)
{
    constexpr bool kStores = STORE || PLANT == kGPlantSumStillStores;
    const uint8_t *src = pc.src;
    uint8_t *dst = pc.dst;
    const uint32_t n = pc.len, run = pc.run;
    const uint64_t stride = pc.stride;
    uint32_t head = STORE ? (0u - (uint32_t)(uintptr_t)dst) & 15u : 0u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = !STORE && PLANT == kGPlantSumTailDropped ? 0u : (n - head) & 15u;
    auto one = [&](uint32_t idx) {
        const uint32_t pos = pc.phase + idx, row = pos / run, r = pos - row * run;
        const uint32_t v = src[row * stride + r];
        if (kStores) dst[idx] = (uint8_t)v;
        a += v;
        b += (uint64_t)(n - idx) * v;
    };
    if (tid < head) one(tid);
    if (nthreads - 1 - tid < tail) one(head + 16 * units + (nthreads - 1 - tid));
    if (tid >= units) return;
    const uint32_t step = 16 * nthreads, srow = step / run, sr = step - srow * run;
    const uint32_t border = PLANT == kGPlantBorderLate ? run + 1 : run;              // r == border: the next row begins
    const uint32_t pos = (PLANT == kGPlantPhaseDropped ? 0u : pc.phase) + head + 16 * tid;
    uint32_t row = pos / run, r = pos - row * run;
    for (uint32_t i = tid; i < units; i += nthreads) {
        const uint32_t i0 = head + 16 * i;
        const uint8_t *p = src + row * stride + r;
        Vec16 o;
        if (PLANT == kGPlantStraddleContiguous || r + 16 <= run) {
            o = load_window<PLANT == kGPlantWindowPastHull>(p, pc.lo, pc.hi);
        } else {
            o = Vec16{{0, 0, 0, 0}};
            uint32_t r1 = r;
            for (uint32_t j = 0; j < 16; j++) {
                o.w[j >> 2] |= (uint32_t)*p++ << (8 * (j & 3u));
                if (++r1 == border) { r1 = 0; p += stride - run; }
            }
        }
        if (kStores) *(Vec16 *)(dst + i0) = o;
        sum_word(o.w[0], i0, n, a, b);
        sum_word(o.w[1], i0 + 4, n, a, b);
        sum_word(o.w[2], i0 + 8, n, a, b);
        sum_word(o.w[3], i0 + 12, n, a, b);
        r += sr;
        row += srow;
        if (r >= run) { r -= run; if (PLANT != kGPlantRowNotAdvanced) row++; }
    }
}

}  // namespace csadev
