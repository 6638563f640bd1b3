// csa_dev_write.h -- the device-resident archive write (CSAMI_DeviceWrite, include/csa_mi355x.h) below the host planner: a task's
// archive-block table, taken from the framed stream where it lies.  Compiles for the host (plain C++:
// tests/test_archive_device_write_host.py runs tests/model/csa_dev_write_model.cpp with g++ and the sanitizers) and for the device
// (k_block_table, csa_dev_kernels.hip), so the model runs the text the kernel runs.
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

}  // namespace csadev
