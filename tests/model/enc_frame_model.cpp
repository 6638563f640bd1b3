// enc_frame_model.cpp -- csc_amd/csrc/csc_enc_frame.h (the walk, the cap rule and the copy k_frame_blocks is built from) run on
// the host, the way the kernel runs it: per round one arena of (ArenaRec, payload padded to 16)*, walked kFrameBatch records at a
// time into a table, every table entry copied by 256 "threads" (here: one after the other), produced / rc carried from round to
// round, a stream whose rc is set skipped.  tests/test_encode_device_host.py builds this with -fsanitize=address,undefined and
// compares what it prints with a replay of the Write sequence in Python.
//
// argv[1]: a file of little-endian words
//   u32 bsize, u32 rounds, per round: u32 records, per record: u32 kind, u32 size, size payload bytes
//   u32 caps, per cap: u64 cap, u32 offset of dst inside its allocation (its alignment)
// prints "batch <kFrameBatch>", then per cap "<cap> <rc> <produced> <crc32 of dst[0, produced)>"; exits 3 if a byte outside
// dst[0, produced) was written (dst lies between sentinel bytes that are checked after every cap).  An arena is allocated at
// exactly its records' size: the sanitizer sees a load behind the last padded payload.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "csc_enc_frame.h"

using namespace cscmi;

static uint32_t crc32(const uint8_t *p, size_t n)
{
    static uint32_t t[256];
    if (!t[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1))); t[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

struct Arena { uint8_t *p; uint32_t used; };

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    int ch;
    while ((ch = fgetc(f)) != EOF) in.push_back((uint8_t)ch);
    fclose(f);
    size_t at = 0;
    auto u32 = [&]() { uint32_t v; if (at + 4 > in.size()) exit(2); memcpy(&v, in.data() + at, 4); at += 4; return v; };
    auto u64 = [&]() { uint64_t v; if (at + 8 > in.size()) exit(2); memcpy(&v, in.data() + at, 8); at += 8; return v; };
    const uint32_t bsize = u32(), rounds = u32();
    std::vector<Arena> arenas;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t nrec = u32();
        size_t scan = at, bytes = 0;
        for (uint32_t k = 0; k < nrec; k++) { uint32_t size; memcpy(&size, in.data() + scan + 4, 4); scan += 8 + size; bytes += 16 + ((size + 15) & ~15u); }
        Arena a;
        a.used = (uint32_t)bytes;
        a.p = (uint8_t *)aligned_alloc(16, bytes ? bytes : 16);      // exactly the records: a load behind the last padded payload is an error
        memset(a.p, 0xEE, bytes ? bytes : 16);
        uint32_t off = 0;
        for (uint32_t k = 0; k < nrec; k++) {
            const uint32_t kind = u32(), size = u32();
            memcpy(a.p + off, &kind, 4); memcpy(a.p + off + 4, &size, 4);
            if (at + size > in.size()) return 2;
            memcpy(a.p + off + 16, in.data() + at, size);
            at += size;
            off += 16 + ((size + 15) & ~15u);
        }
        arenas.push_back(a);
    }
    printf("batch %u\n", kFrameBatch);
    const uint32_t ncaps = u32();
    for (uint32_t q = 0; q < ncaps; q++) {
        const uint64_t cap = u64();
        const uint32_t doff = u32();
        uint8_t *alloc = (uint8_t *)aligned_alloc(16, ((size_t)doff + cap + 15) / 16 * 16 + 16);
        // (aligned_alloc wants a multiple of the alignment: the bytes behind dst + cap are guard bytes checked below)
        const size_t total = ((size_t)doff + cap + 15) / 16 * 16 + 16;
        memset(alloc, 0xA5, total);
        uint8_t *dst = alloc + doff;
        uint64_t produced = 0;
        int32_t rc = 0;
        for (const Arena &a : arenas) {
            if (rc != 0) continue;                                   // a stream that has ended is skipped
            FrameCursor cur;
            cur.arena_pos = 0; cur.error = 0; cur.produced = produced; cur.rc = 0;
            static FrameRec tab[kFrameBatch];
            for (;;) {
                const uint32_t n = frame_walk([&](uint32_t o) { uint32_t v; if (o + 4 > a.used) abort(); memcpy(&v, a.p + o, 4); return v; },
                                              a.used, bsize, cap, &cur, kFrameBatch, [&](uint32_t i, const FrameRec &r) { if (i >= kFrameBatch) abort(); tab[i] = r; });
                for (uint32_t r = 0; r < n; r++)
                    for (uint32_t tid = 0; tid < 256; tid++) {
                        if (tid == 32) frame_put_header(dst, tab[r]);
                        if (tab[r].size) frame_copy(dst + tab[r].dst_off + tab[r].hdr, a.p + tab[r].arena_off, tab[r].size, tid, 256);
                    }
                if (n < kFrameBatch) break;
            }
            if (cur.error) { printf("arena error\n"); return 4; }
            produced = cur.produced; rc = cur.rc;
        }
        if (produced > cap) return 3;
        for (size_t i = 0; i < total; i++)
            if ((i < doff || i >= doff + produced) && alloc[i] != 0xA5) { printf("stray store at %zd (cap %llu)\n", (ssize_t)i - (ssize_t)doff, (unsigned long long)cap); return 3; }
        printf("%llu %d %llu %u\n", (unsigned long long)cap, rc, (unsigned long long)produced, crc32(dst, produced));
        free(alloc);
    }
    for (Arena &a : arenas) free(a.p);
    return 0;
}
