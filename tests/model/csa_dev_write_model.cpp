// csa_dev_write_model.cpp -- csc_amd/csrc/csa_dev_write.h (the walk over a framed stream and the archive-block coalescer that
// k_block_table runs, one lane per task) on the CPU under AddressSanitizer and UBSan (tests/test_archive_device_write_host.py
// builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_write_model PLANT [FILE]     PLANT = 0: the text the kernel runs; 1..3: one of the header's planted mistakes
//
// Without FILE: the constructed streams below.  Each is built from a list of coder blocks, which is also the list of Write calls
// the file path would have seen; the expected table is AsyncWriter::Write (csa_io.h:145-201) restated here over that list.
// With FILE: streams from outside (the oracle encoder's), little-endian: u32 count, per stream u32 csc_blocksize, u64 size, bytes.
// Either way every stream lies in a heap buffer that ends exactly where the stream ends, so a load behind `produced` is the
// sanitizer's to report, and is walked with a table of exactly table_bound() entries.
// Per stream one line "table <name> status <s> blocks <n> : <sizes...>" (FILE: the name is the stream's number); a constructed
// stream also gets "writes <name> : <sizes...>" for a check from outside.  The first case that fails is named on a line
// "FAIL <case>"; when AddressSanitizer ends the run, the case is named on a line "AT <case>".  Exit status 0 only if all passed.
#include <sanitizer/common_interface_defs.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csa_dev_write.h"

using namespace csadev;

static char g_case[128] = "start";
static void on_death() { fprintf(stderr, "AT %s\n", g_case); fflush(stderr); }

struct Block { uint32_t size; bool bit6; };

struct Built { std::vector<uint8_t> stream; std::vector<uint64_t> writes; };

static Built build(const std::vector<Block> &blocks)
{
    Built b;
    b.writes.push_back(kPropBytes);
    uint8_t fill = 1;
    for (const Block &k : blocks) {
        b.stream.push_back((uint8_t)(0x80u | (k.bit6 ? 0x40u : 0u)));
        b.writes.push_back(1);
        if (!k.bit6) {
            b.stream.push_back((uint8_t)(k.size >> 16)); b.stream.push_back((uint8_t)(k.size >> 8)); b.stream.push_back((uint8_t)k.size);
            b.writes.push_back(3);
        }
        // (payload bytes that read as a small size and as flags without bit 6, should a walk take them for either)
        for (uint32_t i = 0; i < k.size; i++) b.stream.push_back((uint8_t)(i < 2 ? 0 : (fill++ & 0x3F) | 1u));
        if (k.size) b.writes.push_back(k.size);
    }
    return b;
}

static std::vector<uint64_t> expect(const std::vector<uint64_t> &writes)      // csa_io.h:188-192, :596-603
{
    std::vector<uint64_t> out;
    uint64_t cur = 0, cap = 1048576;
    for (uint64_t size : writes) {
        if (cur + size > cap) {
            if (cur > 0) out.push_back(cur);
            cur = 0;
            cap = size > 1048576 ? size : 1048576;
        }
        cur += size;
    }
    if (cur > 0) out.push_back(cur);
    return out;
}

template <int PLANT>
static uint32_t walk(const uint8_t *stream, uint64_t produced, uint32_t bsize, std::vector<uint64_t> &table, uint32_t *nblocks)
{
    uint8_t *exact = (uint8_t *)malloc(produced ? produced : 1);              // ends where the stream ends
    if (produced) memcpy(exact, stream, produced);
    const uint64_t bound = table_bound(produced, bsize);
    uint64_t *slots = (uint64_t *)malloc(bound * sizeof(uint64_t));           // and the table where its bound ends
    const uint32_t status = block_table<PLANT>([exact, produced](uint64_t i) { if (i >= produced) abort(); return (uint32_t)exact[i]; },
                                               produced, bsize, (uint32_t)bound, [slots](uint32_t i, uint64_t size) { slots[i] = size; }, nblocks);
    table.assign(slots, slots + (*nblocks < bound ? *nblocks : bound));
    free(slots);
    free(exact);
    return status;
}

static void print_table(const char *name, uint32_t status, uint32_t nblocks, const std::vector<uint64_t> &table)
{
    printf("table %s status %u blocks %u :", name, status, nblocks);
    for (uint64_t s : table) printf(" %llu", (unsigned long long)s);
    printf("\n");
}

static int fail() { printf("FAIL %s\n", g_case); return 1; }

template <int PLANT>
static int run_constructed()
{
    const uint32_t bs = 65536, MiB = 1048576;
    struct Case { const char *name; uint32_t bsize; std::vector<Block> blocks; uint64_t cut; };      // cut: bytes taken off the end
    const std::vector<Case> cases = {
        {"empty stream", bs, {}, 0},
        {"bit-6 block", 64, {{64, true}, {0, false}}, 0},
        {"empty payload", bs, {{100, false}, {0, false}, {7, false}, {0, false}}, 0},
        {"exactly 1 MiB at a flush point", bs, {{MiB - 14, false}, {0, false}}, 0},
        {"1 MiB + 1 at a flush point", bs, {{MiB - 13, false}, {0, false}}, 0},
        {"full blocks across 1 MiB", bs, std::vector<Block>(40, Block{bs, true}), 0},
        {"payload above 1 MiB", bs, {{5, false}, {MiB + 100, false}, {9, false}, {0, false}}, 0},
        {"one byte short of the last payload", bs, {{300, false}, {bs, true}}, 1},
        {"cut inside a size field", bs, {{300, false}, {200, false}}, 202},
    };
    for (const Case &c : cases) {
        snprintf(g_case, sizeof(g_case), "%s", c.name);
        const Built b = build(c.blocks);
        const uint64_t produced = b.stream.size() - c.cut;
        std::vector<uint64_t> table;
        uint32_t nblocks = 0;
        const uint32_t status = walk<PLANT>(b.stream.data(), produced, c.bsize, table, &nblocks);
        print_table(c.name, status, nblocks, table);
        printf("writes %s :", c.name);
        for (uint64_t w : b.writes) printf(" %llu", (unsigned long long)w);
        printf("\n");
        if (c.cut) { if (status != kTableCut) return fail(); continue; }
        if (status != kTableOk || nblocks != table.size() || table != expect(b.writes)) return fail();
        uint64_t sum = 0;
        for (uint64_t s : table) sum += s;
        if (sum != kPropBytes + produced) return fail();
    }
    printf("ok %zu\n", cases.size());
    return 0;
}

template <int PLANT>
static int run_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    int ch;
    while ((ch = fgetc(f)) != EOF) in.push_back((uint8_t)ch);
    fclose(f);
    size_t at = 0;
    auto take = [&](void *p, size_t n) { if (at + n > in.size()) exit(2); memcpy(p, in.data() + at, n); at += n; };
    uint32_t count;
    take(&count, 4);
    for (uint32_t k = 0; k < count; k++) {
        uint32_t bsize;
        uint64_t size;
        take(&bsize, 4); take(&size, 8);
        if (at + size > in.size()) return 2;
        snprintf(g_case, sizeof(g_case), "%u", k);
        std::vector<uint64_t> table;
        uint32_t nblocks = 0;
        const uint32_t status = walk<PLANT>(in.data() + at, size, bsize, table, &nblocks);
        print_table(g_case, status, nblocks, table);
        at += size;
    }
    return 0;
}

template <int PLANT>
static int run(const char *path) { return path ? run_file<PLANT>(path) : run_constructed<PLANT>(); }

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    const char *path = argc > 2 ? argv[2] : nullptr;
    switch (plant) {
    case kWPlantNone: return run<kWPlantNone>(path);
    case kWPlantFlushAtEqual: return run<kWPlantFlushAtEqual>(path);
    case kWPlantPropsLeftOut: return run<kWPlantPropsLeftOut>(path);
    case kWPlantBit6FromField: return run<kWPlantBit6FromField>(path);
    }
    return 2;
}
