// csa_dev_model.cpp -- csc_amd/csrc/csa_dev_read.h on the CPU, thread by thread, under AddressSanitizer and UBSan
// (tests/test_archive_device_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_model PLANT        PLANT = 0: the text the kernels run; 1..4: one of the header's planted mistakes switched on
//   csa_dev_model waves        the wave planner of the archive layer's host side (csc_amd/csrc/csa_waves.h), Part 3
//
// Part 1, copy_sum: source alignment 0..15 x destination alignment 0..15 x the lengths below, with and without the store.  The
// ranges are heap buffers that END exactly where the range ends, so a load or a store behind it is the sanitizer's to report; in
// front of a range lie only the `alignment` bytes that put it there -- they are poisoned as far as ASan's 8-byte granules allow
// (source) and checked for change (destination).  Compared against memcpy and a byte-at-a-time adler32.
// Part 2, piece_split + copy_sum + fold_pieces: whole fragments at task offsets (posblock) of residues 0..15.
// Part 3, wave_count: how many tasks a wave takes under a width and a budget, at the edges of both and of 64 bits.
//
// The first case that fails is named on a line "FAIL <case>"; when AddressSanitizer ends the run, the case it happened in is named
// on a line "AT <case>".  UBSan's runtime makes no such call, so with a mistake planted every case is announced on a line
// "IN <case>" before it runs: the last one is where the run ended.  Exit status 0 only if every case passed.
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csa_dev_read.h"
#include "csa_waves.h"

using namespace csadev;

static char g_case[128] = "start";
static void on_death() { fprintf(stderr, "AT %s\n", g_case); fflush(stderr); }

static uint32_t adler32_bytes(const uint8_t *p, uint64_t n)          // csa_adler32.cpp:63-129 with seed 0, one byte at a time
{
    uint32_t a = 0, b = 0;
    for (uint64_t i = 0; i < n; i++) { a = (a + p[i]) % kAdlerBase; b = (b + a) % kAdlerBase; }
    return a | (b << 16);
}

static uint32_t g_rng = 12345;
static uint8_t next_byte() { g_rng = g_rng * 1664525u + 1013904223u; return (uint8_t)((g_rng >> 24) | 1u); }   // never 0: a dropped byte shows

struct Range {                 // `n` bytes at alignment `al`, ending exactly where their allocation ends
    uint8_t *base, *p;
    uint32_t al;
    Range(uint32_t al_, uint64_t n, bool poison_front) : al(al_)
    {
        base = (uint8_t *)malloc(al + n ? al + n : 1);
        if (((uintptr_t)base & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
        p = base + al;
        memset(base, 0xA5, al);
        if (poison_front) __asan_poison_memory_region(base, al & ~7u);
    }
    bool front_intact() const { for (uint32_t i = 0; i < al; i++) if (base[i] != 0xA5) return false; return true; }
    ~Range() { __asan_unpoison_memory_region(base, al); free(base); }
};

template <bool STORE, int PLANT>
static void run_piece(uint8_t *dst, const uint8_t *src, uint32_t n, PieceSums &s)
{
    s.a = s.b = 0;
    for (uint32_t tid = 0; tid < kThreads; tid++) copy_sum<STORE, true, PLANT>(dst, src, n, tid, kThreads, s.a, s.b);
}

static int fail() { printf("FAIL %s\n", g_case); return 1; }
static void enter(bool announce) { if (announce) { fprintf(stderr, "IN %s\n", g_case); fflush(stderr); } }

template <int PLANT>
static int run_all()
{
    static const uint32_t lens[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 16383, 16384};
    uint64_t ncases = 0;
    for (int store = 1; store >= 0; store--)
        for (uint32_t sa = 0; sa < 16; sa++)
            for (uint32_t da = 0; da < 16; da++)
                for (uint32_t n : lens) {
                    snprintf(g_case, sizeof(g_case), "copy store=%d sa=%u da=%u n=%u", store, sa, da, n);
                    enter(PLANT != kPlantNone);
                    Range src(sa, n, true), dst(da, n, false);
                    for (uint32_t i = 0; i < n; i++) { src.p[i] = next_byte(); dst.p[i] = 0x5A; }
                    PieceSums s;
                    if (store) run_piece<true, PLANT>(dst.p, src.p, n, s);
                    else run_piece<false, PLANT>(dst.p, src.p, n, s);
                    uint64_t A = 0, B = 0;
                    for (uint32_t i = 0; i < n; i++) { A += src.p[i]; B += (uint64_t)(n - i) * src.p[i]; }
                    if (s.a != A || s.b != B) return fail();
                    const PieceSums *sp = &s;
                    if (fold_pieces<PLANT>([sp](uint32_t) { return *sp; }, n ? 1 : 0, n) != adler32_bytes(src.p, n)) return fail();
                    if (!dst.front_intact()) return fail();
                    for (uint32_t i = 0; i < n; i++) if (dst.p[i] != (store ? src.p[i] : 0x5A)) return fail();
                    ncases++;
                }
    static const uint64_t sizes[] = {1, 16383, 16384, 16385, 32768, 32769, 100003};
    for (uint64_t size : sizes)
        for (uint32_t res = 0; res < 16; res++)
            for (int store = 1; store >= 0; store--) {
                snprintf(g_case, sizeof(g_case), "frag size=%llu res=%u store=%d", (unsigned long long)size, res, store);
                enter(PLANT != kPlantNone);
                Range task(res, size, true), dst((res * 7 + 3) & 15u, size, false);
                for (uint64_t i = 0; i < size; i++) { task.p[i] = next_byte(); dst.p[i] = 0x5A; }
                std::vector<CopyPiece> pieces;
                const uint64_t np = piece_split(task.p, store ? dst.p : nullptr, size, kFragPiece, [&](uint64_t k, const CopyPiece &p) {
                    if (k != pieces.size()) exit(3);
                    pieces.push_back(p);
                });
                if (np != piece_count(size, kFragPiece) || np != pieces.size()) return fail();
                std::vector<PieceSums> sums(np);
                uint64_t covered = 0;
                for (uint64_t k = 0; k < np; k++) {
                    if (pieces[k].src != task.p + covered || pieces[k].len == 0 || pieces[k].len > kFragPiece) return fail();
                    if (store) run_piece<true, PLANT>(pieces[k].dst, pieces[k].src, pieces[k].len, sums[k]);
                    else run_piece<false, PLANT>(nullptr, pieces[k].src, pieces[k].len, sums[k]);
                    covered += pieces[k].len;
                }
                if (covered != size) return fail();
                const PieceSums *sp = sums.data();
                if (fold_pieces<PLANT>([sp](uint32_t k) { return sp[k]; }, (uint32_t)np, size) != adler32_bytes(task.p, size)) return fail();
                if (!dst.front_intact()) return fail();
                for (uint64_t i = 0; i < size; i++) if (dst.p[i] != (store ? task.p[i] : 0x5A)) return fail();
                ncases++;
            }
    printf("ok %llu\n", (unsigned long long)ncases);
    return 0;
}

// Part 3, wave_count (csa_waves.h): every expected count below is written out by hand.
static int run_waves()
{
    using csa::wave_count;
    const uint64_t M = UINT64_MAX;
    uint64_t ncases = 0;
    struct Case { const char *name; std::vector<uint64_t> need; size_t first, width; uint64_t budget; size_t want; };
    const std::vector<Case> cases = {
        {"width 1", {10, 10, 10}, 0, 1, 1000, 1},
        {"first task over the whole budget: taken, alone", {5000, 1, 1}, 0, 8, 1000, 1},
        {"exact fit", {400, 300, 300, 1}, 0, 8, 1000, 3},
        {"one byte more than fits", {400, 300, 301, 1}, 0, 8, 1000, 2},
        {"fewer tasks left than width", {10, 10, 10, 10, 10}, 3, 8, 1000, 2},
        {"none left", {10, 10}, 2, 8, 1000, 0},
        {"need UINT64_MAX, not first", {10, M, 10}, 0, 8, M, 1},
        {"need UINT64_MAX, first", {10, M, 10}, 1, 8, M, 1},
        {"a sum that would wrap", {M - 5, 6, 1}, 0, 8, M, 1},
        {"a sum just short of wrapping, over the budget", {M - 5, 4, 1}, 0, 8, M - 2, 1},
    };
    for (const Case &c : cases) {
        snprintf(g_case, sizeof(g_case), "waves %s", c.name);
        const std::vector<uint64_t> &need = c.need;
        if (wave_count(c.first, need.size(), c.width, c.budget, [&](size_t t) { return need.at(t); }) != c.want) return fail();
        ncases++;
    }
    // a walk over eight tasks, budget 100, width 3:
    //   60 + 40 = 100 fits, + 1 does not            -> [0, 2)
    //   1 + 99 = 100 fits, + 100 does not           -> [2, 4)
    //   100 alone, + 30 does not                    -> [4, 5)
    //   30 + 30 + 30 = 90 fits, and width is reached -> [5, 8)
    snprintf(g_case, sizeof(g_case), "waves walk");
    const std::vector<uint64_t> need = {60, 40, 1, 99, 100, 30, 30, 30};
    const std::vector<size_t> want = {0, 2, 4, 5, 8};
    std::vector<size_t> got = {0};
    for (size_t first = 0; first < need.size() && got.size() < 16;) {
        first += wave_count(first, need.size(), 3, 100, [&](size_t t) { return need.at(t); });
        got.push_back(first);
    }
    if (got != want) return fail();
    ncases++;
    // hbm_budget: the override, else 3/4 of what is free
    snprintf(g_case, sizeof(g_case), "waves budget");
    CSAOptions o;
    memset(&o, 0, sizeof(o));
    if (csa::hbm_budget(o, 4000) != 3000) return fail();
    o.hbm_budget = 64u << 20;
    if (csa::hbm_budget(o, 4000) != (64u << 20)) return fail();
    ncases++;
    printf("ok waves %llu\n", (unsigned long long)ncases);
    return 0;
}

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    if (argc > 1 && !strcmp(argv[1], "waves")) return run_waves();
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    switch (plant) {
    case kPlantNone: return run_all<kPlantNone>();
    case kPlantTailDropped: return run_all<kPlantTailDropped>();
    case kPlantWeightOffByOne: return run_all<kPlantWeightOffByOne>();
    case kPlantFoldLastLen: return run_all<kPlantFoldLastLen>();
    case kPlantHeadWrongPointer: return run_all<kPlantHeadWrongPointer>();
    }
    return 2;
}
