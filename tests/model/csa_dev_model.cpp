// csa_dev_model.cpp -- csc_amd/csrc/csa_dev_read.h on the CPU, thread by thread, under AddressSanitizer and UBSan
// (tests/test_archive_device_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_model PLANT        PLANT = 0: the text the kernels run; 1..4: one of the header's planted mistakes switched on
//
// Part 1, copy_sum: source alignment 0..15 x destination alignment 0..15 x the lengths below, with and without the store.  The
// ranges are heap buffers that END exactly where the range ends, so a load or a store behind it is the sanitizer's to report; in
// front of a range lie only the `alignment` bytes that put it there -- they are poisoned as far as ASan's 8-byte granules allow
// (source) and checked for change (destination).  Compared against memcpy and a byte-at-a-time adler32.
// Part 2, piece_split + copy_sum + fold_pieces: whole fragments at task offsets (posblock) of residues 0..15.
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

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
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
