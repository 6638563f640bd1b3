// csa_dev_sum_only_model.cpp -- gather_sum<PLANT, false> of csc_amd/csrc/csa_dev_write.h (the text k_frag_rows runs for a piece
// without a destination: CSAMI_DeviceUpdate's check under CSAMI_UPDATE_TRUST_SUMS) on the CPU, thread by thread, under
// AddressSanitizer and UBSan (tests/test_archive_update_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_sum_only_model PLANT     PLANT = 0: the text the kernel runs; 5, 6, 7: one of the header's planted mistakes switched on
//
// Part 1, the form that only sums against the storing one and a byte-wise sum: alignment of period position 0 of the source 0..15 x
// kLens x kPatterns (run 1, 15, 16, 17 and 4099 among them), the phase such that pieces begin and end inside a run.  The source is
// a heap block that is EXACTLY the hull of the rows the piece meets (it begins `alignment` bytes into its allocation, poisoned in
// front as far as ASan's 8-byte granules allow, and ends where the allocation ends), so a load outside the hull is the sanitizer's
// to report; gap bytes are random like the others, so one that is summed shows.  The form that only sums is handed a destination
// filled with a canary -- the kernel hands it none -- and must leave every byte of it as it was.  Expected: A = sum(b_i) and
// B = sum((len - i) * b_i) over the packed bytes taken with a plain loop, and the same from gather_sum<0, true> into a destination
// of alignment 0 and of alignment 5.
// Part 2, a fragment of 40000 packed bytes at packed offset 12345 of its entry under a few slices, the buffer exactly offset + hull
// bytes: gather_reduce per 16 KiB cell, each piece summed as k_frag_rows sums one without a destination, fold_pieces -- against a
// byte-at-a-time adler32 of the definition's packed bytes.
//
// The first case that fails is named on a line "FAIL <case>"; when a sanitizer ends the run, the case it happened in is named on
// a line "AT <case>".  Exit status 0 only if every case passed.
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csa_dev_write.h"

using namespace csadev;

static char g_case[160] = "start";
static void on_death() { fprintf(stderr, "AT %s\n", g_case); fflush(stderr); }
static int fail() { printf("FAIL %s\n", g_case); return 1; }

static uint32_t adler32_bytes(const uint8_t *p, uint64_t n)          // csa_adler32.cpp:63-129 with seed 0, one byte at a time
{
    uint32_t a = 0, b = 0;
    for (uint64_t i = 0; i < n; i++) { a = (a + p[i]) % kAdlerBase; b = (b + a) % kAdlerBase; }
    return a | (b << 16);
}

static uint32_t g_rng = 2463534242u;
static uint8_t next_byte() { g_rng = g_rng * 1664525u + 1013904223u; return (uint8_t)((g_rng >> 24) | 1u); }   // never 0: a dropped byte shows

struct Range {                 // `n` random bytes at alignment `al`, ending exactly where their allocation ends
    uint8_t *base, *p;
    uint32_t al;
    Range(uint32_t al_, uint64_t n) : al(al_)
    {
        base = (uint8_t *)malloc(al + n ? al + n : 1);
        if (((uintptr_t)base & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
        p = base + al;
        memset(base, 0xA5, al);
        for (uint64_t i = 0; i < n; i++) p[i] = next_byte();
        __asan_poison_memory_region(base, al & ~7u);
    }
    ~Range() { __asan_unpoison_memory_region(base, al); free(base); }
};

static uint64_t defined(const Slice &s, uint64_t p) { return s.offset + (p / s.run) * s.stride + p % s.run; }

static const uint32_t kLens[] = {1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384};
static const uint32_t kPatterns[][2] = {{1, 2}, {1, 16}, {3, 5}, {15, 16}, {16, 16}, {16, 17}, {17, 48}, {100, 1000}, {4099, 4100}, {4099, 8197},
                                        {16384, 16384}};
static const uint32_t kCanary = 16384 + 64;

// every thread of the workgroup over one piece: as k_frag_rows runs one without a destination (STORE == false), or with one
template <int PLANT, bool STORE>
static PieceSums run_piece(const GatherPiece &pc)
{
    PieceSums s = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        if (pc.stride) gather_sum<PLANT, STORE>(pc, tid, kThreads, s.a, s.b);
        else copy_sum<STORE, true>(pc.dst, pc.src, pc.len, tid, kThreads, s.a, s.b);
    }
    return s;
}

template <int PLANT>
static int part1(uint64_t &ncases)
{
    std::vector<uint8_t> canary(kCanary, 0xC3), stored(kCanary);
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t n : kLens)
            for (const uint32_t *pat : kPatterns) {
                const uint32_t run = pat[0], stride = pat[1], phase = (7 * sa + n) % run;
                snprintf(g_case, sizeof(g_case), "sum sa=%u n=%u run=%u stride=%u", sa, n, run, stride);
                const uint32_t rows = (phase + n - 1) / run + 1;
                const uint64_t hull = (uint64_t)(rows - 1) * stride + run;
                Range src(sa, hull);
                uint64_t wa = 0, wb = 0;
                for (uint32_t i = 0; i < n; i++) {                    // the packed bytes, with a plain loop, and their sums
                    const uint8_t v = src.p[(uint64_t)((phase + i) / run) * stride + (phase + i) % run];
                    wa += v;
                    wb += (uint64_t)(n - i) * v;
                }
                // a destination the form that only sums must not touch: alignment 3, so that a head taken from it would show too
                const GatherPiece pc = {src.p, canary.data() + 3, stride, n, phase, run, 0, src.p, src.p + hull};
                const PieceSums s = run_piece<PLANT, false>(pc);
                for (uint8_t c : canary)
                    if (c != 0xC3) return fail();
                if (s.a != wa || s.b != wb) return fail();
                for (uint32_t da : {0u, 5u}) {                        // the storing form, whatever its destination's alignment
                    GatherPiece st = pc;
                    st.dst = stored.data() + da;
                    const PieceSums t = run_piece<kGPlantNone, true>(st);
                    if (t.a != s.a || t.b != s.b) return fail();
                }
                ncases++;
            }
    return 0;
}

template <int PLANT>
static int part2(uint64_t &ncases)
{
    static const uint64_t pats[][2] = {{1, 2}, {15, 16}, {16, 17}, {17, 48}, {4099, 4100}, {20000, 30000}, {81920, 81937}};
    const uint64_t at = 12345, size = 40000;
    for (uint32_t res = 0; res < 16; res += 5)
        for (const uint64_t *pat : pats)
            for (uint64_t offset : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)30000}) {
                Slice s = {offset, pat[0], pat[1], (at + size + pat[0] - 1) / pat[0]};
                const uint64_t hull = (s.count - 1) * s.stride + s.run;
                uint64_t bytes;
                snprintf(g_case, sizeof(g_case), "frag res=%u run=%llu stride=%llu offset=%llu", res, (unsigned long long)pat[0],
                         (unsigned long long)pat[1], (unsigned long long)offset);
                if (!slice_check(s, offset + hull, &bytes) || bytes < at + size) return fail();
                Range buf(res, offset + hull);
                std::vector<uint8_t> want(size);
                for (uint64_t i = 0; i < size; i++) want[i] = buf.p[defined(s, at + i)];
                std::vector<PieceSums> sums;
                for (uint64_t off = 0; off < size; off += kFragPiece) {
                    GatherCut c;
                    const uint32_t len = (uint32_t)(size - off < kFragPiece ? size - off : kFragPiece);
                    const bool whole = gather_reduce(s, at + off, len, c);
                    sums.push_back(run_piece<PLANT, false>(whole ? GatherPiece{buf.p + c.src, nullptr, 0, len, 0, 0, 0, nullptr, nullptr}
                                                                 : GatherPiece{buf.p + c.src, nullptr, c.stride, len, c.phase, c.run, 0, buf.p + offset,
                                                                               buf.p + offset + hull}));
                }
                const PieceSums *sp = sums.data();
                if (fold_pieces([sp](uint32_t k) { return sp[k]; }, (uint32_t)sums.size(), size) != adler32_bytes(want.data(), size)) return fail();
                ncases++;
            }
    return 0;
}

template <int PLANT>
static int run_all()
{
    uint64_t ncases = 0;
    if (part1<PLANT>(ncases) || part2<PLANT>(ncases)) return 1;
    printf("ok %llu\n", (unsigned long long)ncases);
    return 0;
}

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    switch (plant) {
    case kGPlantNone: return run_all<kGPlantNone>();
    case kGPlantWindowPastHull: return run_all<kGPlantWindowPastHull>();
    case kGPlantSumTailDropped: return run_all<kGPlantSumTailDropped>();
    case kGPlantSumStillStores: return run_all<kGPlantSumStillStores>();
    }
    return 2;
}
