// csa_dev_gather_model.cpp -- gather_whole, gather_reduce and gather_sum of csc_amd/csrc/csa_dev_write.h (the text the host planner
// of CSAMI_DeviceWriteSlices and k_frag_rows run) on the CPU, thread by thread, under AddressSanitizer and UBSan
// (tests/test_archive_gather_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_gather_model PLANT     PLANT = 0: the text the kernel runs; 1..5: one of the header's planted mistakes switched on
//
// Part 1, gather_reduce against the 64-bit definition -- packed byte p lies at buffer offset offset + (p / run) * stride + p % run:
// run and stride out of kBig (stride >= run), the largest count <= 3 that fits in 64 bits, offset 5; pieces of 1, 16 and 16384
// bytes (clipped to the entry's end) that begin, in the first and the last row, at the run's start, in its middle and at its last
// byte, and exactly on the border behind the row.  For every byte of the piece the definition is compared with what the cut says; a
// periodic cut must hold 32-bit quantities within the bounds the header states, and leave a pattern that fits as it is.
// Part 2, gather_sum: alignment of period position 0 of the source 0..15 x alignment of the destination 0..15 x kLens x kPatterns.
// The source is a heap block that is EXACTLY the hull of the rows the piece meets (it begins `alignment` bytes into its allocation,
// poisoned in front as far as ASan's 8-byte granules allow, and ends where the allocation ends), so a load outside the hull is the
// sanitizer's to report; gap bytes are random like the others, so one that is taken shows.  The destination holds exactly the
// piece between two canaries of 32 bytes.  All kThreads thread ids are run.  Expected: a packed copy made with a plain loop, and
// A = sum(b_i), B = sum((len - i) * b_i) over it.
// Part 3, a fragment of 40000 packed bytes at packed offset 12345 of its entry under a few slices, the buffer exactly offset + hull
// bytes: gather_reduce per 16 KiB cell, the piece run as k_frag_rows runs it, fold_pieces -- against the definition's packed copy
// and a byte-at-a-time adler32.
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

// the definition: the buffer offset of packed byte p
static uint64_t defined(const Slice &s, uint64_t p) { return s.offset + (p / s.run) * s.stride + p % s.run; }

static const uint64_t kBig[] = {1, 2, 15, 16, 17, 16383, 16384, 16385, 1ull << 31, 1ull << 32, 1ull << 63};
static const uint32_t kSpans[] = {1, 16, 16384};

static int check_reduce(const Slice &s, uint64_t at, uint32_t len)
{
    GatherCut c;
    uint64_t src;
    const bool whole = gather_reduce(s, at, len, c);
    if (whole != gather_whole(s, at, len, &src) || whole != (at / s.run == (at + len - 1) / s.run)) return 1;
    if (whole) {
        if (c.src != src || c.stride || c.run || c.phase) return 1;
        for (uint32_t i = 0; i < len; i++)
            if (c.src + i != defined(s, at + i)) return 1;
        return 0;
    }
    if (!(c.run >= 1 && c.run <= kFragPiece && c.stride >= c.run && c.phase < c.run && (uint64_t)c.phase + len < 65536)) return 1;
    if (s.run <= kFragPiece && (c.run != s.run || c.stride != s.stride)) return 1;
    if (c.src < s.offset) return 1;                                   // period position 0 lies inside the hull
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t pos = c.phase + i, row = pos / c.run, r = pos % c.run;
        if (c.src + row * c.stride + r != defined(s, at + i)) return 1;
    }
    return 0;
}

static int part1(uint64_t &ncases)
{
    static const char *const kinds[] = {"start", "middle", "last", "border"};
    for (uint64_t run : kBig)
        for (uint64_t stride : kBig) {
            if (stride < run) continue;
            Slice s = {5, run, stride, 0};
            uint64_t total = 0;
            for (uint64_t count = 3; count >= 1; count--) {
                Slice t = {5, run, stride, count};
                if (slice_check(t, UINT64_MAX, &total)) { s = t; break; }
            }
            if (!s.count) { snprintf(g_case, sizeof(g_case), "reduce run=%llu stride=%llu: no count fits", (unsigned long long)run, (unsigned long long)stride); return fail(); }
            for (uint32_t span : kSpans)
                for (uint64_t row : {(uint64_t)0, s.count - 1})
                    for (int kind = 0; kind < 4; kind++) {
                        const uint64_t at = row * run + (kind == 0 ? 0 : kind == 1 ? run / 2 : kind == 2 ? run - 1 : run);
                        if (at >= total) continue;                   // (the border behind the last row is the entry's end)
                        const uint32_t len = (uint32_t)(total - at < span ? total - at : span);
                        snprintf(g_case, sizeof(g_case), "reduce run=%llu stride=%llu count=%llu len=%u row=%llu at=%s", (unsigned long long)run,
                                 (unsigned long long)stride, (unsigned long long)s.count, len, (unsigned long long)row, kinds[kind]);
                        if (check_reduce(s, at, len)) return fail();
                        ncases++;
                    }
        }
    return 0;
}

static const uint32_t kLens[] = {1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384};
static const uint32_t kPatterns[][2] = {{1, 2}, {1, 16}, {3, 5}, {15, 16}, {16, 16}, {16, 17}, {17, 48}, {100, 1000}, {4096, 4097}, {16384, 16384},
                                        {7, 11}, {16, 33}, {4097, 8197}};
static const uint32_t kCanary = 32;

// every thread of the workgroup over one piece, as k_frag_rows runs it
template <int PLANT>
static PieceSums run_piece(const GatherPiece &pc)
{
    PieceSums s = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        if (pc.stride) gather_sum<PLANT>(pc, tid, kThreads, s.a, s.b);
        else copy_sum<true, true>(pc.dst, pc.src, pc.len, tid, kThreads, s.a, s.b);
    }
    return s;
}

template <int PLANT>
static int part2(uint64_t &ncases)
{
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t da = 0; da < 16; da++)
            for (uint32_t n : kLens)
                for (const uint32_t *pat : kPatterns) {
                    const uint32_t run = pat[0], stride = pat[1], phase = (7 * sa + 3 * da + n) % run;
                    snprintf(g_case, sizeof(g_case), "sum sa=%u da=%u n=%u run=%u stride=%u", sa, da, n, run, stride);
                    const uint32_t rows = (phase + n - 1) / run + 1;
                    const uint64_t hull = (uint64_t)(rows - 1) * stride + run;
                    Range src(sa, hull);
                    const size_t total = kCanary + 16 + n + kCanary;
                    std::vector<uint8_t> expect(total, 0xC3);
                    uint64_t wa = 0, wb = 0;
                    for (uint32_t i = 0; i < n; i++) {                // the packed copy, with a plain loop, and its sums
                        const uint8_t v = src.p[(uint64_t)((phase + i) / run) * stride + (phase + i) % run];
                        expect[kCanary + da + i] = v;
                        wa += v;
                        wb += (uint64_t)(n - i) * v;
                    }
                    uint8_t *got = (uint8_t *)malloc(total);
                    if (((uintptr_t)got & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
                    memset(got, 0xC3, total);
                    const GatherPiece pc = {src.p, got + kCanary + da, stride, n, phase, run, 0, src.p, src.p + hull};
                    const PieceSums s = run_piece<PLANT>(pc);
                    const bool bad = s.a != wa || s.b != wb || memcmp(got, expect.data(), total) != 0;
                    free(got);
                    if (bad) return fail();
                    ncases++;
                }
    return 0;
}

template <int PLANT>
static int part3(uint64_t &ncases)
{
    static const uint64_t pats[][2] = {{3, 5}, {7, 11}, {100, 1000}, {4096, 4097}, {16384, 16384}, {20000, 30000}, {81920, 81937}};
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
                std::vector<uint8_t> want(kCanary + size + kCanary, 0xC3), got(want);
                for (uint64_t i = 0; i < size; i++) want[kCanary + i] = buf.p[defined(s, at + i)];
                std::vector<PieceSums> sums;
                for (uint64_t off = 0; off < size; off += kFragPiece) {
                    GatherCut c;
                    const uint32_t len = (uint32_t)(size - off < kFragPiece ? size - off : kFragPiece);
                    const bool whole = gather_reduce(s, at + off, len, c);
                    uint8_t *dst = got.data() + kCanary + off;
                    sums.push_back(run_piece<PLANT>(whole ? GatherPiece{buf.p + c.src, dst, 0, len, 0, 0, 0, nullptr, nullptr}
                                                          : GatherPiece{buf.p + c.src, dst, c.stride, len, c.phase, c.run, 0, buf.p + offset,
                                                                        buf.p + offset + hull}));
                }
                const PieceSums *sp = sums.data();
                if (got != want || fold_pieces([sp](uint32_t k) { return sp[k]; }, (uint32_t)sums.size(), size) != adler32_bytes(want.data() + kCanary, size))
                    return fail();
                ncases++;
            }
    return 0;
}

template <int PLANT>
static int run_all()
{
    uint64_t ncases = 0;
    if (part1(ncases) || part2<PLANT>(ncases) || part3<PLANT>(ncases)) return 1;
    printf("ok %llu\n", (unsigned long long)ncases);
    return 0;
}

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    switch (plant) {
    case kGPlantNone: return run_all<kGPlantNone>();
    case kGPlantBorderLate: return run_all<kGPlantBorderLate>();
    case kGPlantPhaseDropped: return run_all<kGPlantPhaseDropped>();
    case kGPlantStraddleContiguous: return run_all<kGPlantStraddleContiguous>();
    case kGPlantRowNotAdvanced: return run_all<kGPlantRowNotAdvanced>();
    case kGPlantWindowPastHull: return run_all<kGPlantWindowPastHull>();
    }
    return 2;
}
