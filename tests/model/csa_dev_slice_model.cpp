// csa_dev_slice_model.cpp -- slice_check, slice_next, slice_reduce and slice_sum of csc_amd/csrc/csa_dev_read.h (the text the host
// planner of CSAMI_DeviceReadSlices and k_frag_slices run) on the CPU, thread by thread, under AddressSanitizer and UBSan
// (tests/test_archive_slices_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_slice_model PLANT     PLANT = 0: the text the kernel runs; 9..12: one of the header's planted mistakes switched on
//
// Part 1, slice_reduce against the 64-bit definition: run and stride out of kBig (stride >= run), the largest count <= 3 that fits
// in 64 bits, offset 5; pieces of 1, 16 and 16384 bytes that begin 3 bytes in front of the slice, and in the first and the last row
// inside the run, at its last byte, in the gap and at the gap's last byte.  For every byte of the piece the definition -- selected
// when (e - offset) / stride < count and (e - offset) % stride < run, stored to packed offset row * run + r -- is compared with what
// the cut says; a kSlicePeriodic cut must hold 32-bit quantities within the bounds the header states.
// Part 2, slice_sum: alignment of the source 0..15 x alignment of the first stored byte 0..15 x kLens x kPatterns x three [lo, hi).
// The source is a heap block that ENDS exactly where the piece ends (and begins `alignment` bytes in front of it, poisoned as far as
// ASan's 8-byte granules allow), so a load outside it is the sanitizer's to report.  The destination holds exactly the selected
// bytes between two canaries of 32 bytes.  All kThreads thread ids are run.  Expected: the sums of copy_sum<false, true>, and a byte-
// by-byte gather.
// Part 3, a fragment of 40000 bytes at offset 12345 of its entry under a few slices: piece_split, slice_reduce, the piece run as
// k_frag_slices runs it, fold_pieces -- against the definition's gather and a byte-at-a-time adler32.
//
// The first case that fails is named on a line "FAIL <case>"; when a sanitizer ends the run, the case it happened in is named on
// a line "AT <case>".  Exit status 0 only if every case passed.
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csa_dev_read.h"

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

struct Range {                 // `n` bytes at alignment `al`, ending exactly where their allocation ends
    uint8_t *base, *p;
    uint32_t al;
    Range(uint32_t al_, uint64_t n) : al(al_)
    {
        base = (uint8_t *)malloc(al + n ? al + n : 1);
        if (((uintptr_t)base & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
        p = base + al;
        memset(base, 0xA5, al);
        __asan_poison_memory_region(base, al & ~7u);
    }
    ~Range() { __asan_unpoison_memory_region(base, al); free(base); }
};

// the definition: is byte e of the entry selected, and where does it go
static bool defined(const Slice &s, uint64_t e, uint64_t *packed)
{
    if (!s.count || e < s.offset) return false;
    const uint64_t t = e - s.offset, row = t / s.stride, r = t % s.stride;
    if (row >= s.count || r >= s.run) return false;
    *packed = row * s.run + r;
    return true;
}

static const uint64_t kBig[] = {1, 2, 15, 16, 17, 16383, 16384, 16385, 1ull << 31, 1ull << 32, 1ull << 63};
static const uint32_t kSpans[] = {1, 16, 16384};

static int check_reduce(const Slice &s, uint64_t at, uint32_t len)
{
    SliceCut c;
    const SliceKind kind = slice_reduce(s, at, len, c);
    uint64_t nsel = 0, first = 0, last = 0, packed = 0, first_at = 0;
    for (uint32_t p = 0; p < len; p++)
        if (defined(s, at + p, &packed)) { if (!nsel++) { first = packed; first_at = at + p; } last = packed; }
    const uint64_t next = slice_next(s, at);                         // O(1): the planner's test for "touched"
    if (nsel ? next != first_at : next < at + len) return 1;
    if (kind == kSliceNone) return nsel != 0;
    if (!nsel) return 1;
    if (kind == kSliceWhole) return !(nsel == len && c.dst == first && last - first == len - 1);
    if (!(c.lo < c.hi && c.hi <= len && c.run >= 1 && c.run <= c.stride && c.stride <= 2 * kFragPiece && c.phase < c.stride
          && (uint64_t)c.phase + len < 65536)) return 1;
    for (uint32_t p = 0; p < len; p++) {
        const uint32_t pos = c.phase + p, row = pos / c.stride, r = pos % c.stride;
        const bool sel = p >= c.lo && p < c.hi && r < c.run;
        if (sel != defined(s, at + p, &packed)) return 1;
        if (sel && c.dst + (uint64_t)row * c.run + r != packed) return 1;
    }
    return 0;
}

static int part1(uint64_t &ncases)
{
    static const char *const kinds[] = {"front", "run", "runlast", "gap", "gaplast"};
    for (uint64_t run : kBig)
        for (uint64_t stride : kBig) {
            if (stride < run) continue;
            Slice s = {5, run, stride, 0};
            uint64_t bytes = 0;
            for (uint64_t count = 3; count >= 1; count--) {
                Slice t = {5, run, stride, count};
                if (slice_check(t, UINT64_MAX, &bytes)) { s = t; break; }
            }
            if (!s.count) { snprintf(g_case, sizeof(g_case), "reduce run=%llu stride=%llu: no count fits", (unsigned long long)run, (unsigned long long)stride); return fail(); }
            for (uint32_t len : kSpans)
                for (uint64_t row : {(uint64_t)0, s.count - 1})
                    for (int kind = 0; kind < 5; kind++) {
                        if (kind == 0 && row) continue;
                        if (kind >= 3 && stride == run) continue;
                        const uint64_t r0 = kind == 1 ? run / 2 : kind == 2 ? run - 1 : kind == 3 ? run + (stride - run) / 2 : stride - 1;
                        const uint64_t base = s.offset + row * s.stride;
                        if (kind && r0 > UINT64_MAX - len - base) continue;                  // (the piece would pass 2^64)
                        const uint64_t at = kind ? base + r0 : s.offset - 3;
                        snprintf(g_case, sizeof(g_case), "reduce run=%llu stride=%llu count=%llu len=%u row=%llu at=%s", (unsigned long long)run,
                                 (unsigned long long)stride, (unsigned long long)s.count, len, (unsigned long long)row, kinds[kind]);
                        if (check_reduce(s, at, len)) return fail();
                        ncases++;
                    }
        }
    // what slice_check refuses, and the two it must not
    snprintf(g_case, sizeof(g_case), "check");
    struct { Slice s; uint64_t size; bool ok; } checks[] = {
        {{0, 0, 0, 0}, 0, true}, {{7, 0, 0, 0}, 0, true}, {{0, 0, 1, 1}, 10, false}, {{0, 2, 1, 2}, 10, false}, {{0, 2, 2, 2}, 4, true},
        {{0, 2, 2, 2}, 3, false}, {{9, 1, 0, 1}, 10, true}, {{10, 1, 0, 1}, 10, false}, {{1, UINT64_MAX, 0, 1}, UINT64_MAX, false},
        {{0, 1, 1ull << 63, 3}, UINT64_MAX, false}, {{UINT64_MAX, 1, 0, 1}, UINT64_MAX, false}, {{0, 3, 5, 2}, 8, true}, {{0, 3, 5, 2}, 7, false}};
    for (auto &k : checks) {
        uint64_t bytes;
        if (slice_check(k.s, k.size, &bytes) != k.ok || (k.ok && bytes != (k.s.count ? k.s.run * k.s.count : 0))) return fail();
        ncases++;
    }
    return 0;
}

static const uint32_t kLens[] = {1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384};
static const uint32_t kPatterns[][2] = {{1, 2}, {1, 16}, {3, 5}, {15, 16}, {16, 16}, {16, 17}, {17, 48}, {100, 1000}, {4096, 4097}, {16384, 16384}};
static const uint32_t kCanary = 32;

// every thread of the workgroup over one periodic piece, as k_frag_slices runs it
template <int PLANT>
static PieceSums run_slice(const SlicePiece &pc)
{
    PieceSums s = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) slice_sum<PLANT>(pc, tid, kThreads, s.a, s.b);
    return s;
}

static PieceSums run_sum(const uint8_t *src, uint32_t n)
{
    PieceSums s = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) copy_sum<false, true>(nullptr, src, n, tid, kThreads, s.a, s.b);
    return s;
}

template <int PLANT>
static int part2(uint64_t &ncases)
{
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t da = 0; da < 16; da++)
            for (uint32_t n : kLens)
                for (const uint32_t *pat : kPatterns)
                    for (int cut = 0; cut < 3; cut++) {
                        const uint32_t lo = cut == 0 ? 0 : cut == 1 ? 1 : n / 3, hi = cut == 0 ? n : cut == 1 ? n - 1 : n - n / 3;
                        if (lo >= hi) continue;
                        const uint32_t run = pat[0], stride = pat[1], phase = (7 * sa + 3 * da + n) % stride;
                        snprintf(g_case, sizeof(g_case), "sum sa=%u da=%u n=%u run=%u stride=%u lo=%u hi=%u", sa, da, n, run, stride, lo, hi);
                        Range src(sa, n);
                        for (uint32_t i = 0; i < n; i++) src.p[i] = next_byte();
                        // the gather, byte by byte: the selected bytes' packed offsets are consecutive
                        std::vector<uint8_t> want;
                        uint32_t first = 0;
                        for (uint32_t i = lo; i < hi; i++) {
                            const uint32_t pos = phase + i, row = pos / stride, r = pos % stride;
                            if (r >= run) continue;
                            if (want.empty()) first = row * run + r;
                            if (row * run + r != first + want.size()) return fail();
                            want.push_back(src.p[i]);
                        }
                        const size_t total = kCanary + 16 + want.size() + kCanary;
                        std::vector<uint8_t> expect(total, 0xC3);
                        uint8_t *got = (uint8_t *)malloc(total);
                        if (((uintptr_t)got & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
                        memset(got, 0xC3, total);
                        if (!want.empty()) memcpy(expect.data() + kCanary + da, want.data(), want.size());
                        SlicePiece pc = {src.p, (uint8_t *)((uintptr_t)got + kCanary + da - first), n, lo, hi, phase, run, stride};
                        const PieceSums s = run_slice<PLANT>(pc), plain = run_sum(src.p, n);
                        const bool bad = s.a != plain.a || s.b != plain.b || memcmp(got, expect.data(), total) != 0;
                        free(got);
                        if (bad) return fail();
                        ncases++;
                    }
    return 0;
}

template <int PLANT>
static int part3(uint64_t &ncases)
{
    static const uint64_t pats[][2] = {{3, 5}, {100, 1000}, {4096, 4097}, {16384, 16384}, {20000, 30000}, {100, 20000}, {1, 40000}};
    const uint64_t posfile = 12345, size = 40000, entry = 100000;
    for (uint32_t res = 0; res < 16; res += 5)
        for (const uint64_t *pat : pats)
            for (uint64_t offset : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)30000}) {
                Slice s = {offset, pat[0], pat[1], (entry - offset - pat[0]) / pat[1] + 1};
                uint64_t bytes;
                snprintf(g_case, sizeof(g_case), "frag res=%u run=%llu stride=%llu offset=%llu", res, (unsigned long long)pat[0],
                         (unsigned long long)pat[1], (unsigned long long)offset);
                if (!slice_check(s, entry, &bytes)) return fail();
                Range x(res, size);
                for (uint64_t i = 0; i < size; i++) x.p[i] = next_byte();
                std::vector<uint8_t> want(kCanary + bytes + kCanary, 0xC3), got(want);
                uint64_t packed;
                for (uint64_t i = 0; i < size; i++)
                    if (defined(s, posfile + i, &packed)) want[kCanary + packed] = x.p[i];
                std::vector<PieceSums> sums;
                piece_split(x.p, nullptr, size, kFragPiece, [&](uint64_t k, const CopyPiece &p) {
                    SliceCut c;
                    const SliceKind kind = slice_reduce(s, posfile + k * kFragPiece, p.len, c);
                    uint8_t *dst = (uint8_t *)((uintptr_t)got.data() + kCanary + c.dst);
                    PieceSums ps = {0, 0};
                    if (kind == kSlicePeriodic) {
                        ps = run_slice<PLANT>(SlicePiece{p.src, dst, p.len, c.lo, c.hi, c.phase, c.run, c.stride});
                    } else {
                        for (uint32_t tid = 0; tid < kThreads; tid++) {
                            if (kind == kSliceWhole) copy_sum<true, true>(dst, p.src, p.len, tid, kThreads, ps.a, ps.b);
                            else copy_sum<false, true>(nullptr, p.src, p.len, tid, kThreads, ps.a, ps.b);
                        }
                    }
                    sums.push_back(ps);
                });
                const PieceSums *sp = sums.data();
                if (got != want || fold_pieces([sp](uint32_t k) { return sp[k]; }, (uint32_t)sums.size(), size) != adler32_bytes(x.p, size)) return fail();
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
    case kPlantNone: return run_all<kPlantNone>();
    case kPlantSliceBorderLate: return run_all<kPlantSliceBorderLate>();
    case kPlantSlicePhaseDropped: return run_all<kPlantSlicePhaseDropped>();
    case kPlantSliceStraddleWhole: return run_all<kPlantSliceStraddleWhole>();
    case kPlantSliceRowNotAdvanced: return run_all<kPlantSliceRowNotAdvanced>();
    }
    return 2;
}
