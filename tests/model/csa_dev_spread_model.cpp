// csa_dev_spread_model.cpp -- spread_sum and compare_rows of csc_amd/csrc/csa_dev_read.h (the text k_frag_spread and
// k_frag_compare_rows run), planned as the host plans them with gather_reduce of csc_amd/csrc/csa_dev_write.h, on the CPU, thread
// by thread, under AddressSanitizer and UBSan (tests/test_archive_spread_host.py builds and runs it; a program of its own, nothing
// is preloaded).
//
//   csa_dev_spread_model PLANT     PLANT = 0: the text the kernels run; 13..18: one of the header's planted mistakes switched on
//
// A case is a piece of n packed bytes that begins r0 bytes into a run of a slice {0, run, run + gap, count} of the caller's buffer,
// count just large enough to hold it, cut by gather_reduce exactly as the planner cuts it (a run above kFragPiece is reduced, a piece
// inside one run is a plain one).  kRuns x kGaps x kLens x the phases that put the first run border into the piece's head (byte 1),
// into a 16-byte unit (5 bytes behind the head), onto a unit's edge and into its tail (byte n - 1) x alignment of the source 0..15
// x alignment of the hull 0..15; where the hull is larger than kFullHull only one hull alignment per source alignment is run.
// The source is a heap block of exactly n bytes, `alignment` bytes into its allocation -- poisoned in front as far as ASan's 8-byte
// granules allow -- that ends where the allocation ends, and the caller's buffer is exactly the hull laid out the same way: a load
// window that leaves the piece, and a load or a store that leaves the hull, are the sanitizer's to report.
// Part 1, spread_sum: the hull is 0xA5 everywhere; all kThreads thread ids are run; expected is the hull with the piece's bytes at
// the places the definition gives them -- offset + (p / run) * stride + p % run -- and 0xA5 in every gap byte, in front of the piece
// and behind it, and in the guard bytes in front of the hull; the sums are copy_sum<false, true>'s over the source.
// Part 2, compare_rows: the hull holds the piece's bytes at their places and random bytes everywhere else, so a gap byte that is
// compared shows as a difference; expected is no difference and the same sums.  For one hull alignment per source alignment a
// difference is then planted at each position class in turn -- byte 0, the head's last byte, the first unit's first byte, the first
// byte behind a run border inside a unit, the last unit's last byte, byte n - 1 -- and must be found exactly there, and one in a gap
// byte and in the bytes in front of and behind the piece, where it must not be seen.
// Part 3, compare_rows with a summed tail: cmp < len.
// Part 4, a fragment of 40000 packed bytes at packed offset 12345 of its entry under a few slices, runs above a piece included:
// gather_reduce per 16 KiB cell, the piece run as k_frag_spread runs it, fold_pieces -- against the definition and a
// byte-at-a-time adler32.
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

static char g_case[200] = "start";
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

struct Range {                 // `n` bytes at alignment `al`, ending exactly where their allocation ends; 0xA5 in the al bytes in front
    uint8_t *base, *p;
    uint32_t al;
    Range(uint32_t al_, uint64_t n, const uint8_t *image) : al(al_)
    {
        base = (uint8_t *)malloc(al + n ? al + n : 1);
        if (((uintptr_t)base & 15u) != 0) { fprintf(stderr, "malloc is not 16-byte aligned\n"); exit(2); }
        p = base + al;
        memset(base, 0xA5, al);
        if (image) memcpy(p, image, n); else memset(p, 0xA5, n);
        __asan_poison_memory_region(base, al & ~7u);
    }
    bool guard_ok() const
    {
        for (uint32_t i = al & ~7u; i < al; i++)
            if (base[i] != 0xA5) return false;
        return true;
    }
    ~Range() { __asan_unpoison_memory_region(base, al); free(base); }
};

// the definition: the buffer offset of packed byte p
static uint64_t defined(const Slice &s, uint64_t p) { return s.offset + (p / s.run) * s.stride + p % s.run; }

static const uint32_t kRuns[] = {1, 3, 7, 15, 16, 17, 31, 33, 4097, 16384, 16385};
static const uint32_t kGaps[] = {0, 1, 13, 4099};
static const uint32_t kLens[] = {1, 15, 16, 17, 4095, 16383, 16384};
static const uint64_t kFullHull = 65536;

// the piece [at, at + n) of the packed bytes under s, of which the first `cmp` are compared, as FragTables::add_spread plans it
static SpreadPiece plan(const Slice &s, uint64_t at, uint32_t n, uint32_t cmp, const uint8_t *src, uint8_t *buf, bool compare)
{
    const uint8_t *lo = buf + s.offset, *hi = lo + (s.count - 1) * s.stride + s.run;
    SpreadPiece sp = {src, nullptr, 0, n, 0, 0, 0, nullptr, nullptr};
    GatherCut c;
    const bool whole = gather_reduce(s, at, cmp, c);
    sp.dst = buf + c.src;
    sp.cmp = compare ? cmp : 0;
    if (!whole) { sp.stride = c.stride; sp.phase = c.phase; sp.run = c.run; sp.lo = lo; sp.hi = hi; }
    return sp;
}

// every thread of the workgroup over one piece, as k_frag_spread runs it
template <int PLANT>
static PieceSums run_spread(const SpreadPiece &pc)
{
    PieceSums s = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        if (pc.stride) spread_sum<PLANT>(pc, tid, kThreads, s.a, s.b);
        else if (pc.dst == nullptr) copy_sum<false, true>(nullptr, pc.src, pc.len, tid, kThreads, s.a, s.b);
        else copy_sum<true, true>(pc.dst, pc.src, pc.len, tid, kThreads, s.a, s.b);
    }
    return s;
}

// ... as k_frag_compare_rows runs it: the workgroup's smallest `first`
template <int PLANT>
static PieceSums run_rows(const SpreadPiece &pc, uint32_t &first)
{
    PieceSums s = {0, 0};
    first = pc.len;
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        uint32_t f;
        if (pc.stride) compare_rows<PLANT>(pc, tid, kThreads, s.a, s.b, f);
        else compare_piece<PLANT>(pc.src, pc.dst, pc.len, pc.dst ? pc.cmp : 0u, tid, kThreads, s.a, s.b, f);
        if (f < first) first = f;
    }
    return s;
}

static PieceSums plain_sums(const uint8_t *src, uint32_t n)        // copy_sum<false, true>'s, and the formula they stand for
{
    PieceSums s = {0, 0}, w = {0, 0};
    for (uint32_t tid = 0; tid < kThreads; tid++) copy_sum<false, true>(nullptr, src, n, tid, kThreads, s.a, s.b);
    for (uint32_t i = 0; i < n; i++) { w.a += src[i]; w.b += (uint64_t)(n - i) * src[i]; }
    if (s.a != w.a || s.b != w.b) { fprintf(stderr, "copy_sum<false, true> is not the formula\n"); exit(2); }
    return s;
}

// the phases of a case: r0, the piece's first byte's place in its run, so that the first run border falls behind byte `want` - 1
static std::vector<uint32_t> phases(uint32_t run, uint32_t n, uint32_t sa)
{
    const uint32_t head = (0u - sa) & 15u;
    std::vector<uint32_t> out;
    for (uint32_t want : {1u, head + 5u, head + 16u, n - 1u}) {
        const uint32_t r0 = (run - want % run) % run;
        bool seen = false;
        for (uint32_t o : out) seen = seen || o == r0;
        if (!seen) out.push_back(r0);
    }
    return out;
}

template <int PLANT>
static int parts12(uint64_t &ncases)
{
    std::vector<uint8_t> want, image;
    for (uint32_t run : kRuns)
        for (uint32_t gap : kGaps)
            for (uint32_t n : kLens)
                for (uint32_t sa = 0; sa < 16; sa++)
                    for (uint32_t r0 : phases(run, n, sa)) {
                        Slice s = {0, run, (uint64_t)run + gap, ((uint64_t)r0 + n + run - 1) / run};
                        const uint64_t at = r0;
                        uint64_t bytes;
                        const bool checked = slice_check(s, UINT64_MAX, &bytes);
                        const uint64_t hull = (s.count - 1) * s.stride + s.run;
                        snprintf(g_case, sizeof(g_case), "plan sa=%u n=%u run=%u gap=%u r0=%u", sa, n, run, gap, r0);
                        if (!checked || bytes < at + n) return fail();
                        Range src(sa, n, nullptr);
                        for (uint32_t i = 0; i < n; i++) src.p[i] = next_byte();
                        const PieceSums sums = plain_sums(src.p, n);
                        const uint32_t head = ((0u - sa) & 15u) < n ? (0u - sa) & 15u : n, units = (n - head) >> 4;
                        // part 1: the hull 0xA5 with the piece at its places
                        want.assign(hull, 0xA5);
                        for (uint32_t i = 0; i < n; i++) want[defined(s, at + i)] = src.p[i];
                        // part 2: the piece at its places among random bytes
                        image.resize(hull);
                        for (uint64_t i = 0; i < hull; i++) image[i] = next_byte();
                        for (uint32_t i = 0; i < n; i++) image[defined(s, at + i)] = src.p[i];
                        for (uint32_t da = 0; da < 16; da++) {
                            const bool chosen = da == (5 * sa + n) % 16;
                            if (hull > kFullHull && !chosen) continue;
                            {
                                snprintf(g_case, sizeof(g_case), "spread sa=%u da=%u n=%u run=%u gap=%u r0=%u", sa, da, n, run, gap, r0);
                                Range dst(da, hull, nullptr);
                                const PieceSums got = run_spread<PLANT>(plan(s, at, n, n, src.p, dst.p, false));
                                if (got.a != sums.a || got.b != sums.b || memcmp(dst.p, want.data(), hull) != 0 || !dst.guard_ok()) return fail();
                                ncases++;
                            }
                            snprintf(g_case, sizeof(g_case), "rows sa=%u da=%u n=%u run=%u gap=%u r0=%u", sa, da, n, run, gap, r0);
                            Range y(da, hull, image.data());
                            const SpreadPiece pc = plan(s, at, n, n, src.p, y.p, true);
                            uint32_t first;
                            PieceSums got = run_rows<PLANT>(pc, first);
                            if (got.a != sums.a || got.b != sums.b || first != n || memcmp(y.p, image.data(), hull) != 0) return fail();
                            ncases++;
                            if (!chosen) continue;
                            // a difference at each position class
                            uint32_t straddle = n;                   // the first byte behind a run border inside a unit
                            for (uint32_t u = 0; u < units && straddle == n; u++)
                                for (uint32_t j = 1; j < 16; j++)
                                    if ((at + head + 16 * u + j) % run == 0) { straddle = head + 16 * u + j; break; }
                            const uint32_t cls[6] = {0, head ? head - 1 : n, units ? head : n, straddle, units ? head + 16 * units - 1 : n, n - 1};
                            static const char *const names[6] = {"byte 0", "head end", "unit start", "behind a border", "unit end", "last byte"};
                            for (int k = 0; k < 6; k++) {
                                if (cls[k] >= n) continue;
                                snprintf(g_case, sizeof(g_case), "diff %s sa=%u da=%u n=%u run=%u gap=%u r0=%u", names[k], sa, da, n, run, gap, r0);
                                uint8_t &b = y.p[defined(s, at + cls[k])];
                                b ^= 0x40;
                                got = run_rows<PLANT>(pc, first);
                                b ^= 0x40;
                                if (got.a != sums.a || got.b != sums.b || first != cls[k]) return fail();
                                ncases++;
                            }
                            // ... and where it must not be seen: a gap byte, the byte in front of the piece, the byte behind it
                            const uint64_t unseen[3] = {gap && s.count > 1 ? (uint64_t)run : hull, r0 ? (uint64_t)r0 - 1 : hull,
                                                        defined(s, at + n - 1) + 1};
                            for (int k = 0; k < 3; k++) {
                                if (unseen[k] >= hull) continue;
                                snprintf(g_case, sizeof(g_case), "unseen %d sa=%u da=%u n=%u run=%u gap=%u r0=%u", k, sa, da, n, run, gap, r0);
                                y.p[unseen[k]] ^= 0x40;
                                got = run_rows<PLANT>(pc, first);
                                y.p[unseen[k]] ^= 0x40;
                                if (got.a != sums.a || got.b != sums.b || first != n) return fail();
                                ncases++;
                            }
                        }
                    }
    return 0;
}

template <int PLANT>
static int part3(uint64_t &ncases)
{
    static const uint32_t pats[][2] = {{3, 5}, {16, 17}, {33, 46}, {4097, 4110}};
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t cmp : {1u, 15u, 16u, 17u, 4095u})
            for (uint32_t extra : {1u, 16u, 300u})
                for (const uint32_t *pat : pats) {
                    const uint32_t len = cmp + extra, r0 = pat[0] - 1, da = (3 * sa + cmp) % 16;
                    snprintf(g_case, sizeof(g_case), "tail sa=%u cmp=%u len=%u run=%u", sa, cmp, len, pat[0]);
                    Slice s = {0, pat[0], pat[1], ((uint64_t)r0 + cmp + pat[0] - 1) / pat[0]};
                    uint64_t bytes;
                    if (!slice_check(s, UINT64_MAX, &bytes)) return fail();
                    const uint64_t hull = (s.count - 1) * s.stride + s.run;
                    Range src(sa, len, nullptr);
                    for (uint32_t i = 0; i < len; i++) src.p[i] = next_byte();
                    const PieceSums sums = plain_sums(src.p, len);
                    std::vector<uint8_t> image(hull);
                    for (uint64_t i = 0; i < hull; i++) image[i] = next_byte();
                    for (uint32_t i = 0; i < cmp; i++) image[defined(s, r0 + i)] = src.p[i];
                    Range y(da, hull, image.data());
                    SpreadPiece pc = plan(s, r0, cmp, cmp, src.p, y.p, true);
                    pc.len = len;
                    uint32_t first;
                    PieceSums got = run_rows<PLANT>(pc, first);
                    if (got.a != sums.a || got.b != sums.b || first != len) return fail();
                    y.p[defined(s, r0 + cmp - 1)] ^= 1;
                    got = run_rows<PLANT>(pc, first);
                    if (got.a != sums.a || got.b != sums.b || first != cmp - 1) return fail();
                    ncases++;
                }
    return 0;
}

template <int PLANT>
static int part4(uint64_t &ncases)
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
                Range frag(res, size, nullptr);
                for (uint64_t i = 0; i < size; i++) frag.p[i] = next_byte();
                std::vector<uint8_t> want(offset + hull, 0xA5);
                for (uint64_t i = 0; i < size; i++) want[defined(s, at + i)] = frag.p[i];
                Range buf((res + 7) % 16, offset + hull, nullptr);
                std::vector<PieceSums> sums;
                for (uint64_t off = 0; off < size; off += kFragPiece) {
                    const uint32_t len = (uint32_t)(size - off < kFragPiece ? size - off : kFragPiece);
                    sums.push_back(run_spread<PLANT>(plan(s, at + off, len, len, frag.p + off, buf.p, false)));
                }
                const PieceSums *sp = sums.data();
                if (memcmp(buf.p, want.data(), offset + hull) != 0 || !buf.guard_ok()
                    || fold_pieces([sp](uint32_t k) { return sp[k]; }, (uint32_t)sums.size(), size) != adler32_bytes(frag.p, size))
                    return fail();
                ncases++;
            }
    return 0;
}

template <int PLANT>
static int run_all()
{
    uint64_t ncases = 0;
    if (parts12<PLANT>(ncases) || part3<PLANT>(ncases) || part4<PLANT>(ncases)) return 1;
    printf("ok %llu\n", (unsigned long long)ncases);
    return 0;
}

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    switch (plant) {
    case kPlantNone: return run_all<kPlantNone>();
    case kPlantSpreadBorderLate: return run_all<kPlantSpreadBorderLate>();
    case kPlantSpreadPhaseDropped: return run_all<kPlantSpreadPhaseDropped>();
    case kPlantSpreadStraddleWhole: return run_all<kPlantSpreadStraddleWhole>();
    case kPlantSpreadRowNotAdvanced: return run_all<kPlantSpreadRowNotAdvanced>();
    case kPlantRowsWindowPastHull: return run_all<kPlantRowsWindowPastHull>();
    case kPlantRowsHeadNotCompared: return run_all<kPlantRowsHeadNotCompared>();
    }
    return 2;
}
