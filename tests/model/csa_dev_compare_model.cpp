// csa_dev_compare_model.cpp -- compare_sum, compare_piece and fold_first of csc_amd/csrc/csa_dev_read.h (the text k_frag_compare and
// k_frag_fold_diff run) on the CPU, thread by thread, under AddressSanitizer and UBSan (tests/test_archive_scatter_host.py builds
// and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_compare_model PLANT     PLANT = 0: the text the kernels run; 5..8: one of the header's planted mistakes switched on
//
// Part 1, compare_sum: alignment of x 0..15 x alignment of y 0..15 x the lengths below x the difference cases below.  Both ranges
// are heap buffers that END exactly where the range ends, so a load behind either is the sanitizer's to report; in front of a range
// lie only the `alignment` bytes that put it there, poisoned as far as ASan's 8-byte granules allow.  All kThreads thread ids are
// run and reduced here: the sums added, `first` by minimum.  Expected: a byte loop for the first difference, plain sums and a
// byte-at-a-time adler32 (zlib's arithmetic) for a, b and their fold.
//   difference cases (head = the bytes that bring x to a 16-byte line, clipped to n; a case whose index is not below n is left out):
//     none | 0 | head-1 | head | head+15 | head+16 | lastunit (the first byte of the last whole unit) | n-1 | two (n/3 and n-1)
// Part 2, compare_piece: a piece of which only the first `cmp` bytes are compared -- the sums are the whole piece's, a difference
// at or behind cmp is not seen, and y holds cmp bytes and not one more.
// Part 3, piece_split + compare_piece + fold_first + fold_pieces: a fragment of three pieces with a difference at 16383, 16384,
// 16385, at none, and at two of them.
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

static char g_case[128] = "start";
static void on_death() { fprintf(stderr, "AT %s\n", g_case); fflush(stderr); }

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

static int fail() { printf("FAIL %s\n", g_case); return 1; }

struct Got { uint64_t a, b; uint32_t first; };

template <bool SUM, int PLANT>
static Got run_compare(const uint8_t *x, const uint8_t *y, uint32_t n)
{
    Got g = {0, 0, n};
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        uint32_t f = 0xFFFFFFFFu;
        compare_sum<SUM, PLANT>(x, y, n, tid, kThreads, g.a, g.b, f);
        if (f > n) { g.first = 0xFFFFFFFFu; return g; }              // (a thread's `first` is an index, or n)
        if (f < g.first) g.first = f;
    }
    return g;
}

template <int PLANT>
static Got run_piece(const uint8_t *x, const uint8_t *y, uint32_t len, uint32_t cmp)
{
    Got g = {0, 0, len};
    for (uint32_t tid = 0; tid < kThreads; tid++) {
        uint32_t f = 0xFFFFFFFFu;
        compare_piece<PLANT>(x, y, len, cmp, tid, kThreads, g.a, g.b, f);
        if (f > len) { g.first = 0xFFFFFFFFu; return g; }
        if (f < g.first) g.first = f;
    }
    return g;
}

static bool sums_ok(const Got &g, const uint8_t *x, uint32_t n)
{
    uint64_t A = 0, B = 0;
    for (uint32_t i = 0; i < n; i++) { A += x[i]; B += (uint64_t)(n - i) * x[i]; }
    if (g.a != A || g.b != B) return false;
    const PieceSums s = {g.a, g.b};
    return fold_pieces([s](uint32_t) { return s; }, n ? 1 : 0, n) == adler32_bytes(x, n);
}

static uint32_t first_diff_bytes(const uint8_t *x, const uint8_t *y, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) if (x[i] != y[i]) return i;
    return n;
}

template <int PLANT>
static int run_all()
{
    static const uint32_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 255, 256, 4095, 16383, 16384};
    static const char *const kinds[] = {"none", "0", "head-1", "head", "head+15", "head+16", "lastunit", "n-1", "two"};
    uint64_t ncases = 0;
    for (uint32_t xa = 0; xa < 16; xa++)
        for (uint32_t ya = 0; ya < 16; ya++)
            for (uint32_t n : lens) {
                Range x(xa, n), y(ya, n);
                for (uint32_t i = 0; i < n; i++) x.p[i] = next_byte();
                const uint32_t head = ((16u - xa) & 15u) < n ? (16u - xa) & 15u : n, units = (n - head) >> 4;
                for (uint32_t kind = 0; kind < 9; kind++) {
                    // -1: no such index in this range
                    int64_t at[2] = {-1, -1};
                    switch (kind) {
                    case 1: at[0] = 0; break;
                    case 2: at[0] = (int64_t)head - 1; break;
                    case 3: at[0] = head; break;
                    case 4: at[0] = head + 15; break;
                    case 5: at[0] = head + 16; break;
                    case 6: at[0] = units ? (int64_t)(head + 16 * (units - 1)) : -1; break;
                    case 7: at[0] = (int64_t)n - 1; break;
                    case 8: at[0] = n >= 2 ? (int64_t)(n / 3) : -1; at[1] = (int64_t)n - 1; break;
                    }
                    if (kind && (at[0] < 0 || at[0] >= (int64_t)n)) continue;
                    snprintf(g_case, sizeof(g_case), "cmp xa=%u ya=%u n=%u diff=%s", xa, ya, n, kinds[kind]);
                    if (n) memcpy(y.p, x.p, n);
                    for (int64_t k : at) if (k >= 0) y.p[k] ^= (uint8_t)(1u << (k & 7));
                    const Got g = run_compare<true, PLANT>(x.p, y.p, n);
                    if (g.first != first_diff_bytes(x.p, y.p, n) || !sums_ok(g, x.p, n)) return fail();
                    if (kind == 0) {                                          // and without the sums: `first` alone
                        const Got h = run_compare<false, PLANT>(x.p, y.p, n);
                        if (h.first != n || h.a != 0 || h.b != 0) return fail();
                    }
                    ncases++;
                }
            }
    // Part 2: (len, cmp); y holds cmp bytes
    static const uint32_t parts[][2] = {{100, 0}, {100, 37}, {100, 100}, {4097, 4096}, {16384, 1}, {16384, 16383}, {16384, 8200}};
    for (const uint32_t *pc : parts)
        for (uint32_t res = 0; res < 16; res += 5)
            for (int where = 0; where < 3; where++) {                        // no difference | one at cmp - 1 | x changed at cmp (not compared)
                const uint32_t len = pc[0], cmp = pc[1];
                if (where == 1 && !cmp) continue;
                if (where == 2 && cmp == len) continue;
                snprintf(g_case, sizeof(g_case), "piece len=%u cmp=%u res=%u where=%d", len, cmp, res, where);
                Range x(res, len), y((res * 7 + 3) & 15u, cmp);
                for (uint32_t i = 0; i < len; i++) x.p[i] = next_byte();
                if (cmp) memcpy(y.p, x.p, cmp);
                if (where == 1) y.p[cmp - 1] ^= 0x80;
                if (where == 2) x.p[cmp] ^= 0x01;
                const Got g = run_piece<PLANT>(x.p, cmp ? y.p : nullptr, len, cmp);
                if (g.first != (where == 1 ? cmp - 1 : len) || !sums_ok(g, x.p, len)) return fail();
                ncases++;
            }
    // Part 3: a fragment of three pieces
    static const int64_t folds[][2] = {{-1, -1}, {16383, -1}, {16384, -1}, {16385, -1}, {16385, 16383}, {39999, 16384}};
    const uint64_t size = 40000;
    for (uint32_t res = 0; res < 16; res += 3)
        for (const int64_t *fd : folds) {
            snprintf(g_case, sizeof(g_case), "fold res=%u diff=%lld", res, (long long)(fd[1] >= 0 && fd[1] < fd[0] ? fd[1] : fd[0]));
            Range x(res, size), y((res * 5 + 9) & 15u, size);
            for (uint64_t i = 0; i < size; i++) y.p[i] = x.p[i] = next_byte();
            for (int k = 0; k < 2; k++) if (fd[k] >= 0) y.p[fd[k]] ^= 0x10;
            std::vector<CopyPiece> pieces;
            piece_split(x.p, y.p, size, kFragPiece, [&](uint64_t, const CopyPiece &p) { pieces.push_back(p); });
            std::vector<PieceSums> sums;
            std::vector<uint32_t> firsts;
            for (const CopyPiece &p : pieces) {
                const Got g = run_piece<PLANT>(p.src, p.dst, p.len, p.len);
                sums.push_back(PieceSums{g.a, g.b});
                firsts.push_back(g.first);
            }
            uint64_t want = size;
            for (uint64_t i = 0; i < size; i++) if (x.p[i] != y.p[i]) { want = i; break; }
            const uint32_t *fp = firsts.data();
            const PieceSums *sp = sums.data();
            if (fold_first<PLANT>([fp](uint32_t k) { return fp[k]; }, (uint32_t)pieces.size(), size) != want) return fail();
            if (fold_pieces([sp](uint32_t k) { return sp[k]; }, (uint32_t)pieces.size(), size) != adler32_bytes(x.p, size)) return fail();
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
    case kPlantCmpHeadNotCompared: return run_all<kPlantCmpHeadNotCompared>();
    case kPlantCmpUnitWithoutHead: return run_all<kPlantCmpUnitWithoutHead>();
    case kPlantCmpWindowPastEnd: return run_all<kPlantCmpWindowPastEnd>();
    case kPlantFirstPieceIndex: return run_all<kPlantFirstPieceIndex>();
    }
    return 2;
}
