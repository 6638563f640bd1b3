// csa_dev_digest_model.cpp -- digest_leaf<PLANT> and digest_root of csc_amd/csrc/csa_dev_digest.h (the text k_digest_leaves and
// k_digest_roots run: the BLAKE2s tree-mode digest of a fragment) on the CPU, lane by lane, under AddressSanitizer and UBSan
// (tests/test_archive_digest_host.py builds and runs it; a program of its own, nothing is preloaded).
//
//   csa_dev_digest_model PLANT     PLANT = 0: the text the kernels run; 1 .. 4: one of the header's planted mistakes switched on
//
// Byte i of a fragment of n bytes is ((i * 2654435761 + n) mod 2^32) >> 13, so the test rebuilds every fragment and takes its
// digest with hashlib.  Each case prints one line "<case> <64 hex digits>" and is named before it runs.
// Part 1, contiguous sources: kSizes x source alignments 0, 1, 7, 8, 15.  The source is a heap block that begins `alignment` bytes
// into its allocation (poisoned in front as far as ASan's 8-byte granules allow) and ends where the allocation ends, so a byte
// loaded outside it is the sanitizer's to report.
// Part 2, the runs of a periodic slice: a fragment at packed offset 12345 of its entry under a few slices (run 5, 16, 4099 among
// them), the buffer exactly offset + hull bytes with 0xEE in the gaps: digest_split per leaf, as the host planner cuts it.
// Part 3, the tables of k_digest_roots at an odd address, exactly as large as their digests: the root stored byte by byte and
// compared with an expected table that is equal (0) and one with one bit flipped (1); "root ok" is printed.
//
// When a sanitizer ends the run, the case it happened in is named on a line "AT <case>".  Exit status 0 only if every case ran.
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csa_dev_digest.h"

using namespace csadev;

static char g_case[160] = "start";
static void on_death() { fprintf(stderr, "AT %s\n", g_case); fflush(stderr); }

static uint8_t byte_of(uint64_t i, uint64_t n) { return (uint8_t)(((uint32_t)i * 2654435761u + (uint32_t)n) >> 13); }

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

static const uint32_t kSizes[] = {0, 1, 55, 63, 64, 65, 127, 128, 16383, 16384, 16385, 32768, 49153};
static const uint32_t kAligns[] = {0, 1, 7, 8, 15};
struct Pattern { uint64_t run, stride; };
static const Pattern kPatterns[] = {{5, 9}, {16, 48}, {17, 17}, {4099, 5000}, {20000, 20001}};

// the fragment as the two kernels see it: every leaf by one lane, then the root by one
template <int PLANT>
static DigestWords digest_of(const uint8_t *buf, const Slice &sl, uint64_t at, uint64_t size)
{
    std::vector<DigestLeaf> leaves;
    digest_split(buf, sl, at, size, [&](const DigestLeaf &l) { leaves.push_back(l); });
    std::vector<DigestWords> dl(leaves.size());
    for (size_t i = 0; i < leaves.size(); i++) digest_leaf<PLANT>(leaves[i], dl[i]);
    uint8_t out[kDigestBytes];
    const DigestFrag f = {0, kDigestNone, 0, (uint32_t)leaves.size()};
    digest_root(f, dl.data(), out, nullptr);
    DigestWords d;
    memcpy(d.w, out, kDigestBytes);
    return d;
}

static void print(const DigestWords &d)
{
    const uint8_t *b = (const uint8_t *)d.w;
    printf("%s ", g_case);
    for (uint32_t j = 0; j < kDigestBytes; j++) printf("%02x", b[j]);
    printf("\n");
    fflush(stdout);
}

template <int PLANT>
static int run()
{
    int n = 0;
    for (uint32_t size : kSizes)
        for (uint32_t al : kAligns) {
            snprintf(g_case, sizeof(g_case), "size=%u al=%u", size, al);
            Range r(al, size);
            for (uint32_t i = 0; i < size; i++) r.p[i] = byte_of(i, size);
            print(digest_of<PLANT>(r.p, Slice{0, size, size, size ? 1u : 0u}, 0, size));
            n++;
        }
    for (uint32_t size : {16385u, 49153u})
        for (const Pattern &pt : kPatterns)
            for (uint32_t al : {0u, 3u}) {
                snprintf(g_case, sizeof(g_case), "rows size=%u run=%llu stride=%llu al=%u", size, (unsigned long long)pt.run,
                         (unsigned long long)pt.stride, al);
                const uint64_t at = 12345, count = (at + size + pt.run - 1) / pt.run, offset = 3;
                Slice sl = {offset, pt.run, pt.stride, count};
                const uint64_t bytes = offset + (count - 1) * pt.stride + pt.run;
                Range r(al, bytes);
                memset(r.p, 0xEE, bytes);
                for (uint64_t p = at; p < at + size; p++) r.p[offset + (p / pt.run) * pt.stride + p % pt.run] = byte_of(p - at, size);
                uint64_t sel;
                if (!slice_check(sl, bytes, &sel)) { printf("FAIL %s\n", g_case); return 1; }
                print(digest_of<PLANT>(r.p, sl, at, size));
                n++;
            }
    // the root's tables, byte by byte at an odd address
    snprintf(g_case, sizeof(g_case), "root tables");
    {
        Range src(0, 40000), out(1, 3 * kDigestBytes), exp(5, 2 * kDigestBytes);
        for (uint32_t i = 0; i < 40000; i++) src.p[i] = byte_of(i, 40000);
        std::vector<DigestLeaf> leaves;
        digest_split(src.p, Slice{0, 40000, 40000, 1}, 0, 40000, [&](const DigestLeaf &l) { leaves.push_back(l); });
        std::vector<DigestWords> dl(leaves.size());
        for (size_t i = 0; i < leaves.size(); i++) digest_leaf<PLANT>(leaves[i], dl[i]);
        memset(out.p, 0, 3 * kDigestBytes);
        DigestFrag f = {2, kDigestNone, 0, (uint32_t)leaves.size()};
        if (digest_root(f, dl.data(), out.p, nullptr) != 0) { printf("FAIL %s\n", g_case); return 1; }
        memcpy(exp.p + kDigestBytes, out.p + 2 * kDigestBytes, kDigestBytes);
        memset(exp.p, 0, kDigestBytes);
        f.out = 0; f.expect = 1;
        if (digest_root(f, dl.data(), out.p, exp.p) != 0 || memcmp(out.p, exp.p + kDigestBytes, kDigestBytes) != 0) { printf("FAIL %s\n", g_case); return 1; }
        exp.p[kDigestBytes + 31] ^= 0x80;
        if (digest_root(f, dl.data(), nullptr, exp.p) != 1) { printf("FAIL %s\n", g_case); return 1; }
        f.expect = 0;
        if (digest_root(f, dl.data(), nullptr, exp.p) != 1) { printf("FAIL %s\n", g_case); return 1; }
        for (uint32_t j = 0; j < kDigestBytes; j++) if (out.p[kDigestBytes + j] != 0) { printf("FAIL %s\n", g_case); return 1; }
        printf("root ok\n");
    }
    printf("ok %d\n", n);
    return 0;
}

int main(int argc, char **argv)
{
    __sanitizer_set_death_callback(on_death);
    const int plant = argc > 1 ? atoi(argv[1]) : 0;
    switch (plant) {
    case 0: return run<kDPlantNone>();
    case 1: return run<kDPlantExtraEmptyBlock>();
    case 2: return run<kDPlantLastNodeEveryLeaf>();
    case 3: return run<kDPlantNodeOffsetUnset>();
    case 4: return run<kDPlantWindowPastEnd>();
    }
    return 2;
}
