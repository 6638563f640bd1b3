// csa_dev_digest.h -- the fragment digests of the device-resident archive (CSAMI_DeviceDigestSlices, CSAMI_DeviceUpdateDigests,
// CSAMI_DeviceReadDigests, include/csa_mi355x.h) below the host planner: BLAKE2s-256 in tree mode over the 16 KiB grid the piece
// tables already put on a packed fragment.  Compiles for the host (plain C++: tests/test_archive_digest_host.py runs
// tests/model/csa_dev_digest_model.cpp with g++ and the sanitizers) and for the device (k_digest_leaves, k_digest_roots in
// csa_dev_kernels.hip), so the model runs the text the kernels run.
//
// The digest of a fragment of n bytes (RFC 7693, with the tree parameters of the BLAKE2 paper, section 2.10): fan-out 0, maximal
// depth 2, leaf length 16384, inner length 32, digest length 32, no key, salt or personalisation.  L = max(1, ceil(n / 16384))
// leaves; leaf i is the bytes [16384 i, min(n, 16384 (i + 1))), hashed with node offset i, node depth 0 and the last-node flag on
// leaf L - 1 only; the root is hashed over the L leaf digests, node offset 0, node depth 1, last-node flag set.  Python's
// hashlib.blake2s computes both with stock parameters (csc_amd.csa.fragment_digest), so the checker shares no text with this file.
//
// A leaf is a serial chain of up to 256 compressions, so the parallelism is across leaves: one LANE per leaf (k_digest_leaves), and
// one lane per fragment over its leaves' digests (k_digest_roots), which also compares with an expected table where one is given.
// A lane loads its own 64-byte blocks: nothing outside the leaf's bytes is loaded, not even by an aligned window.
//
// The template parameter PLANT switches one deliberate mistake on (0: none).  The product instantiates 0 only; the model runs each
// of the others and has to see it caught by a named case.
#pragma once
#include <stdint.h>

#include "csa_dev_write.h"

namespace csadev {

constexpr uint32_t kDigestLeaf = kFragPiece;    // bytes of a leaf: the piece grid
constexpr uint32_t kDigestBytes = 32;
constexpr uint32_t kDigestThreads = 64;         // workgroup of k_digest_leaves and k_digest_roots: one wavefront, so that few leaves still spread over the CUs
constexpr uint64_t kDigestNone = ~0ull;         // DigestFrag::expect: the fragment is not compared

enum DigestPlant { kDPlantNone = 0, kDPlantExtraEmptyBlock = 1, kDPlantLastNodeEveryLeaf = 2, kDPlantNodeOffsetUnset = 3, kDPlantWindowPastEnd = 4 };

struct DigestWords { uint32_t w[8]; };          // a digest as the eight little-endian words of the chaining value
struct DigestLeaf {        // one lane of k_digest_leaves
    const uint8_t *src;    // stride == 0: the leaf's contiguous bytes, any alignment; else the address of period position 0 (GatherPiece's)
    uint64_t stride;       // periodic: the address step from one run to the next, >= run
    uint32_t len;          // <= kDigestLeaf; 0: the one leaf of an empty fragment, src is not looked at
    uint32_t node;         // the leaf's number in its fragment
    uint32_t last;         // 1: the fragment's last leaf
    uint32_t phase;        // periodic: byte i of the leaf is period position pos = phase + i; row = pos / run, r = pos % run; it lies
    uint32_t run;          //           at src + row * stride + r
    uint32_t pad;
};
struct DigestFrag {        // one lane of k_digest_roots
    uint64_t out;          // the fragment's place in the output table
    uint64_t expect;       // its place in the expected table, kDigestNone: not compared
    uint32_t first;        // its first leaf; the leaves of a fragment are consecutive
    uint32_t nleaves;      // >= 1
};

#define CSADEV_B2S_G(a, b, c, d, x, y)                                  \
    do {                                                                \
        v[a] = v[a] + v[b] + (x); v[d] = rotr32(v[d] ^ v[a], 16);       \
        v[c] = v[c] + v[d];       v[b] = rotr32(v[b] ^ v[c], 12);       \
        v[a] = v[a] + v[b] + (y); v[d] = rotr32(v[d] ^ v[a], 8);        \
        v[c] = v[c] + v[d];       v[b] = rotr32(v[b] ^ v[c], 7);        \
    } while (0)
#define CSADEV_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                \
        CSADEV_B2S_G(0, 4, 8, 12, m[s0], m[s1]);                        \
        CSADEV_B2S_G(1, 5, 9, 13, m[s2], m[s3]);                        \
        CSADEV_B2S_G(2, 6, 10, 14, m[s4], m[s5]);                       \
        CSADEV_B2S_G(3, 7, 11, 15, m[s6], m[s7]);                       \
        CSADEV_B2S_G(0, 5, 10, 15, m[s8], m[s9]);                       \
        CSADEV_B2S_G(1, 6, 11, 12, m[s10], m[s11]);                     \
        CSADEV_B2S_G(2, 7, 8, 13, m[s12], m[s13]);                      \
        CSADEV_B2S_G(3, 4, 9, 14, m[s14], m[s15]);                      \
    } while (0)

CSADEV_FHD uint32_t rotr32(uint32_t x, uint32_t n) { return (x >> n) | (x << (32u - n)); }

CSADEV_FHD uint32_t blake2s_iv(uint32_t i)
{
    return i == 0 ? 0x6A09E667u : i == 1 ? 0xBB67AE85u : i == 2 ? 0x3C6EF372u : i == 3 ? 0xA54FF53Au
         : i == 4 ? 0x510E527Fu : i == 5 ? 0x9B05688Cu : i == 6 ? 0x1F83D9ABu : 0x5BE0CD19u;
}

// The compression function F of RFC 7693, section 3.2: h over the 16 message words m, the 64-bit counter (t0, t1) and the two
// finalisation words (f0: the node's last block; f1: the last node of its level).  Every index is a literal: h, m and v stay in registers.
CSADEV_FHD void blake2s_compress(uint32_t h[8], const uint32_t m[16], uint32_t t0, uint32_t t1, uint32_t f0, uint32_t f1)
{
    uint32_t v[16];
    for (uint32_t i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = blake2s_iv(i); }
    v[12] ^= t0; v[13] ^= t1; v[14] ^= f0; v[15] ^= f1;
    CSADEV_B2S_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    CSADEV_B2S_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    CSADEV_B2S_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    CSADEV_B2S_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    CSADEV_B2S_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    CSADEV_B2S_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    CSADEV_B2S_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    CSADEV_B2S_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    CSADEV_B2S_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    CSADEV_B2S_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    for (uint32_t i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

// One node of the tree: `len` bytes, served in blocks by load(off, n, m) -- the n <= 64 bytes at offset off of the node into the 16
// words of m, little endian, zero behind them -- hashed with node offset `node`, node depth `depth` and the last-node flag `last`.
// BLAKE2 holds the last block back: a node whose length is a multiple of 64 compresses its last 64 bytes with the final flag and
// no empty block behind them; an empty node is one zero block with counter 0.
template <int PLANT = kDPlantNone, class Load>
CSADEV_FHD void blake2s_node(Load load, uint64_t len, uint32_t node, uint32_t depth, bool last, uint32_t h[8])
{
    // the parameter block: digest length 32, no key, fan-out 0, maximal depth 2 | leaf length | node offset (48 bits) | node depth,
    // inner length 32 | salt and personalisation zero
    const uint32_t off = PLANT == kDPlantNodeOffsetUnset ? 0u : node;
    const uint32_t p[4] = {32u | 0u << 8 | 0u << 16 | 2u << 24, kDigestLeaf, off, 0u | depth << 16 | kDigestBytes << 24};
    for (uint32_t i = 0; i < 8; i++) h[i] = blake2s_iv(i) ^ (i < 4 ? p[i] : 0u);
    uint32_t m[16], t0 = 0, t1 = 0;
    uint64_t done = 0;
    while (PLANT == kDPlantExtraEmptyBlock ? len - done >= 64 : len - done > 64) {
        load(done, 64u, m);
        t0 += 64u;
        t1 += t0 < 64u ? 1u : 0u;
        blake2s_compress(h, m, t0, t1, 0u, 0u);
        done += 64;
    }
    const uint32_t rest = (uint32_t)(len - done);
    load(done, rest, m);
    t0 += rest;
    t1 += t0 < rest ? 1u : 0u;
    blake2s_compress(h, m, t0, t1, ~0u, last || PLANT == kDPlantLastNodeEveryLeaf ? ~0u : 0u);
}

// The n <= 64 bytes at offset off of the contiguous leaf src[0, len) into m.  The leaf has any alignment; nothing outside it is
// loaded.  A whole block on a 4-byte line is 16 word loads (four 16-byte loads on a 16-byte line); a whole block off the line is
// the 17 aligned words around it, funnel-shifted, where they lie inside the leaf; anything else -- the last, short block, and the
// first and last whole block of a leaf off the line -- goes byte by byte.
template <int PLANT = kDPlantNone>
CSADEV_FHD void digest_load(const uint8_t *src, uint32_t len, uint32_t off, uint32_t n, uint32_t m[16])
{
    const uint8_t *p = src + off;
    const uint32_t a = (uint32_t)(uintptr_t)p & 3u;
    if (n == 64 && a == 0) {
        if (((uintptr_t)p & 15u) == 0) {
            for (uint32_t k = 0; k < 4; k++) {
                const Vec16 x = ((const Vec16 *)p)[k];
                m[4 * k] = x.w[0]; m[4 * k + 1] = x.w[1]; m[4 * k + 2] = x.w[2]; m[4 * k + 3] = x.w[3];
            }
        } else {
            for (uint32_t k = 0; k < 16; k++) m[k] = ((const uint32_t *)p)[k];
        }
    } else if (n == 64 && off >= a && (PLANT == kDPlantWindowPastEnd || off - a + 68 <= len)) {
        const uint32_t *q = (const uint32_t *)(p - a);
        const uint32_t sh = 8 * a;
        uint32_t lo = q[0];
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t hi = q[k + 1];
            m[k] = (lo >> sh) | (hi << (32u - sh));
            lo = hi;
        }
    } else {
        for (uint32_t k = 0; k < 16; k++) m[k] = 0;
        for (uint32_t j = 0; j < n; j++) m[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3u));
    }
}

// The same out of the runs of a periodic leaf (DigestLeaf with stride != 0): four bytes of one run on a 4-byte line are one word
// load, anything else goes byte by byte.  One division a block; only bytes of the leaf are loaded, no gap byte.
CSADEV_FHD void digest_load_rows(const DigestLeaf &lf, uint32_t off, uint32_t n, uint32_t m[16])
{
    for (uint32_t k = 0; k < 16; k++) m[k] = 0;
    const uint32_t pos = lf.phase + off;
    uint32_t row = pos / lf.run, r = pos - row * lf.run;
    const uint8_t *p = lf.src + row * lf.stride + r;
    for (uint32_t j = 0; j < n;) {
        if (!(j & 3u) && j + 4 <= n && r + 4 <= lf.run && !((uintptr_t)p & 3u)) {
            m[j >> 2] = *(const uint32_t *)p;
            j += 4; r += 4; p += 4;
        } else {
            m[j >> 2] |= (uint32_t)*p << (8 * (j & 3u));
            j++; r++; p++;
        }
        if (r == lf.run) { r = 0; p += lf.stride - lf.run; }
    }
}

// One lane of k_digest_leaves: the digest of leaf lf into out
template <int PLANT = kDPlantNone>
CSADEV_FHD void digest_leaf(const DigestLeaf &lf, DigestWords &out)
{
    if (lf.stride)
        blake2s_node<PLANT>([&lf](uint64_t off, uint32_t n, uint32_t m[16]) { digest_load_rows(lf, (uint32_t)off, n, m); },
                            lf.len, lf.node, 0u, lf.last != 0, out.w);
    else
        blake2s_node<PLANT>([&lf](uint64_t off, uint32_t n, uint32_t m[16]) { digest_load<PLANT>(lf.src, lf.len, (uint32_t)off, n, m); },
                            lf.len, lf.node, 0u, lf.last != 0, out.w);
}

// One lane of k_digest_roots: the root of fragment f over its leaves' digests, stored to out[f.out] (out == NULL: nowhere) and
// compared with expect[f.expect] (f.expect == kDigestNone: not compared).  Both tables are 32 bytes a fragment at ANY alignment,
// so they are touched byte by byte.  Returns 1 where a compared digest differs.
CSADEV_FHD uint32_t digest_root(const DigestFrag &f, const DigestWords *leaves, uint8_t *out, const uint8_t *expect)
{
    const DigestWords *lv = leaves + f.first;
    DigestWords d;
    blake2s_node([lv](uint64_t off, uint32_t n, uint32_t m[16]) {
        const uint32_t *w = (const uint32_t *)lv + off / 4;              // (a block is two leaf digests, the last one maybe one)
        for (uint32_t k = 0; k < 16; k++) m[k] = 4 * k < n ? w[k] : 0u;
    }, (uint64_t)f.nleaves * kDigestBytes, 0u, 1u, true, d.w);
    uint32_t differs = 0;
    for (uint32_t j = 0; j < kDigestBytes; j++) {
        const uint8_t b = (uint8_t)(d.w[j >> 2] >> (8 * (j & 3u)));
        if (out) out[f.out * kDigestBytes + j] = b;
        if (f.expect != kDigestNone && expect[f.expect * kDigestBytes + j] != b) differs = 1;
    }
    return differs;
}

// The leaves of a fragment of `size` bytes that is the packed bytes [at, at + size) of the (checked) slice sl of the buffer `buf`:
// put(DigestLeaf) for each, in order.  Returns their number: max(1, ceil(size / kDigestLeaf)).
template <class Put>
inline uint64_t digest_split(const uint8_t *buf, const Slice &sl, uint64_t at, uint64_t size, Put put)
{
    if (!size) { put(DigestLeaf{nullptr, 0, 0, 0, 1, 0, 0, 0}); return 1; }
    uint64_t k = 0;
    for (uint64_t off = 0; off < size; off += kDigestLeaf, k++) {
        const uint32_t len = (uint32_t)(size - off < kDigestLeaf ? size - off : kDigestLeaf);
        GatherCut c;
        gather_reduce(sl, at + off, len, c);                                // (inside one run: stride, phase and run are 0)
        put(DigestLeaf{buf + c.src, c.stride, len, (uint32_t)k, off + len == size ? 1u : 0u, c.phase, c.run, 0});
    }
    return k;
}

}  // namespace csadev
