// csa_dev_read.h -- the device-resident archive read (CSAMI_DeviceRead, include/csa_mi355x.h) below the host planner: the piece
// tables its three kernels walk, the copy between two byte ranges of ANY alignment, the adler32 sums taken in the same pass, and
// the fold of a fragment's pieces.  Compiles for the host (plain C++: tests/test_archive_device_host.py runs
// tests/model/csa_dev_model.cpp with g++ and the sanitizers) and for the device (csa_dev_kernels.hip), so the model runs the text
// the kernels run.
//
// What the reference does with these bytes: AsyncArchiveReader (csa_io.h:466-542) serves a task's archive blocks back to back --
// here k_gather_extents copies them into one range; AsyncFileWriter (csa_io.h:274-408) cuts the decoded task into its fragments,
// writes each at its file offset and folds adler32 (csa_adler32.cpp:63-129) over it -- here k_frag_pieces and k_frag_fold.
//
// adler32 piecewise: a piece of `len` bytes gives A = sum(b_i) and B = sum((len - i) * b_i) as plain integers, and consecutive
// pieces fold as b' = b + len * a + B, a' = a + A (mod 65521), seed 0.  CSA_Add and CSAMI_Adler32Device (csa_archive.cpp) take
// the same sums with k_frag_pieces<false> and fold them on the host: their pieces are cut per chunk and their seed runs on.
//
// CSAMI_DeviceCompare runs the same tables with k_frag_compare and k_frag_fold_diff in the place of the last two: compare_sum reads a
// fragment's piece and the caller's range side by side, compare_piece joins a compared front and a summed rest into one piece's sums,
// fold_first folds the pieces' first differences (tests/model/csa_dev_compare_model.cpp is their model).
//
// CSAMI_DeviceReadSlices runs them with k_frag_slices in the middle: slice_check / slice_next / slice_reduce are its planner's,
// slice_sum the piece that is summed whole and stored in part (tests/model/csa_dev_slice_model.cpp is their model).
//
// CSAMI_DeviceReadIntoSlices and CSAMI_DeviceCompareSlices run them with k_frag_spread / k_frag_compare_rows in the middle wherever a
// piece's side in the caller's buffer is the runs of a periodic pattern: spread_sum is gather_sum (csa_dev_write.h) with source and
// destination exchanged, compare_rows is compare_piece against such rows (tests/model/csa_dev_spread_model.cpp is their model).
//
// The template parameter PLANT switches one deliberate mistake on (0: none).  The product instantiates 0 only; the models run each
// of the others and have to see it caught by a named case.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSADEV_FHD __host__ __device__ inline
#else
#define CSADEV_FHD inline
#endif

namespace csadev {

constexpr uint32_t kThreads = 256;              // workgroup of k_gather_extents and k_frag_pieces
constexpr uint32_t kGatherPiece = 65536;        // bytes of an extent one workgroup copies
constexpr uint32_t kFragPiece = 16384;          // bytes of a fragment one workgroup sums (and stores)
constexpr uint32_t kAdlerBase = 65521;

enum Plant {
    kPlantNone = 0, kPlantTailDropped = 1, kPlantWeightOffByOne = 2, kPlantFoldLastLen = 3, kPlantHeadWrongPointer = 4,
    // compare_sum and fold_first (tests/model/csa_dev_compare_model.cpp)
    kPlantCmpHeadNotCompared = 5, kPlantCmpUnitWithoutHead = 6, kPlantCmpWindowPastEnd = 7, kPlantFirstPieceIndex = 8,
    // slice_sum (tests/model/csa_dev_slice_model.cpp)
    kPlantSliceBorderLate = 9, kPlantSlicePhaseDropped = 10, kPlantSliceStraddleWhole = 11, kPlantSliceRowNotAdvanced = 12,
    // spread_sum and compare_rows (tests/model/csa_dev_spread_model.cpp)
    kPlantSpreadBorderLate = 13, kPlantSpreadPhaseDropped = 14, kPlantSpreadStraddleWhole = 15, kPlantSpreadRowNotAdvanced = 16,
    kPlantRowsWindowPastHull = 17, kPlantRowsHeadNotCompared = 18
};

struct CopyPiece {         // one workgroup of k_gather_extents / k_frag_pieces / k_frag_compare
    const uint8_t *src;
    uint8_t *dst;          // k_frag_pieces<false>: unused; k_frag_pieces<true>: NULL = summed, not stored; k_frag_compare: the caller's range y, read only
    uint32_t len;          // <= kGatherPiece / kFragPiece
    uint32_t cmp;          // k_frag_compare: the leading bytes that are compared, <= len, 0 where dst is NULL; the others: 0, unused
};
struct PieceSums { uint64_t a, b; };
struct FragFold {          // one lane of k_frag_fold
    uint64_t size;         // the fragment's bytes that were delivered (clipped to its task's `produced`)
    uint32_t first;        // its first piece; the pieces of a fragment are consecutive
    uint32_t npieces;
    uint32_t checksum;     // the index's
    uint32_t pad;
};
struct FragResult { uint32_t adler, ok; };      // all the host reads back of a fragment
struct FragDiff {                               // ... of a fragment that was compared (k_frag_fold_diff)
    uint32_t adler, ok;
    uint64_t first;        // the first differing offset in the fragment's delivered bytes, FragFold::size if there is none
};

CSADEV_FHD uint64_t piece_count(uint64_t size, uint32_t piece) { return (size + piece - 1) / piece; }

// src[0, size) -> dst[0, size) in pieces of at most `piece` bytes: put(k, CopyPiece) for k = 0 .. piece_count - 1.  dst may be NULL.
template <class Put>
CSADEV_FHD uint64_t piece_split(const uint8_t *src, uint8_t *dst, uint64_t size, uint32_t piece, Put put)
{
    uint64_t k = 0;
    for (uint64_t off = 0; off < size; off += piece, k++) {
        CopyPiece p;
        p.src = src + off;
        p.dst = dst ? dst + off : nullptr;
        p.len = (uint32_t)(size - off < piece ? size - off : piece);
        p.cmp = 0;
        put(k, p);
    }
    return k;
}

struct alignas(16) Vec16 { uint32_t w[4]; };

// the four bytes of w sit at piece positions i0 .. i0 + 3 (little endian), all inside [0, len); wl = len (the weight of byte 0)
CSADEV_FHD void sum_word(uint32_t w, uint32_t i0, uint32_t wl, uint64_t &a, uint64_t &b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t s = __builtin_amdgcn_sad_u8(w, 0u, 0u);                      // b0+b1+b2+b3
    const uint32_t t = __builtin_amdgcn_udot4(w, 0x03020100u, 0u, false);       // 0*b0+1*b1+2*b2+3*b3
#else
    const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
    const uint32_t s = b0 + b1 + b2 + b3, t = b1 + 2 * b2 + 3 * b3;
#endif
    a += s;
    b += (uint64_t)(wl - i0) * s - t;
}

// The 16 bytes that begin m bytes, 0 < m < 16, into the aligned vector x, whose next one is y: funnel-shifted into place
CSADEV_FHD Vec16 funnel16(const Vec16 &x, const Vec16 &y, uint32_t m)
{
    const uint32_t sw = m >> 2, sb = 8 * (m & 3u);
    const uint32_t t0 = (sw & 2u) ? x.w[2] : x.w[0], t1 = (sw & 2u) ? x.w[3] : x.w[1], t2 = (sw & 2u) ? y.w[0] : x.w[2],
                   t3 = (sw & 2u) ? y.w[1] : x.w[3], t4 = (sw & 2u) ? y.w[2] : y.w[0], t5 = (sw & 2u) ? y.w[3] : y.w[1];
    const uint32_t u0 = (sw & 1u) ? t1 : t0, u1 = (sw & 1u) ? t2 : t1, u2 = (sw & 1u) ? t3 : t2, u3 = (sw & 1u) ? t4 : t3,
                   u4 = (sw & 1u) ? t5 : t4;
    Vec16 o;
    o.w[0] = (uint32_t)((((uint64_t)u1 << 32) | u0) >> sb);
    o.w[1] = (uint32_t)((((uint64_t)u2 << 32) | u1) >> sb);
    o.w[2] = (uint32_t)((((uint64_t)u3 << 32) | u2) >> sb);
    o.w[3] = (uint32_t)((((uint64_t)u4 << 32) | u3) >> sb);
    return o;
}

// the 16 bytes at p, of any alignment, one by one
CSADEV_FHD Vec16 load_bytes16(const uint8_t *p)
{
    Vec16 o;
    for (uint32_t k = 0; k < 4; k++)
        o.w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    return o;
}

// Unit i -- the 16 bytes [s0 + 16 i, s0 + 16 i + 16) -- of a range r[0, n), where s0 = r + head has any alignment and the unit lies
// inside the range: one aligned 16-byte load; or two of them, funnel-shifted into place; or, where that 32-byte window would begin
// before r or end behind r + n (the first and the last unit, at most), the 16 bytes one by one.
template <bool WINDOW_UNCHECKED = false>
CSADEV_FHD Vec16 load_unit(const uint8_t *s0, uint32_t head, uint32_t n, uint32_t i)
{
    const uint32_t m = (uint32_t)(uintptr_t)s0 & 15u;
    const uintptr_t base = (uintptr_t)s0 - m;                         // aligned; vector i of it covers bytes [16 i - m, 16 i - m + 16) of s0
    if (m == 0) return *(const Vec16 *)(base + 16ull * i);
    if (WINDOW_UNCHECKED || (head + 16 * i >= m && head + 16 * i + 32 <= n + m))    // the window [16 i - m, 16 i - m + 32) of s0 lies in r[0, n)
        return funnel16(*(const Vec16 *)(base + 16ull * i), *(const Vec16 *)(base + 16ull * i + 16), m);
    return load_bytes16(s0 + 16 * i);
}

// The 16 bytes at p, of any alignment, all inside the hull [lo, hi): one aligned 16-byte load; or two of them, funnel-shifted into
// place, as load_unit; or, where that 32-byte window would leave the hull, the 16 bytes one by one.
template <bool END_UNCHECKED = false>
CSADEV_FHD Vec16 load_window(const uint8_t *p, const uint8_t *lo, const uint8_t *hi)
{
    const uint32_t m = (uint32_t)(uintptr_t)p & 15u;
    const uintptr_t base = (uintptr_t)p - m;
    if (m == 0) return *(const Vec16 *)base;
    if (base >= (uintptr_t)lo && (END_UNCHECKED || base + 32 <= (uintptr_t)hi)) return funnel16(*(const Vec16 *)base, *(const Vec16 *)(base + 16), m);
    return load_bytes16(p);
}

// Thread `tid` of `nthreads`: its share of src[0, n) -- copied to dst[0, n) (STORE) and/or summed into a, b as one piece of n bytes
// (SUM; the caller adds the threads' a and b up).  n <= 65536.  src and dst have any alignment.  Nothing outside src[0, n) is
// loaded, not even by an aligned 16-byte window, and nothing outside dst[0, n) is stored.
//
// Up to 15 head bytes bring the anchor (dst with STORE, else src) to a 16-byte line and up to 15 tail bytes end the range: those
// are byte accesses.  Between them every unit is one 16-byte store of source words funnel-shifted into place, from two aligned
// 16-byte loads; a unit whose load window would begin before src or end behind src + n (the first and the last, at most) takes
// its 16 bytes one by one.
template <bool STORE, bool SUM, int PLANT = kPlantNone>
CSADEV_FHD void copy_sum(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b)
{
    const uint8_t *anchor = STORE && PLANT != kPlantHeadWrongPointer ? (const uint8_t *)dst : src;
    uint32_t head = (0u - (uint32_t)(uintptr_t)anchor) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = PLANT == kPlantTailDropped ? 0u : (n - head) & 15u;
    const uint32_t wl = PLANT == kPlantWeightOffByOne ? n - 1 : n;
    if (tid < head) {
        const uint32_t v = src[tid];
        if (STORE) dst[tid] = (uint8_t)v;
        if (SUM) { a += v; b += (uint64_t)(wl - tid) * v; }
    }
    // (the tail from the far end of the workgroup: the head's lanes are busy)
    if (nthreads - 1 - tid < tail) {
        const uint32_t k = head + 16 * units + (nthreads - 1 - tid);
        const uint32_t v = src[k];
        if (STORE) dst[k] = (uint8_t)v;
        if (SUM) { a += v; b += (uint64_t)(wl - k) * v; }
    }
    const uint8_t *s0 = src + head;                                   // unit i is source bytes [s0 + 16 i, s0 + 16 i + 16)
    for (uint32_t i = tid; i < units; i += nthreads) {
        const Vec16 o = load_unit(s0, head, n, i);
        if (STORE) *(Vec16 *)(dst + head + 16 * i) = o;
        if (SUM) {
            const uint32_t i0 = head + 16 * i;
            sum_word(o.w[0], i0, wl, a, b);
            sum_word(o.w[1], i0 + 4, wl, a, b);
            sum_word(o.w[2], i0 + 8, wl, a, b);
            sum_word(o.w[3], i0 + 12, wl, a, b);
        }
    }
}

// Thread `tid` of `nthreads`: its share of x[0, n) against y[0, n) (CSAMI_DeviceCompare).  x[0, n) is summed into a, b exactly as
// copy_sum<false, true> sums it (SUM) and compared with y[0, n): `first` is the smallest index at which THIS thread saw a difference,
// n if it saw none (the caller takes the minimum over the threads).  n <= 65536.  x and y have any, unrelated, alignment, and
// nothing outside x[0, n) or y[0, n) is loaded, not even by an aligned 16-byte window.
//
// The anchor is x: up to 15 head bytes bring it to a 16-byte line and up to 15 tail bytes end the range, byte by byte on both
// sides.  Between them a unit is one aligned 16-byte load of x against load_unit of y -- two aligned loads funnel-shifted, or bytes
// where that window would leave y[0, n).  The first differing byte of a unit is read off the XOR of its words: trailing zeros / 8.
template <bool SUM, int PLANT = kPlantNone>
CSADEV_FHD void compare_sum(const uint8_t *x, const uint8_t *y, uint32_t n, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b,
                            uint32_t &first)
{
    uint32_t head = (0u - (uint32_t)(uintptr_t)x) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = (n - head) & 15u;
    first = n;
    if (tid < head) {
        const uint32_t v = x[tid];
        if (PLANT != kPlantCmpHeadNotCompared && v != y[tid]) first = tid;
        if (SUM) { a += v; b += (uint64_t)(n - tid) * v; }
    }
    if (nthreads - 1 - tid < tail) {
        const uint32_t k = head + 16 * units + (nthreads - 1 - tid);
        const uint32_t v = x[k];
        if (v != y[k] && k < first) first = k;
        if (SUM) { a += v; b += (uint64_t)(n - k) * v; }
    }
    for (uint32_t i = tid; i < units; i += nthreads) {
        const uint32_t i0 = head + 16 * i;
        const Vec16 p = *(const Vec16 *)(x + i0), q = load_unit<PLANT == kPlantCmpWindowPastEnd>(y + head, head, n, i);
        const uint64_t lo = ((uint64_t)(p.w[1] ^ q.w[1]) << 32) | (p.w[0] ^ q.w[0]), hi = ((uint64_t)(p.w[3] ^ q.w[3]) << 32) | (p.w[2] ^ q.w[2]);
        if (lo | hi) {
            const uint32_t at = (PLANT == kPlantCmpUnitWithoutHead ? 16 * i : i0)
                                + (lo ? (uint32_t)__builtin_ctzll(lo) >> 3 : 8u + ((uint32_t)__builtin_ctzll(hi) >> 3));
            if (at < first) first = at;
        }
        if (SUM) {
            sum_word(p.w[0], i0, n, a, b);
            sum_word(p.w[1], i0 + 4, n, a, b);
            sum_word(p.w[2], i0 + 8, n, a, b);
            sum_word(p.w[3], i0 + 12, n, a, b);
        }
    }
}

// A piece of k_frag_compare: the first `cmp` of its `len` bytes are compared (compare_sum), the rest are summed only
// (copy_sum<false, true>), and the two parts' sums join as one piece of `len` bytes -- a byte of the front part weighs
// len - i = (cmp - i) + (len - cmp).  cmp == 0 (nothing to compare against, y may be NULL) and cmp == len are the usual cases; a
// piece in between is the one that straddles the end of the caller's buffer.  `first`: as compare_sum over [0, cmp), else len.
template <int PLANT = kPlantNone>
CSADEV_FHD void compare_piece(const uint8_t *x, const uint8_t *y, uint32_t len, uint32_t cmp, uint32_t tid, uint32_t nthreads, uint64_t &a,
                              uint64_t &b, uint32_t &first)
{
    first = len;
    if (cmp) {
        uint64_t fa = 0, fb = 0;
        uint32_t f;
        compare_sum<true, PLANT>(x, y, cmp, tid, nthreads, fa, fb, f);
        a += fa;
        b += fb + (uint64_t)(len - cmp) * fa;
        if (f < cmp) first = f;
    }
    if (cmp < len) copy_sum<false, true>(nullptr, x + cmp, len - cmp, tid, nthreads, a, b);
}

// ---- slices of an entry (CSAMI_DeviceReadSlices): a piece that is summed whole and stored in part ----
//
// A slice selects the bytes [offset + k * stride, offset + k * stride + run), k < count, of an entry and delivers them packed, row
// after row.  The pieces of a fragment stay on the fixed kFragPiece grid (fold_pieces needs it), so a piece may hold the tail of one
// run, a gap and the head of the next -- or, where run and stride are small, many of them.  slice_check, slice_next and slice_reduce
// are the host planner's; slice_sum is the workgroup's.

struct Slice { uint64_t offset, run, stride, count; };     // CSADevSlice of include/csa_mi355x.h

// What the read refuses in a slice of an entry of `size` bytes: false.  count == 1 gets stride = run; *bytes = run * count.
CSADEV_FHD bool slice_check(Slice &s, uint64_t size, uint64_t *bytes)
{
    *bytes = 0;
    if (!s.count) return true;
    if (!s.run) return false;
    if (s.count == 1) s.stride = s.run;
    if (s.stride < s.run) return false;
    uint64_t span, end;
    if (__builtin_mul_overflow(s.count - 1, s.stride, &span) || __builtin_add_overflow(span, s.run, &span)
        || __builtin_add_overflow(s.offset, span, &end) || end > size) return false;
    *bytes = s.run * s.count;                                         // (<= span, as run <= stride)
    return true;
}

// The first selected offset at or behind x of a checked slice, UINT64_MAX if there is none: one division, no walk over the rows.
// [x, y) holds a selected byte exactly when slice_next(s, x) < y.
CSADEV_FHD uint64_t slice_next(const Slice &s, uint64_t x)
{
    if (!s.count) return UINT64_MAX;
    if (x <= s.offset) return s.offset;
    const uint64_t t = x - s.offset, k = t / s.stride, r = t - k * s.stride;
    if (k >= s.count) return UINT64_MAX;
    if (r < s.run) return x;
    return k + 1 < s.count ? s.offset + (k + 1) * s.stride : UINT64_MAX;
}

struct SlicePiece {        // one workgroup of k_frag_slices: 32-bit quantities and two addresses, whatever the slice's 64-bit ones are
    const uint8_t *src;
    uint8_t *dst;          // stride == 0: the piece's one contiguous destination, NULL = summed, not stored (copy_sum, as a CopyPiece);
                           // else the address period position 0 would be stored to (it may lie in front of the caller's range: never stored to)
    uint32_t len;          // <= kFragPiece
    uint32_t lo, hi;       // periodic: only the piece's bytes [lo, hi) can be selected (the slice's hull cut to the piece)
    uint32_t phase;        // periodic: byte i of the piece stands at pos = phase + i; row = pos / stride, r = pos % stride; it is
    uint32_t run, stride;  //           selected when lo <= i < hi and r < run, and is stored to dst + row * run + r
};

enum SliceKind { kSliceNone = 0, kSliceWhole = 1, kSlicePeriodic = 2 };
struct SliceCut { uint32_t lo, hi, phase, run, stride; uint64_t dst; };

// The piece [at, at + len) of the entry, len <= kFragPiece, under a checked slice:
//   kSliceNone      it holds no selected byte
//   kSliceWhole     it lies inside one run; its bytes go to packed offset c.dst
//   kSlicePeriodic  anything else: c is the SlicePiece's lo, hi, phase, run, stride, and c.dst the packed offset of period position 0
//                   (modulo 2^64: it may stand for an offset below 0)
// A piece sees at most kFragPiece consecutive bytes, so whatever run and stride are it sees the same as under a pattern whose run is
// cut to kFragPiece -- the run it begins in from its front, since what lies before the piece is not seen, the next one from its
// back -- and whose gap is cut to kFragPiece likewise: stride' <= 2 * kFragPiece, and phase + len < 2^16.  Patterns that fit are left
// as they are (run' = run, stride' = stride).
CSADEV_FHD SliceKind slice_reduce(const Slice &s, uint64_t at, uint32_t len, SliceCut &c)
{
    c = SliceCut{0, 0, 0, 0, 0, 0};
    if (!s.count || !len) return kSliceNone;
    const uint64_t hull_hi = s.offset + (s.count - 1) * s.stride + s.run;            // (checked by slice_check)
    const uint64_t x0 = at > s.offset ? at : s.offset, x1 = at + len < hull_hi ? at + len : hull_hi;
    if (x0 >= x1 || slice_next(s, x0) >= x1) return kSliceNone;
    const uint64_t t = x0 - s.offset, k0 = t / s.stride, r0 = t - k0 * s.stride;
    if (x0 == at && x1 == at + len && r0 < s.run && s.run - r0 >= len) {
        c.dst = k0 * s.run + r0;
        return kSliceWhole;
    }
    const uint64_t gap = s.stride - s.run;
    const uint32_t R = (uint32_t)(s.run < kFragPiece ? s.run : kFragPiece), G = (uint32_t)(gap < kFragPiece ? gap : kFragPiece);
    uint32_t ph;                                                                      // the period position of x0
    uint64_t d;
    if (r0 < s.run) {                                     // in a run, `left` bytes from its end
        const uint64_t left = s.run - r0;
        ph = R - (uint32_t)(left < R ? left : R);
        d = k0 * s.run + r0 - ph;
    } else {                                              // in the gap, `left` bytes from the next run
        const uint64_t left = s.stride - r0;
        ph = R + G - (uint32_t)(left < G ? left : G);
        d = (k0 + 1) * s.run - R;
    }
    c.lo = (uint32_t)(x0 - at);
    c.hi = (uint32_t)(x1 - at);
    c.run = R;
    c.stride = R + G;
    // x0 is the piece's byte lo; the pattern is carried back to its byte 0 over whole periods
    const uint32_t back = c.lo > ph ? (c.lo - ph + c.stride - 1) / c.stride : 0;
    c.phase = ph + back * c.stride - c.lo;
    c.dst = d - (uint64_t)back * R;
    return kSlicePeriodic;
}

// Thread `tid` of `nthreads`: its share of a periodic piece.  Every byte of src[0, len) is loaded once -- the anchor is src, as x is in
// compare_sum: head and tail bytes one by one, between them aligned 16-byte units, so no window leaves src[0, len) -- and summed into a, b as one piece of len bytes, so the sums
// are copy_sum<false, true>'s; the selected bytes are stored to their packed places and nothing else is stored.  A unit that lies
// inside one run goes out as 16 bytes -- one store, four, or sixteen, as its destination's alignment allows; any other unit that
// meets [lo, hi) goes out byte by byte under the predicate.  No division in the unit loop: a thread's (row, r) advances by the
// workgroup's step, 16 * nthreads positions, with one carry.
template <int PLANT = kPlantNone>
CSADEV_FHD void slice_sum(const SlicePiece &pc, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b)
{
    const uint8_t *src = pc.src;
    const uintptr_t d0 = (uintptr_t)pc.dst;
    const uint32_t n = pc.len, lo = pc.lo, hi = pc.hi, run = pc.run, stride = pc.stride;
    uint32_t head = (0u - (uint32_t)(uintptr_t)src) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = (n - head) & 15u;
    const uint32_t border = PLANT == kPlantSliceBorderLate ? run + 1 : run;          // r < border: selected
    auto one = [&](uint32_t idx) {
        const uint32_t v = src[idx];
        a += v;
        b += (uint64_t)(n - idx) * v;
        if (idx >= lo && idx < hi) {
            const uint32_t pos = pc.phase + idx, row = pos / stride, r = pos - row * stride;
            if (r < border) *(uint8_t *)(d0 + row * run + r) = (uint8_t)v;
        }
    };
    if (tid < head) one(tid);
    if (nthreads - 1 - tid < tail) one(head + 16 * units + (nthreads - 1 - tid));
    if (tid >= units) return;
    const uint32_t step = 16 * nthreads, srow = step / stride, sr = step - srow * stride;
    const uint32_t pos = (PLANT == kPlantSlicePhaseDropped ? 0u : pc.phase) + head + 16 * tid;
    uint32_t row = pos / stride, r = pos - row * stride;
    for (uint32_t i = tid; i < units; i += nthreads) {
        const uint32_t i0 = head + 16 * i;
        const Vec16 o = *(const Vec16 *)(src + i0);                   // (aligned: the anchor is src, so load_unit has no window to shift)
        sum_word(o.w[0], i0, n, a, b);
        sum_word(o.w[1], i0 + 4, n, a, b);
        sum_word(o.w[2], i0 + 8, n, a, b);
        sum_word(o.w[3], i0 + 12, n, a, b);
        if (i0 < hi && i0 + 16 > lo) {
            if (i0 >= lo && i0 + 16 <= hi && (PLANT == kPlantSliceStraddleWhole ? r < run : r + 16 <= run)) {
                const uintptr_t d = d0 + row * run + r;
                if (!(d & 15u)) {
                    *(Vec16 *)d = o;
                } else if (!(d & 3u)) {
                    for (uint32_t j = 0; j < 4; j++) ((uint32_t *)d)[j] = o.w[j];
                } else {
                    for (uint32_t j = 0; j < 16; j++) ((uint8_t *)d)[j] = (uint8_t)(o.w[j >> 2] >> (8 * (j & 3u)));
                }
            } else {
                uint32_t row1 = row, r1 = r;
                for (uint32_t j = 0; j < 16; j++) {
                    if (i0 + j >= lo && i0 + j < hi && r1 < border) *(uint8_t *)(d0 + row1 * run + r1) = (uint8_t)(o.w[j >> 2] >> (8 * (j & 3u)));
                    if (++r1 == stride) { r1 = 0; row1++; }
                }
            }
        }
        r += sr;
        row += srow;
        if (r >= stride) { r -= stride; if (PLANT != kPlantSliceRowNotAdvanced) row++; }
    }
}

// ---- a fragment's piece against a strided slice of the caller's buffer (CSAMI_DeviceReadIntoSlices, CSAMI_DeviceCompareSlices) ----
//
// The caller's side of entry i is what a checked Slice selects of a buffer: packed byte p of the entry lies at buffer offset
// offset + (p / run) * stride + p % run.  The pieces stay on the fixed kFragPiece grid of the decoded (packed) fragment, so a
// piece's source is contiguous and its side in the buffer is the tail of one run, a gap and the head of the next -- or, where run
// is small, many of them.  The host plans a piece with gather_whole / gather_reduce (csa_dev_write.h), as the write does; spread_sum
// and compare_rows are the workgroup's.  With run < 16 every 16-byte unit crosses a run border and goes byte by byte: that is the
// slow path, and no rate is promised for it.

struct SpreadPiece {       // one workgroup of k_frag_spread / k_frag_compare_rows: a GatherPiece with src and dst exchanged
    const uint8_t *src;    // the piece of the decoded fragment, contiguous
    uint8_t *dst;          // stride == 0: the piece's one contiguous range in the caller's buffer (as a CopyPiece: NULL = summed only);
                           // else the address of period position 0, inside the hull (what lies in front of `phase` is not touched).
                           // k_frag_compare_rows only loads from it
    uint64_t stride;       // periodic: the address step from one run to the next, >= run
    uint32_t len;          // <= kFragPiece
    uint32_t phase;        // periodic: byte i of the piece is period position pos = phase + i; row = pos / run, r = pos % run; its
    uint32_t run;          //           place is dst + row * stride + r
    uint32_t cmp;          // k_frag_compare_rows: the leading bytes that are compared, <= len (periodic: > 0); k_frag_spread: 0, unused
    const uint8_t *lo, *hi;   // periodic: the slice's hull [lo, hi): all that a load window of k_frag_compare_rows may touch
};

// Thread `tid` of `nthreads`: its share of a periodic piece, the transpose of gather_sum.  The anchor is the SOURCE, as in slice_sum:
// up to 15 head bytes bring it to a 16-byte line and up to 15 tail bytes end the piece, byte by byte; between them every unit is
// one aligned 16-byte load, so no load window ever leaves src[0, len).  Every byte is loaded once and summed as one piece of len
// bytes: exactly copy_sum<false, true>'s sums.  A unit whose 16 packed bytes fall in one run goes out as 16 bytes -- one store,
// four, or sixteen, as its destination's alignment allows; a unit across a run border goes out byte by byte, row segment by row
// segment.  Nothing but the places of the piece's bytes is stored to: no gap byte, nothing outside the hull.  No division in the
// unit loop: a thread's (row, r) advances by the workgroup's step, 16 * nthreads packed positions, with one carry.
template <int PLANT = kPlantNone>
CSADEV_FHD void spread_sum(const SpreadPiece &pc, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b)
{
    const uint8_t *src = pc.src;
    uint8_t *dst = pc.dst;
    const uint32_t n = pc.len, run = pc.run;
    const uint64_t stride = pc.stride;
    uint32_t head = (0u - (uint32_t)(uintptr_t)src) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = (n - head) & 15u;
    auto one = [&](uint32_t idx) {
        const uint32_t v = src[idx];
        const uint32_t pos = pc.phase + idx, row = pos / run, r = pos - row * run;
        dst[row * stride + r] = (uint8_t)v;
        a += v;
        b += (uint64_t)(n - idx) * v;
    };
    if (tid < head) one(tid);
    if (nthreads - 1 - tid < tail) one(head + 16 * units + (nthreads - 1 - tid));
    if (tid >= units) return;
    const uint32_t step = 16 * nthreads, srow = step / run, sr = step - srow * run;
    const uint32_t border = PLANT == kPlantSpreadBorderLate ? run + 1 : run;         // r == border: the next row begins
    const uint32_t pos = (PLANT == kPlantSpreadPhaseDropped ? 0u : pc.phase) + head + 16 * tid;
    uint32_t row = pos / run, r = pos - row * run;
    for (uint32_t i = tid; i < units; i += nthreads) {
        const uint32_t i0 = head + 16 * i;
        const Vec16 o = *(const Vec16 *)(src + i0);                   // (aligned: the anchor is src)
        sum_word(o.w[0], i0, n, a, b);
        sum_word(o.w[1], i0 + 4, n, a, b);
        sum_word(o.w[2], i0 + 8, n, a, b);
        sum_word(o.w[3], i0 + 12, n, a, b);
        uint8_t *d = dst + row * stride + r;
        if (PLANT == kPlantSpreadStraddleWhole ? r < run : r + 16 <= run) {
            if (!((uintptr_t)d & 15u)) {
                *(Vec16 *)d = o;
            } else if (!((uintptr_t)d & 3u)) {
                for (uint32_t j = 0; j < 4; j++) ((uint32_t *)d)[j] = o.w[j];
            } else {
                for (uint32_t j = 0; j < 16; j++) d[j] = (uint8_t)(o.w[j >> 2] >> (8 * (j & 3u)));
            }
        } else {
            uint32_t r1 = r;
            for (uint32_t j = 0; j < 16; j++) {
                *d++ = (uint8_t)(o.w[j >> 2] >> (8 * (j & 3u)));
                if (++r1 == border) { r1 = 0; d += stride - run; }
            }
        }
        r += sr;
        row += srow;
        if (r >= run) { r -= run; if (PLANT != kPlantSpreadRowNotAdvanced) row++; }
    }
}

// Thread `tid` of `nthreads`: its share of a periodic piece of k_frag_compare_rows.  x = pc.src, the fragment's piece, is the anchor,
// as in compare_sum; its first pc.cmp bytes are compared with the rows of the caller's buffer and the rest summed only, the two
// parts' sums joined as compare_piece joins them.  A unit whose 16 packed bytes fall in one run loads the caller's 16 bytes with
// load_window, checked against the HULL -- gap bytes may be loaded; they are never compared -- and a unit across a run border takes
// them byte by byte, row segment by row segment.  The first differing byte of a unit comes off the XOR of its words.  `first`: the
// smallest index below cmp at which THIS thread saw a difference, else len.  Nothing outside the hull is loaded, not even by an
// aligned 16-byte window, and nothing is stored.
template <int PLANT = kPlantNone>
CSADEV_FHD void compare_rows(const SpreadPiece &pc, uint32_t tid, uint32_t nthreads, uint64_t &a, uint64_t &b, uint32_t &first)
{
    const uint8_t *x = pc.src, *y = pc.dst;
    const uint32_t n = pc.cmp, run = pc.run;
    const uint64_t stride = pc.stride;
    uint32_t head = (0u - (uint32_t)(uintptr_t)x) & 15u;
    if (head > n) head = n;
    const uint32_t units = (n - head) >> 4, tail = (n - head) & 15u;
    uint64_t fa = 0, fb = 0;
    uint32_t f = n;
    auto one = [&](uint32_t idx, bool compared) {
        const uint32_t v = x[idx];
        const uint32_t pos = pc.phase + idx, row = pos / run, r = pos - row * run;
        if (compared && v != y[row * stride + r] && idx < f) f = idx;
        fa += v;
        fb += (uint64_t)(n - idx) * v;
    };
    if (tid < head) one(tid, PLANT != kPlantRowsHeadNotCompared);
    if (nthreads - 1 - tid < tail) one(head + 16 * units + (nthreads - 1 - tid), true);
    if (tid < units) {
        const uint32_t step = 16 * nthreads, srow = step / run, sr = step - srow * run;
        const uint32_t pos = pc.phase + head + 16 * tid;
        uint32_t row = pos / run, r = pos - row * run;
        for (uint32_t i = tid; i < units; i += nthreads) {
            const uint32_t i0 = head + 16 * i;
            const Vec16 p = *(const Vec16 *)(x + i0);
            const uint8_t *q0 = y + row * stride + r;
            Vec16 q;
            if (r + 16 <= run) {
                q = load_window<PLANT == kPlantRowsWindowPastHull>(q0, pc.lo, pc.hi);
            } else {
                q = Vec16{{0, 0, 0, 0}};
                uint32_t r1 = r;
                for (uint32_t j = 0; j < 16; j++) {
                    q.w[j >> 2] |= (uint32_t)*q0++ << (8 * (j & 3u));
                    if (++r1 == run) { r1 = 0; q0 += stride - run; }
                }
            }
            const uint64_t lo = ((uint64_t)(p.w[1] ^ q.w[1]) << 32) | (p.w[0] ^ q.w[0]), hi = ((uint64_t)(p.w[3] ^ q.w[3]) << 32) | (p.w[2] ^ q.w[2]);
            if (lo | hi) {
                const uint32_t at = i0 + (lo ? (uint32_t)__builtin_ctzll(lo) >> 3 : 8u + ((uint32_t)__builtin_ctzll(hi) >> 3));
                if (at < f) f = at;
            }
            sum_word(p.w[0], i0, n, fa, fb);
            sum_word(p.w[1], i0 + 4, n, fa, fb);
            sum_word(p.w[2], i0 + 8, n, fa, fb);
            sum_word(p.w[3], i0 + 12, n, fa, fb);
            r += sr;
            row += srow;
            if (r >= run) { r -= run; row++; }
        }
    }
    a += fa;
    b += fb + (uint64_t)(pc.len - n) * fa;
    first = f < n ? f : pc.len;
    if (n < pc.len) copy_sum<false, true>(nullptr, x + n, pc.len - n, tid, nthreads, a, b);
}

// The first differing offset of a fragment of `size` delivered bytes from its pieces' `first` values (first(k): piece k's, its
// length where the piece saw none): first_piece_index * kFragPiece + first, or `size` if no piece saw one
template <int PLANT = kPlantNone, class First>
CSADEV_FHD uint64_t fold_first(First first, uint32_t npieces, uint64_t size)
{
    for (uint32_t k = 0; k < npieces; k++) {
        const uint64_t left = size - (uint64_t)k * kFragPiece, len = left < kFragPiece ? left : kFragPiece;
        const uint32_t f = first(k);
        if (f < len) return (uint64_t)(PLANT == kPlantFirstPieceIndex ? 0u : k) * kFragPiece + f;
    }
    return size;
}

// adler32 (seed 0) of a fragment of `size` bytes from the sums of its piece_count(size, kFragPiece) consecutive pieces; sums(k)
// returns piece k's PieceSums
template <int PLANT = kPlantNone, class Sums>
CSADEV_FHD uint32_t fold_pieces(Sums sums, uint32_t npieces, uint64_t size)
{
    uint64_t a = 0, b = 0;
    for (uint32_t k = 0; k < npieces; k++) {
        uint64_t left = size - (uint64_t)(PLANT == kPlantFoldLastLen ? npieces - 1 : k) * kFragPiece;
        const uint64_t len = left < kFragPiece ? left : kFragPiece;
        const PieceSums s = sums(k);
        b = (b + len * a + s.b % kAdlerBase) % kAdlerBase;
        a = (a + s.a % kAdlerBase) % kAdlerBase;
    }
    return (uint32_t)(a | (b << 16));
}

}  // namespace csadev
