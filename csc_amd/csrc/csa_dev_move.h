// csa_dev_move.h -- the move layer of CSAMI_DeviceUpdateInPlace (include/csa_mi355x.h): the streams an update reuses change their
// places INSIDE the one buffer the archive lives in.  The host half (plan_moves) turns a list of moves into at most two phases of
// chunks and a list of parked moves; the device half (move_load, move_store) is what one thread of k_move_extents
// (csa_dev_kernels.hip) does with its share of a chunk.  Compiles for the host (plain C++: tests/test_archive_inplace_host.py runs
// tests/model/csa_dev_move_model.cpp with g++ and the sanitizers) and for the device, so the model runs the text the kernel runs.
//
// The contract is that of reading every source first and writing every destination afterwards.  Sources are pairwise disjoint and
// destinations are pairwise disjoint; a destination may meet any source, its own included.  How the order comes about:
//
//   left moves  (dst < src) are cut into chunks and the chunks sorted by source address, ASCENDING.  A chunk's place in that order
//               is its ticket.  Chunk i stores to [d, d + n) with d < s_i, so d + n < s_i + n <= s_j for every j > i (sources are
//               disjoint and sorted): a chunk's destination meets only its own source and sources of LOWER tickets.  And a lower
//               ticket j stores below s_j + n_j <= s_i: nothing is stored into a source before its own chunk, or a higher one, does.
//   right moves (dst > src) are the mirror image: sorted DESCENDING, and the same two sentences hold.
//   the phases  run one after the other, left first.  A left chunk may store into the source of a right move, which would then be
//               read too late: such a right move is PARKED -- copied to scratch before the left phase and placed from there after the
//               right phase.  A right chunk that stores into the source of a left move does no harm: that source has been read.
//
// Inside a phase chunk i may store once the chunks whose sources its destination meets have LOADED (write after read; no byte is
// handed from one workgroup to another).  Those chunks are a contiguous ticket range [lo, hi], hi < i, found by binary search.
//
// kMoveChunk is 32 KiB: 256 lanes x 8 units x 16 bytes, so a whole chunk sits in 32 payload registers a lane between its last load
// and its first store -- which is what makes a chunk whose destination overlaps its own source safe without any order among its
// lanes -- and the kernel stays at or below 64 VGPRs, so eight waves a SIMD can be resident.  16 KiB would double the tickets and the
// flag traffic for the same bytes; 64 KiB would double the registers a lane holds.
//
// The template parameter PLANT switches one deliberate mistake on (0: none).  The product instantiates 0 only; the model runs each
// of the others and has to see it caught by a named case.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "csa_dev_read.h"

namespace csadev {

constexpr uint32_t kMoveChunk = 32768;
constexpr uint32_t kMoveUnits = kMoveChunk / (16 * kThreads);      // 16-byte units a lane holds
constexpr uint32_t kMoveNone = 0xFFFFFFFFu;                         // MoveChunk::lo of a chunk that waits for nobody
constexpr uint32_t kMoveStateWords = 4;                             // k_move_extents' state block: ticket counter, error word, two of padding; then the flags

enum MovePlant {
    kMPlantNone = 0, kMPlantHiShort = 1, kMPlantRightAscending = 2, kMPlantNoParking = 3, kMPlantCoalesceUnequal = 4, kMPlantStoreEarly = 5
};

struct Move { uint64_t src, dst, len; };       // offsets into the one buffer

struct MoveChunk {         // one workgroup of k_move_extents; its index in the phase's table is its ticket
    uint64_t src, dst;     // offsets into the buffer
    uint32_t len;          // <= kMoveChunk
    uint32_t lo, hi;       // the tickets, all lower than its own, whose sources its destination meets; lo == kMoveNone: none
    uint32_t pad;
};

struct MovePlan {
    std::vector<Move> parked;              // read before the left phase, written after the right phase
    std::vector<MoveChunk> phase[2];       // left, right: in ticket order
    uint64_t moves = 0, moved_bytes = 0;   // after dropping src == dst and coalescing; the parked ones included
    uint64_t parked_moves = 0, parked_bytes = 0;
};

inline bool move_meets(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return an && bn && a < b + bn && b < a + an; }

// The chunks of one phase's moves, in ticket order, each with its range of tickets to wait for.
template <int PLANT = kMPlantNone>
inline void move_phase(const std::vector<Move> &moves, bool right, std::vector<MoveChunk> &out)
{
    out.clear();
    for (const Move &m : moves)
        for (uint64_t off = 0; off < m.len; off += kMoveChunk)
            out.push_back(MoveChunk{m.src + off, m.dst + off, (uint32_t)std::min<uint64_t>(m.len - off, kMoveChunk), kMoveNone, 0, 0});
    const bool descending = right && PLANT != kMPlantRightAscending;
    std::sort(out.begin(), out.end(), [descending](const MoveChunk &a, const MoveChunk &b) { return descending ? a.src > b.src : a.src < b.src; });
    for (size_t i = 0; i < out.size(); i++) {
        MoveChunk &c = out[i];
        const uint64_t d = c.dst, e = c.dst + c.len;
        const auto b0 = out.begin(), bi = out.begin() + (int64_t)i;
        // among the lower tickets the ones whose source meets [d, e) are consecutive: the sources are disjoint and sorted
        int64_t lo, hi;
        if (!right) {
            lo = std::partition_point(b0, bi, [d](const MoveChunk &x) { return x.src + x.len <= d; }) - b0;
            hi = std::partition_point(b0, bi, [e](const MoveChunk &x) { return x.src < e; }) - b0 - 1;
        } else {
            lo = std::partition_point(b0, bi, [e](const MoveChunk &x) { return x.src >= e; }) - b0;
            hi = std::partition_point(b0, bi, [d](const MoveChunk &x) { return x.src + x.len > d; }) - b0 - 1;
        }
        if (PLANT == kMPlantHiShort) hi--;
        if (lo <= hi) { c.lo = (uint32_t)lo; c.hi = (uint32_t)hi; }
    }
}

// The plan of a move list (sources pairwise disjoint, destinations pairwise disjoint, everything inside one buffer; a list the
// caller has checked).  Moves of no bytes and moves that stay where they are are dropped, neighbours whose sources AND destinations
// are adjacent become one move.
template <int PLANT = kMPlantNone>
inline void plan_moves(std::vector<Move> in, MovePlan &P)
{
    P = MovePlan();
    in.erase(std::remove_if(in.begin(), in.end(), [](const Move &m) { return !m.len || m.src == m.dst; }), in.end());
    std::sort(in.begin(), in.end(), [](const Move &a, const Move &b) { return a.src < b.src; });
    std::vector<Move> all;
    for (const Move &m : in) {
        if (!all.empty() && all.back().src + all.back().len == m.src
            && (PLANT == kMPlantCoalesceUnequal || all.back().dst + all.back().len == m.dst)) all.back().len += m.len;
        else all.push_back(m);
    }
    std::vector<Move> side[2];
    for (const Move &m : all) { side[m.dst < m.src ? 0 : 1].push_back(m); P.moves++; P.moved_bytes += m.len; }
    // a right move whose source a left move stores into is parked: the left moves' destinations, sorted, and one search a right move
    std::vector<Move> ld = side[0], right;
    std::sort(ld.begin(), ld.end(), [](const Move &a, const Move &b) { return a.dst < b.dst; });
    for (const Move &m : side[1]) {
        auto it = std::partition_point(ld.begin(), ld.end(), [&m](const Move &x) { return x.dst + x.len <= m.src; });
        if (PLANT != kMPlantNoParking && it != ld.end() && move_meets(it->dst, it->len, m.src, m.len)) {
            P.parked.push_back(m);
            P.parked_moves++;
            P.parked_bytes += m.len;
        } else right.push_back(m);
    }
    move_phase<PLANT>(side[0], false, P.phase[0]);
    move_phase<PLANT>(right, true, P.phase[1]);
}

// ---- one thread of k_move_extents ----
//
// The anchor is the destination: up to 15 head bytes bring it to a 16-byte line and up to 15 tail bytes end the chunk, byte by
// byte; between them every unit is one aligned 16-byte store of source bytes funnel-shifted into place from two aligned 16-byte
// loads (load_window: where that 32-byte window would leave the BUFFER [lo, hi), the 16 bytes one by one).  A window may hold bytes
// of a neighbouring chunk's source, which another workgroup may be storing to at that moment: the funnel shift drops them, no byte
// outside the chunk's own source reaches a store.  move_load is the whole chunk into registers; move_store is every store.

struct MoveRegs { Vec16 u[kMoveUnits]; uint32_t head, tail; };

CSADEV_FHD uint32_t move_head(const MoveChunk &c, const uint8_t *buf)
{
    const uint32_t head = (0u - (uint32_t)(uintptr_t)(buf + c.dst)) & 15u;
    return head > c.len ? c.len : head;
}

template <int PLANT = kMPlantNone>
CSADEV_FHD void move_load(const MoveChunk &c, uint8_t *buf, const uint8_t *lo, const uint8_t *hi, uint32_t tid, uint32_t nthreads, MoveRegs &r)
{
    const uint8_t *src = buf + c.src;
    const uint32_t n = c.len, head = move_head(c, buf), units = (n - head) >> 4, tail = (n - head) & 15u;
    r.head = r.tail = 0;
    for (uint32_t k = 0; k < kMoveUnits; k++) r.u[k] = Vec16{{0, 0, 0, 0}};
    if (tid < head) r.head = src[tid];
    if (nthreads - 1 - tid < tail) r.tail = src[head + 16 * units + (nthreads - 1 - tid)];
    // Source alignment is one number for the whole chunk, so which of the three forms loads it is uniform.
    const uint8_t *s0 = src + head;
    const uint32_t m = (uint32_t)(uintptr_t)s0 & 15u;
    const uint8_t *w0 = s0 - m, *w1 = s0 + 16ull * units + (m ? 16 - m : 0);      // every unit's load window lies in [w0, w1)
    auto each = [&](auto load) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < kMoveUnits; k++) {
            // (a lane without a unit k loads the chunk's last unit once more and never stores it: no branch parts one unit's loads
            // from the next's, so all of a lane's loads are in flight together)
            const uint32_t i = tid + k * nthreads, ii = i < units ? i : units - 1;
            r.u[k] = load(ii);
            if (PLANT == kMPlantStoreEarly && k == 0 && i < units) *(Vec16 *)(buf + c.dst + head + 16 * i) = r.u[k];
        }
    };
    if (!units) return;
    if (m == 0) each([&](uint32_t i) { return *(const Vec16 *)(s0 + 16 * i); });
    else if (w0 >= lo && w1 <= hi) each([&](uint32_t i) { return funnel16(*(const Vec16 *)(w0 + 16 * i), *(const Vec16 *)(w0 + 16 * i + 16), m); });
    else each([&](uint32_t i) { return load_window(s0 + 16 * i, lo, hi); });       // (a chunk at the buffer's edge)
}

CSADEV_FHD void move_store(const MoveChunk &c, uint8_t *buf, uint32_t tid, uint32_t nthreads, const MoveRegs &r)
{
    uint8_t *dst = buf + c.dst;
    const uint32_t n = c.len, head = move_head(c, buf), units = (n - head) >> 4, tail = (n - head) & 15u;
    if (tid < head) dst[tid] = (uint8_t)r.head;
    if (nthreads - 1 - tid < tail) dst[head + 16 * units + (nthreads - 1 - tid)] = (uint8_t)r.tail;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < kMoveUnits; k++) {
        const uint32_t i = tid + k * nthreads;
        if (i < units) *(Vec16 *)(dst + head + 16 * i) = r.u[k];
    }
}

}  // namespace csadev
