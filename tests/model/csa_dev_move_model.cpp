// csa_dev_move_model.cpp -- the move layer of CSAMI_DeviceUpdateInPlace (csc_amd/csrc/csa_dev_move.h) on the CPU: plan_moves and the
// text one thread of k_move_extents runs, over a buffer allocated exactly as large as the archive, so that the sanitizers see every
// byte loaded or stored outside it.  tests/test_archive_inplace_host.py builds it with g++ -fsanitize=address,undefined and runs it.
//
// A phase is simulated the way the kernel runs it: tickets are handed out in order; at most K workgroups are resident (have drawn
// a ticket and not yet stored); a resident workgroup LOADS (its whole chunk into MoveRegs, all 256 threads) and thereby sets its
// flag; it may STORE once it has loaded and the flags lo..hi of its chunk are set.  Three kinds of schedule choose among the steps
// that are possible: every store as early as allowed, every store as late as possible (all loads of the phase first, the stores
// then in reverse), and seeded random choices with K = 1, 2, 3, 7 resident.  A schedule in which no step is possible is a deadlock
// -- what a wait for a higher ticket would give -- and fails the case.  Every case is compared with the copy that reads every
// source before it writes any destination, and every plan is checked for what the header promises: a chunk's destination meets
// only its own source and sources of lower tickets, and those lie in [lo, hi].
//
// argv[1]: the planted mistake (MovePlant; 0: none).  Prints "ok <cases>" and returns 0, or "FAIL <case>: <what>" and returns 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csa_dev_move.h"

using namespace csadev;

namespace {

int g_plant = 0;
int g_cases = 0;

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

[[noreturn]] void fail(const std::string &name, const std::string &what)
{
    printf("FAIL %s: %s\n", name.c_str(), what.c_str());
    fflush(stdout);
    exit(3);
}

void plan(const std::vector<Move> &in, MovePlan &P)
{
    switch (g_plant) {
    case kMPlantHiShort: plan_moves<kMPlantHiShort>(in, P); break;
    case kMPlantRightAscending: plan_moves<kMPlantRightAscending>(in, P); break;
    case kMPlantNoParking: plan_moves<kMPlantNoParking>(in, P); break;
    case kMPlantCoalesceUnequal: plan_moves<kMPlantCoalesceUnequal>(in, P); break;
    default: plan_moves<kMPlantNone>(in, P); break;
    }
}

void check_plan(const std::string &name, const MovePlan &P, uint64_t size)
{
    for (int ph = 0; ph < 2; ph++) {
        const std::vector<MoveChunk> &c = P.phase[ph];
        for (size_t i = 0; i < c.size(); i++) {
            if (c[i].len == 0 || c[i].len > kMoveChunk) fail(name, "a chunk of no bytes or of more than kMoveChunk");
            if (c[i].src + c[i].len > size || c[i].dst + c[i].len > size) fail(name, "plan: a chunk leaves the buffer");
            if (ph == 0 ? c[i].dst >= c[i].src : c[i].dst <= c[i].src) fail(name, "a chunk in the wrong phase");
            if (c[i].lo != kMoveNone && !(c[i].lo <= c[i].hi && c[i].hi < i)) fail(name, "a chunk waits for its own or a higher ticket");
            for (size_t j = 0; j < c.size(); j++) {
                if (j == i || !move_meets(c[i].dst, c[i].len, c[j].src, c[j].len)) continue;
                if (j > i) fail(name, "plan: a chunk's destination meets the source of a higher ticket");
                if (c[i].lo == kMoveNone || j < c[i].lo || j > c[i].hi) fail(name, "plan: a chunk's destination meets a lower ticket outside [lo, hi]");
            }
        }
    }
}

struct Group { MoveRegs r[kThreads]; };

void wg_load(const MoveChunk &c, uint8_t *buf, uint64_t size, Group &g)
{
    for (uint32_t t = 0; t < kThreads; t++) {
        if (g_plant == kMPlantStoreEarly) move_load<kMPlantStoreEarly>(c, buf, buf, buf + size, t, kThreads, g.r[t]);
        else move_load<kMPlantNone>(c, buf, buf, buf + size, t, kThreads, g.r[t]);
    }
}

void wg_store(const MoveChunk &c, uint8_t *buf, const Group &g)
{
    for (uint32_t t = 0; t < kThreads; t++) move_store(c, buf, t, kThreads, g.r[t]);
}

enum Sched { kEarly, kLate, kRandom };

// one phase under one schedule; false: deadlock
bool run_phase(const std::vector<MoveChunk> &c, uint8_t *buf, uint64_t size, Sched sched, uint32_t K, Rng &rng)
{
    const size_t n = c.size();
    std::vector<Group *> regs(n, nullptr);
    std::vector<uint8_t> state(n, 0);                  // 0: not loaded, 1: loaded (flag set), 2: stored
    auto ready = [&](size_t i) {
        if (state[i] != 1) return false;
        if (c[i].lo == kMoveNone) return true;
        for (uint32_t j = c[i].lo; j <= c[i].hi; j++) if (!state[j]) return false;
        return true;
    };
    auto load = [&](size_t i) { regs[i] = new Group(); wg_load(c[i], buf, size, *regs[i]); state[i] = 1; };
    auto store = [&](size_t i) { wg_store(c[i], buf, *regs[i]); delete regs[i]; regs[i] = nullptr; state[i] = 2; };
    bool ok = true;
    if (sched == kEarly) {
        for (size_t i = 0; i < n && ok; i++) { load(i); if (ready(i)) store(i); else ok = false; }
    } else if (sched == kLate) {
        for (size_t i = 0; i < n; i++) load(i);
        for (size_t i = n; i-- > 0 && ok;) { if (ready(i)) store(i); else ok = false; }
    } else {
        size_t admitted = 0, done = 0;                 // tickets [0, admitted) have been drawn
        std::vector<size_t> resident;
        while (done < n && ok) {
            std::vector<std::pair<int, size_t>> steps;     // (0: admit the next ticket, 1: load, 2: store; which resident)
            if (admitted < n && resident.size() < K) steps.push_back({0, 0});
            for (size_t k = 0; k < resident.size(); k++) {
                if (state[resident[k]] == 0) steps.push_back({1, k});
                else if (ready(resident[k])) steps.push_back({2, k});
            }
            if (steps.empty()) { ok = false; break; }
            const auto s = steps[rng.below((uint32_t)steps.size())];
            if (s.first == 0) resident.push_back(admitted++);
            else if (s.first == 1) load(resident[s.second]);
            else { store(resident[s.second]); resident.erase(resident.begin() + (int64_t)s.second); done++; }
        }
    }
    for (Group *g : regs) delete g;
    return ok;
}

struct Stats { uint64_t moves, moved_bytes, parked_moves, parked_bytes; };

// the case: the moves inside a buffer of exactly `size` bytes, under every schedule
Stats run_case(const std::string &name, const std::vector<Move> &moves, uint64_t size)
{
    g_cases++;
    printf("case %s\n", name.c_str());
    MovePlan P;
    plan(moves, P);
    check_plan(name, P, size);
    std::vector<uint8_t> init(size), want;
    Rng fill{0x9E3779B97F4A7C15ull ^ size};
    for (uint8_t &b : init) b = (uint8_t)(fill.next() >> 7);
    want = init;
    for (const Move &m : moves) {
        if (m.src + m.len > size || m.dst + m.len > size) fail(name, "the case itself leaves the buffer");
        memcpy(want.data() + m.dst, init.data() + m.src, m.len);
    }
    struct Run { Sched s; uint32_t K; uint64_t seed; const char *what; };
    const Run runs[] = {{kEarly, 0, 0, "early"}, {kLate, 0, 0, "late"}, {kRandom, 1, 11, "random K=1"}, {kRandom, 2, 12, "random K=2"},
                        {kRandom, 3, 13, "random K=3"}, {kRandom, 7, 14, "random K=7"}};
    for (const Run &r : runs) {
        uint8_t *buf = (uint8_t *)malloc(size ? size : 1);        // exactly the archive: the sanitizer's red zone begins behind it
        memcpy(buf, init.data(), size);
        Rng rng{r.seed * 0x2545F4914F6CDD1Dull + size};
        std::vector<std::vector<uint8_t>> park;
        for (const Move &m : P.parked) park.emplace_back(buf + m.src, buf + m.src + m.len);
        for (int ph = 0; ph < 2; ph++)
            if (!run_phase(P.phase[ph], buf, size, r.s, r.K, rng)) { free(buf); fail(name, std::string("deadlock under ") + r.what); }
        for (size_t k = 0; k < P.parked.size(); k++) memcpy(buf + P.parked[k].dst, park[k].data(), park[k].size());
        const bool same = memcmp(buf, want.data(), size) == 0;
        free(buf);
        if (!same) fail(name, std::string("bytes differ under ") + r.what);
    }
    return Stats{P.moves, P.moved_bytes, P.parked_moves, P.parked_bytes};
}

// streams of the given sizes back to back from `base` on, moved to where the sizes `now` of what lies in front put them
// (gone[i]: stream i is not reused -- it is encoded anew, and its new size is now[i])
std::vector<Move> relayout(const std::vector<uint64_t> &was, const std::vector<uint64_t> &now, const std::vector<bool> &gone, uint64_t base, uint64_t &size)
{
    std::vector<Move> mv;
    uint64_t s = base, d = base;
    for (size_t i = 0; i < was.size(); i++) {
        if (!gone[i]) mv.push_back(Move{s, d, was[i]});
        s += was[i];
        d += gone[i] ? now[i] : was[i];
    }
    size = std::max(s, d);
    return mv;
}

}   // namespace

int main(int argc, char **argv)
{
    g_plant = argc > 1 ? atoi(argv[1]) : 0;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int64_t C = kMoveChunk;
    char name[128];

    // 1. one move of three chunks and five bytes, every shift
    const int64_t L = 3 * C + 5;
    const int64_t shifts[] = {1, -1, 15, -15, 16, -16, 17, -17, C - 1, -(C - 1), C, -C, C + 1, -(C + 1), L + 7, -(L + 7)};
    for (int64_t sh : shifts) {
        const uint64_t src = sh < 0 ? (uint64_t)-sh + 3 : 3, dst = (uint64_t)((int64_t)src + sh);
        snprintf(name, sizeof(name), "shift=%lld len=%lld", (long long)sh, (long long)L);
        run_case(name, {Move{src, dst, (uint64_t)L}}, std::max(src, dst) + (uint64_t)L);
    }
    // 2. every length, overlapping its own source in either direction
    const int64_t lens[] = {1, 15, 16, 17, C - 1, C + 1, L};
    for (int64_t len : lens)
        for (int64_t sh : {1, -1, 17, -17}) {
            const uint64_t src = sh < 0 ? (uint64_t)-sh : 0, dst = (uint64_t)((int64_t)src + sh);
            snprintf(name, sizeof(name), "len=%lld shift=%lld", (long long)len, (long long)sh);
            run_case(name, {Move{src, dst, (uint64_t)len}}, std::max(src, dst) + (uint64_t)len);
        }
    // 3. one short move, every pair of alignments (the shift is 16 + da - sa: the two ranges overlap)
    for (uint32_t sa = 0; sa < 16; sa++)
        for (uint32_t da = 0; da < 16; da++) {
            snprintf(name, sizeof(name), "align sa=%u da=%u", sa, da);
            run_case(name, {Move{32 + sa, 48 + da, 100}}, 48 + da + 100);
        }
    // 4. forty streams in id order, one in front grown and one shrunk: nothing is parked
    {
        std::vector<uint64_t> was, now;
        std::vector<bool> gone(40, false);
        Rng r{40};
        for (int i = 0; i < 40; i++) { was.push_back(1000 + r.below(60000)); now.push_back(was.back()); }
        gone[1] = gone[7] = true;
        now[1] = was[1] + 333;
        now[7] = was[7] - 900;
        uint64_t size;
        const std::vector<Move> mv = relayout(was, now, gone, 24, size);
        const Stats s = run_case("id order: 40 streams, one grown, one shrunk", mv, size);
        if (s.parked_moves != 0) fail("id order: 40 streams, one grown, one shrunk", "a move was parked");
        if (s.moves != 2) fail("id order: 40 streams, one grown, one shrunk", "neighbours of one shift were not coalesced");
    }
    // 5. random archives in id order: whatever changed size, nothing is parked
    for (int k = 0; k < 30; k++) {
        Rng r{1000 + (uint64_t)k};
        const int n = 2 + (int)r.below(20);
        std::vector<uint64_t> was, now;
        std::vector<bool> gone;
        for (int i = 0; i < n; i++) {
            was.push_back(1 + r.below(k % 3 ? 3000 : 70000));
            gone.push_back(r.below(3) == 0);
            now.push_back(gone.back() ? 1 + r.below(2 * (uint32_t)was.back()) : was.back());
        }
        uint64_t size;
        const std::vector<Move> mv = relayout(was, now, gone, 24, size);
        snprintf(name, sizeof(name), "id order: random %d", k);
        if (run_case(name, mv, size).parked_moves != 0) fail(name, "a move was parked");
    }
    // 6. two streams that swap places: the one that moves right is parked
    {
        const uint64_t a = 50000, b = 41000;
        const Stats s = run_case("swap", {Move{24, 24 + b, a}, Move{24 + a, 24, b}}, 24 + a + b);
        if (g_plant != kMPlantNoParking && s.parked_moves != 1) fail("swap", "the stream that moves right was not parked");
    }
    // 7. three streams whose extents of 1, 2, 9, 10, 11 and 4097 bytes were dealt out in turn, brought back to back in id order
    {
        const uint64_t cut[] = {1, 2, 9, 10, 11, 4097};
        const uint64_t total[3] = {90000, 61234, 33333};
        std::vector<std::vector<Move>> per(3);
        uint64_t left[3] = {total[0], total[1], total[2]}, pos = 24, done[3] = {0, 0, 0};
        for (size_t k = 0; left[0] || left[1] || left[2]; k++) {
            const size_t t = k % 3;
            if (!left[t]) continue;
            const uint64_t n = std::min(left[t], cut[(k / 3) % 6]);
            per[t].push_back(Move{pos, done[t], n});
            pos += n; left[t] -= n; done[t] += n;
        }
        std::vector<Move> mv;
        uint64_t at = 24 + 77;                      // (something in front grew by 77 bytes)
        for (size_t t = 0; t < 3; t++) {
            for (Move m : per[t]) { m.dst += at; mv.push_back(m); }
            at += total[t];
        }
        run_case("interleaved extents", mv, std::max(pos, at));
    }
    // 8. seeded random lists: disjoint sources, disjoint destinations, nothing else
    for (int k = 0; k < 200; k++) {
        Rng r{77000 + (uint64_t)k};
        const int n = 1 + (int)r.below(12);
        const uint32_t big = k % 4 == 0 ? 80000 : 2000;
        std::vector<uint64_t> len, sgap, dgap;
        for (int i = 0; i < n; i++) { len.push_back(1 + r.below(big)); sgap.push_back(r.below(3) ? r.below(40) : 0); dgap.push_back(r.below(3) ? r.below(40) : 0); }
        std::vector<int> order(n);
        for (int i = 0; i < n; i++) order[i] = i;
        for (int i = n - 1; i > 0; i--) std::swap(order[i], order[r.below((uint32_t)i + 1)]);
        std::vector<Move> mv(n);
        uint64_t s = r.below(20), d = r.below(20);
        for (int i = 0; i < n; i++) { s += sgap[i]; mv[i].src = s; mv[i].len = len[i]; s += len[i]; }
        for (int i = 0; i < n; i++) { const int j = order[i]; d += dgap[i]; mv[j].dst = d; d += len[j]; }
        snprintf(name, sizeof(name), "random %d", k);
        run_case(name, mv, std::max(s, d));
    }
    printf("ok %d\n", g_cases);
    return 0;
}
