// csc_kernels_hp.inc -- the hash-bucket match finder of the lazy levels (1 / 2: csc_lz.cpp:156-199 over csc_mf.cpp:243-495 with a
// bucket of up to eight) as an INSERTER wavefront that runs ahead of the parser.  Included by csc_kernels.hip inside namespace
// cscmi.  tests/model/hp_model.c is this arrangement on the CPU, proven byte-identical to the oracle (tests/test_hp_model.py).
//
// The one-wavefront search (mf_find_match_ht) pays two dependent memory round trips per searched position on the parser's chain:
// the table gather and the candidates' bytes.  Neither depends on the parse:
//  * SPECULATIVE INSERTER (as in the level-3 pipeline, csc_kernels_dp4.inc, here for buckets of up to eight).  Every position of a
//    sub-block is inserted ahead of the parser with find_match's rule (HT2 / HT3 overwrite, bucket shifted by one with the position
//    in front; :365-366, :487-491), 64 positions per batch, one per lane: one gather, positions of a batch with the same key
//    resolved from the batch itself, the last position of a key stores.  SlidePos (:134-206) inserts the same words EXCEPT the
//    long-match skip (:145) and the same-hash no-shift rule (:150-156): the parser looks at the slid range's flags itself and
//    needs the inserter only where they are set (0.2 % of the slides on the configs[4] mix) -- then everything inserted beyond the
//    match's first byte is taken back (the records hold every word as the position found it) and SlidePos replayed exactly.
//  * RECORDS.  Distances as the position found the tables, which of them find_match looks at (strictly increasing distance,
//    :301-363, :453-485) and their match lengths capped at good_len: per position in LDS.  The parser compares the four rep
//    distances (sixteen positions per round trip), runs mf_find_match_ht's acceptance over rep + record slots -- four positions per
//    call, one per row of 16 lanes -- and extends a capped length on demand.

constexpr uint32_t kHpRec = 256;          // record ring (positions)
#ifndef HP_LA
#define HP_LA 128
#endif
constexpr uint32_t kHpLA = HP_LA;           // the inserter starts a batch while it is less than this far ahead of the parser
constexpr uint32_t kHpW = 8;              // bucket slots a record holds
constexpr uint32_t kHpSlots = 2 + kHpW;   // HT2, HT3, bucket
constexpr uint32_t kHpMultiMax = 768;      // launches with at most this many streams use this form (~47 KiB of LDS, three wavefronts a stream)
constexpr uint32_t ERR_HP_STALL = 0x40400000u;
static_assert(kHpLA + 64 <= kHpRec, "a batch must not overwrite the record the parser is reading");

struct HpX {
    uint32_t sb_seq, sb_ack, quit, abort;
    uint32_t sb0, pos0, size, pad;        // the open sub-block: window position / pos_ of its first byte, length
    uint32_t m_pos, ins_head;             // parser's position (sub-block offset); positions [0, ins_head) are in the tables and have records
    uint32_t ev_seq, ev_s, ev_len, ev_ack;   // "SlidePos(ev_s, ev_len) needs the inserter"
    uint32_t st_dev, st_ev, pad2[2];
    uint32_t r_dist[kHpSlots][kHpRec];    // [slot][position & 255]: 0 HT2, 1 HT3, 2.. bucket -- distance as the position found the table word
    uint8_t r_len[kHpSlots][kHpRec];      // match length capped at min(good_len, climit); 0 where find_match does not look
    uint16_t r_vm[kHpRec];                // which slots find_match looks at
    uint8_t r_hflag[kHpRec];              // SlidePos would not shift the bucket here (h6 == 0 or == h6 of the position before)
    uint32_t hS[2], hand[20];             // what the roles' own functions build their contexts from (end of this file)
};
struct EncLdsHp { EncLds base; HpX x; };
// the LDS image of a stream in this form, file-scope so that the roles' own functions address it directly
__shared__ EncLdsHp g_ldshp;
static_assert(3 * sizeof(EncLdsHp) <= kLdsPerCU, "kHpMultiMax counts on three workgroups a CU");
struct HpSb { uint32_t sb0, pos0, size; };

DEV HpX *hpx(Sc &c) { return reinterpret_cast<HpX *>(c.X); }

DEV bool hp_spin(Sc &c, HpX *X, uint32_t &spins, uint32_t site)
{
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 1023u) == 0 && (spins > (kDpSpinLimit << 2) || lds_vload(&X->abort))) {
        if (!lds_vload(&X->abort)) lds_vstore(&X->abort, ERR_HP_STALL | (site << 16) | (spins & 0xFFFFu));
        c.error = lds_vload(&X->abort);
        return false;
    }
    return true;
}

// positions [i0, i0 + n), n <= 64, of the open sub-block: find_match's inserts (csc_mf.cpp:365-366, :487-491) and their records
// Development aid (tools/ab_variant_other.sh): idle cycles in one role -- HP_PAD_PARSER a search, HP_PAD_INSERTER a batch of 64 positions, HP_PAD_CODER a token
// (lz.inc) -- say which wavefront the throughput hangs on.
template <int N> DEV void hp_pad() {
#pragma unroll 1
    for (int q = 0; q < N / 16; q++) asm volatile("s_nop 15");
}
DEV void hp_insert_batch(Sc &c, HpX *X, const HpSb &sb, uint32_t i0, uint32_t n, uint32_t &carry_h6)
{
    EncLds *L = c.L;
    const uint32_t lane = c.lane;
    const bool act = lane < n;
    const uint32_t p = i0 + lane, ai = p + 16;
    const uint64_t va = stage_load8(L->stage, ai);
    const uint32_t lo = (uint32_t)va, hi = (uint32_t)(va >> 32);
    const uint32_t h2 = hash2_of(lo), h3 = hash3_of(lo), h6 = hash6_mul(lo, hi) >> (32 - c.ht_bits);
    const uint32_t pos = sb.pos0 + p, wpos = sb.sb0 + p, limit = sb.size - p;
    const uint32_t W = umin(c.ht_width, c.ht_cyc);
    const uint32_t vld = c.vld_rge, good = c.good_len, wsz = c.wnd_size;
    gu32 *bk = c.ht6 + (size_t)h6 * c.ht_width;
    TM_DECL;
    // one gather, before any store of this batch
    uint32_t e2 = 0, e3 = 0, eb[kHpW];
#pragma unroll
    for (uint32_t t = 0; t < kHpW; t++) eb[t] = 0;
    if (act) {
        e2 = c.ht2[h2]; e3 = c.ht3[h3];
#pragma unroll
        for (uint32_t t = 0; t < kHpW; t++) if (t < W) eb[t] = bk[t];
    }
    // same-key positions inside the batch: the latest earlier lane of a key (HT2 / HT3), whether a later lane has it (that one
    // stores); for the bucket every earlier lane of the key shifts this lane's view -- walked over those lanes only
    bool l2 = false, l3 = false, l6 = false, b6 = false;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t k2 = rdlane(h2, j), k3 = rdlane(h3, j), k6 = rdlane(h6, j);
        const bool below = lane > j, above = lane < j;
        const uint32_t pj = sb.pos0 + i0 + j;
        e2 = (below && h2 == k2) ? pj : e2;
        e3 = (below && h3 == k3) ? pj : e3;
        b6 = b6 || (below && h6 == k6);
        l2 = l2 || (above && h2 == k2);
        l3 = l3 || (above && h3 == k3);
        l6 = l6 || (above && h6 == k6);
    }
    if (__ballot(b6 && act)) {
        for (uint64_t m = __ballot(l6 && act); m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctzll(m);
            const uint32_t k6 = rdlane(h6, j);
            const uint32_t pj = sb.pos0 + i0 + j;
            const bool s6 = lane > j && h6 == k6;
#pragma unroll
            for (uint32_t t = kHpW - 1; t > 0; t--) eb[t] = s6 ? eb[t - 1] : eb[t];
            eb[0] = s6 ? pj : eb[0];
        }
    }
    if (act) {
        if (!l2) c.ht2[h2] = pos;
        if (!l3) c.ht3[h3] = pos;
        if (!l6) {
            bk[0] = pos;
#pragma unroll
            for (uint32_t t = 1; t < kHpW; t++) if (t < W) bk[t] = eb[t - 1];
        }
    }
    TM_ADD(c, 0);
    // which candidates find_match looks at: strictly increasing distance (csc_mf.cpp:303, :334, :456)
    uint32_t dd[kHpSlots];
    dd[0] = pos - e2; dd[1] = pos - e3;
#pragma unroll
    for (uint32_t t = 0; t < kHpW; t++) dd[2 + t] = pos - eb[t];
    uint32_t vm = 0, M = 0;
#pragma unroll
    for (uint32_t t = 0; t < kHpSlots; t++) {
        const bool in = t < 2 + W && dd[t] > M;
        M = in ? dd[t] : M;
        vm |= (in && dd[t] < vld) ? 1u << t : 0u;
    }
    if (!act) vm = 0;
    // their match lengths, capped at good_len: the first eight bytes of all of them in one round trip, longer ones slot by slot
    uint32_t len[kHpSlots], lim[kHpSlots];
    uint64_t vb[kHpSlots];
#pragma unroll
    for (uint32_t t = 0; t < kHpSlots; t++) {
        const bool on = (vm >> t) & 1u;
        const bool fwd = t == 0 ? wpos > dd[t] : wpos >= dd[t];                 // HT2 wraps with `>` (:306)
        const uint32_t cp = fwd ? wpos - dd[t] : wpos + wsz - dd[t];
        lim[t] = on ? umin(umin(limit, wsz - cp), good) : 0u;
        dd[t] = on ? dd[t] : dd[t];
        vb[t] = 0;
        if (on) vb[t] = load8u(c.wnd + cp);
        len[t] = cp;                                                            // (kept for the continuation below)
    }
#pragma unroll
    for (uint32_t t = 0; t < kHpSlots; t++) {
        const uint32_t cp = len[t];
        const uint64_t x = va ^ vb[t];
        uint32_t nn = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
        bool go = ((vm >> t) & 1u) && nn == 8 && lim[t] > 8;
        while (go) {
            const uint64_t a8 = stage_load8(L->stage, ai + nn), b8 = load8u(c.wnd + cp + nn);
            const uint64_t y = a8 ^ b8;
            if (y) { nn += (uint32_t)__builtin_ctzll(y) >> 3; go = false; }
            else { nn += 8; go = nn < lim[t]; }
        }
        len[t] = umin(nn, lim[t]);
    }
    if (act) {
        const uint32_t slot = p & (kHpRec - 1);
#pragma unroll
        for (uint32_t t = 0; t < kHpSlots; t++) { X->r_dist[t][slot] = dd[t]; X->r_len[t][slot] = (uint8_t)len[t]; }
        X->r_vm[slot] = (uint16_t)vm;
        uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_h6, (int)h6, 0x138, 0xF, 0xF, false);   // wave_shr:1: lane i <- lane i - 1
        if (lane == 0) prev = carry_h6;
        X->r_hflag[slot] = (h6 == 0 || h6 == prev) ? 1 : 0;
    }
    carry_h6 = rdlane(h6, n - 1);
    TM_ADD(c, 1);
}

// take back the speculative inserts of positions [a, head): 64 at a time from the top; the FIRST position of a key in a batch holds
// the oldest words and restores them
DEV void hp_undo(Sc &c, HpX *X, const HpSb &sb, uint32_t a, uint32_t head)
{
    EncLds *L = c.L;
    const uint32_t lane = c.lane;
    const uint32_t W = umin(c.ht_width, c.ht_cyc);
    uint32_t hi_ = head;
    while (hi_ > a) {
        const uint32_t lo_ = hi_ - a > 64 ? hi_ - 64 : a;
        const uint32_t n = hi_ - lo_;
        const bool act = lane < n;
        const uint64_t v = stage_load8(L->stage, lo_ + lane + 16);
        const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        const uint32_t h2 = hash2_of(lo), h3 = hash3_of(lo), h6 = hash6_mul(lo, hi) >> (32 - c.ht_bits);
        bool f2 = true, f3 = true, f6 = true;
        for (uint32_t j = 0; j + 1 < n; j++) {
            const uint32_t k2 = rdlane(h2, j), k3 = rdlane(h3, j), k6 = rdlane(h6, j);
            const bool below = lane > j;
            f2 = f2 && !(below && h2 == k2);
            f3 = f3 && !(below && h3 == k3);
            f6 = f6 && !(below && h6 == k6);
        }
        if (act) {
            const uint32_t pos = sb.pos0 + lo_ + lane, slot = (lo_ + lane) & (kHpRec - 1);
            if (f2) c.ht2[h2] = pos - X->r_dist[0][slot];
            if (f3) c.ht3[h3] = pos - X->r_dist[1][slot];
            if (f6) {
                gu32 *b = c.ht6 + (size_t)h6 * c.ht_width;
#pragma unroll
                for (uint32_t t = 0; t < kHpW; t++) if (t < W) b[t] = pos - X->r_dist[2 + t][slot];
            }
        }
        wave_fence();
        hi_ = lo_;
    }
}

DEV void hp_inserter(Sc &c)
{
    HpX *X = hpx(c);
    EncLds *L = c.L;
    uint32_t seen_sb = 0, ev_done = 0;
    for (;;) {
        uint32_t s;
        while ((s = lds_vload(&X->sb_seq)) == seen_sb) {
            if (lds_vload(&X->quit) || lds_vload(&X->abort)) goto out;
            __builtin_amdgcn_s_sleep(2);
        }
        seen_sb = s;
        dp_fence();
        HpSb sb;
        sb.sb0 = lds_vload(&X->sb0); sb.pos0 = lds_vload(&X->pos0); sb.size = lds_vload(&X->size);
        c.stage_base = sb.sb0; c.stage_end = sb.sb0 + sb.size + 40;
        uint32_t head = 0, carry_h6 = 0xFFFFFFFFu;
        ev_done = lds_vload(&X->ev_seq);
        lds_vstore(&X->sb_ack, s);
        for (;;) {
            if (lds_vload(&X->abort)) goto out;
            if (lds_vload(&X->sb_seq) != seen_sb || lds_vload(&X->quit)) break;
            const uint32_t ev = lds_vload(&X->ev_seq);
            if (ev != ev_done) {
                // SlidePos(es, len) where the parser could not wave it through: a flagged position, a long match, or a range this
                // wavefront has not reached yet
                lds_fence();
                const uint32_t es = lds_vload(&X->ev_s), len = lds_vload(&X->ev_len);
                const uint32_t a = es + 1, b = es + len;
                TM_DECL;
                bool dev = len > 129;
                const uint32_t hi_ = umin(head, b);
                for (uint32_t q0 = a; q0 < hi_ && !dev; q0 += 64) {
                    const uint32_t q = q0 + c.lane;
                    dev = __ballot(q < hi_ && X->r_hflag[q & (kHpRec - 1)] != 0) != 0;
                }
                if (head <= a || dev) {
                    if (head > a) { hp_undo(c, X, sb, a, head); if (c.lane == 0) X->st_dev++; }
                    c.pos = sb.pos0 + a;
                    mf_slide_pos(c, sb.sb0 + es, len, sb.size - es);
                    head = b; carry_h6 = 0xFFFFFFFFu;
                } else if (hi_ < b) {
                    // the rest of the range: SlidePos, continuing behind the last position inserted
                    const uint64_t pv = stage_load8(L->stage, hi_ - 1 + 16);
                    const uint32_t lasth6 = UNI(hash6_mul((uint32_t)pv, (uint32_t)(pv >> 32)) >> (32 - c.ht_bits));
                    c.pos = sb.pos0 + hi_;
                    mf_slide_pos(c, sb.sb0 + es, len, sb.size - es, hi_ - es, lasth6);
                    head = b; carry_h6 = 0xFFFFFFFFu;
                }
                wave_fence();
                if (c.lane == 0) X->st_ev++;
                lds_vstore(&X->ins_head, head);
                lds_fence();
                ev_done = ev;
                lds_vstore(&X->ev_ack, ev);
                TM_ADD(c, 3);
                continue;
            }
            const uint32_t mp = lds_vload(&X->m_pos);
            if (head < sb.size && head < mp + kHpLA) {
                const uint32_t n = umin(64u, sb.size - head);
                hp_insert_batch(c, X, sb, head, n, carry_h6);
#ifdef HP_PAD_INSERTER
                hp_pad<HP_PAD_INSERTER>();
#endif
                wave_fence();
                head += n;
                lds_fence();
                lds_vstore(&X->ins_head, head);
            } else {
                __builtin_amdgcn_s_sleep(4);
            }
        }
    }
out:
#ifdef CSCMI_TIMERS
    if (c.lane == 0) for (int q = 0; q < 4; q++) atomicAdd(&c.S->stats.tm[12 + q], c.tm[q]);
#endif
    return;
}

// ------------------------------------------------------------------------------------------------------------------------------
// parser side (wavefront 0)

// mf_find_match_ht (csc_kernels_mf.inc) over the records of up to FOUR positions at once: row r (lanes 16 r .. 16 r + 15) is position
// wpos + r; slots 0-3 the rep distances, 4 HT2, 5 HT3, 7.. the bucket -- lengths and distances of the hash slots come from the
// records, the rep lengths from the sixteen-position compare.  The lazy parser looks at the next position before it codes a match
// (csc_lz.cpp:176) and searches on position by position after a literal, with the same rep distances until a match is coded: rows
// 1-3 are those searches, for the instructions of the first.  nrow = candidates per row (lane 16 r), compacted into lanes 16 r ..
DEV uint32_t hp_find_match4(Sc &c, uint32_t wpos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3, RepCache16 &rc,
                            uint32_t cnt)
{
    HpX *X = hpx(c);
    TM_DECL;
    const uint32_t p = wpos - c.stage_base;
    lds_vstore(&X->m_pos, p);
    {
        const uint32_t last = p + cnt - 1u;
        uint32_t spins = 0;
        while (lds_vload(&X->ins_head) <= last)
            if (!hp_spin(c, X, spins, 1)) return 0;
    }
    lds_fence();
    TM_ADD(c, 0);
    const uint32_t lane = c.lane, k = lane & 15, row = lane >> 4;
    const bool on = row < cnt;
    const uint32_t wp = wpos + row;
    const uint32_t slot = (p + row) & (kHpRec - 1);
    const uint32_t vld = c.vld_rge, good = c.good_len, wsz = c.wnd_size;
    const uint32_t rs = k == 4 ? 0u : k == 5 ? 1u : k >= 7 ? umin(k - 5u, kHpSlots - 1) : 0u;      // record slot of lane slot k
    const bool ishs = k == 4 || k == 5 || (k >= 7 && k - 5u < kHpSlots);
    const uint32_t vm = X->r_vm[slot];
    const uint32_t dk = X->r_dist[rs][slot];
    uint32_t Lr = X->r_len[rs][slot];
    const uint32_t rv = (k & 3u) == 0 ? rep0 : (k & 3u) == 1 ? rep1 : (k & 3u) == 2 ? rep2 : rep3;
    const bool repok = on && k < 4 && rv < vld;
    if (!(rc.valid && wpos - rc.wpos0 + cnt - 1u < 16u)) {
        rc.res = mf_rep_prefix16(c, wpos, limit, rep0, rep1, rep2, rep3);
        rc.wpos0 = wpos; rc.valid = true;
    }
    uint32_t res = (uint32_t)__shfl((int)rc.res, (int)(((wp - rc.wpos0) & 15u) * 4u + (k & 3u)));
    const bool cons_h = on && ishs && ((vm >> rs) & 1u);
    {
        // capped lengths (a rep length at the compare's cap, a record length at good_len): the real ones
        uint64_t em = __ballot((repok && res >= kRepCap16) || (cons_h && Lr >= good));
        while (__builtin_expect(em != 0, 0)) {
            const uint32_t j = (uint32_t)__builtin_ctzll(em);
            em &= em - 1;
            const uint32_t jk = j & 15u, jr = j >> 4;
            const uint32_t wpj = wpos + jr, limj = limit - jr;
            const uint32_t d = jk < 4 ? (jk == 0 ? rep0 : jk == 1 ? rep1 : jk == 2 ? rep2 : rep3) : rdlane(dk, j);
            const bool fwd = jk == 4 ? wpj > d : wpj >= d;
            const uint32_t cp = fwd ? wpj - d : wpj + wsz - d;
            const uint32_t ext = wave_prefix_from(c, wpj, cp, jk < 4 ? kRepCap16 : good, umin(limj, wsz - cp));
            if (lane == j) { if (jk < 4) res = ext; else Lr = ext; }
        }
    }
    TM_ADD(c, 1);
    const bool considered = k < 4 ? repok : cons_h;
    const uint32_t Lk = considered ? (k < 4 ? res : Lr) : 0u;
    uint32_t x = Lk;                                  // inclusive prefix max inside each row of 16 lanes
    x = max(x, dpp_row_shr<1>(0, x));
    x = max(x, dpp_row_shr<2>(0, x));
    x = max(x, dpp_row_shr<4>(0, x));
    x = max(x, dpp_row_shr<8>(0, x));
    const uint32_t premax = max(1u, dpp_row_shr<1>(0, x));
    const bool isht = k >= 4;
    const bool acc = considered && Lk > premax;
    const bool dropped = isht && Lk <= 6 && dk >= len_bound(umin(Lk, 6u));
    bool push = acc && !dropped;
    const uint32_t killm = (uint32_t)(__ballot(push && Lk >= good) >> (16u * row)) & 0xFFFFu;
    if (killm) push = push && k <= (uint32_t)__builtin_ctz(killm);
    const uint32_t pm = (uint32_t)(__ballot(push) >> (16u * row)) & 0xFFFFu;
    const uint32_t res0 = (uint32_t)__shfl((int)res, (int)(lane & 48u));              // the row's rep0 length
    const uint32_t has1 = (on && rep0 < vld && res0 >= 2) ? 1u : 0u;                  // rep0len1, :280-286
    const uint32_t n = (uint32_t)__builtin_popcount(pm) + has1;
    const uint32_t my_idx = (uint32_t)__builtin_popcount(pm & ((1u << k) - 1u)) + has1;
    const uint32_t tgt = (push ? (lane & 48u) + my_idx : 63u) * 4u;
    uint32_t clen = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)Lk);
    uint32_t cdst = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)(isht ? 4u + dk : 1u + k));
    if (has1 && k == 0) { clen = 1; cdst = 1; }
    c.cand_len_v = clen;
    c.cand_dist_v = cdst;
    TM_ADD(c, 2);
    return n;                          // per row; rows >= cnt: 0
}

// MatchFinder::FindMatch, csc_mf.cpp:497-524, for the position asked for; the candidate lists of the positions behind it stay in
// registers for the next calls (dropped when a match changes the rep distances)
struct HpNext { uint32_t wpos0, cnt, cl, cd, nrow; bool valid; };
DEV void hp_pick(uint32_t cl, uint32_t cd, uint32_t base, uint32_t n, uint32_t &out_len, uint32_t &out_dist)
{
    uint32_t bl = 1, bd = 0;
    bool have = false;
    for (uint32_t i = 1; i <= n; i++) {
        uint32_t l2 = rdlane(cl, base + i - 1), d2 = rdlane(cd, base + i - 1);
        if (!have) { bl = l2; bd = d2; have = true; continue; }
        if (second_better(bl, bd, l2, d2)) { bl = l2; bd = d2; }
    }
    out_len = bl; out_dist = bd;
}
DEV void hp_find_best(Sc &c, uint32_t wnd_pos, uint32_t limit, const uint32_t (&rep)[4], RepCache16 &rc, HpNext &nx, uint32_t &out_len, uint32_t &out_dist)
{
#ifdef HP_PAD_PARSER
    hp_pad<HP_PAD_PARSER>();
#endif
    c.st_find++;
    if (!(nx.valid && wnd_pos - nx.wpos0 < nx.cnt)) {
        nx.cnt = umin(4u, limit);
        nx.nrow = hp_find_match4(c, wnd_pos, limit, rep[0], rep[1], rep[2], rep[3], rc, nx.cnt);
        nx.cl = c.cand_len_v; nx.cd = c.cand_dist_v;
        nx.wpos0 = wnd_pos; nx.valid = true;
    }
    TM_DECL;
    const uint32_t row = wnd_pos - nx.wpos0;
    hp_pick(nx.cl, nx.cd, row * 16u, rdlane(nx.nrow, row * 16u), out_len, out_dist);
    TM_ADD(c, 11);
}

// the parser coded `len` bytes at sub-block offset s and calls SlidePos(s, len): positions s + 1 .. s + len - 1.  When the
// inserter has been through all of them and none is flagged, its inserts ARE SlidePos's: nothing to do
DEV void hp_slide(Sc &c, uint32_t s, uint32_t len)
{
    HpX *X = hpx(c);
    if (len <= 1) return;
    TM_DECL;
    c.st_slide += len - 1;
    const uint32_t a = s + 1, b = s + len;
    if (len <= 129 && lds_vload(&X->ins_head) >= b) {
        lds_fence();
        bool dev = false;
        for (uint32_t q0 = a; q0 < b; q0 += 64) {
            const uint32_t q = q0 + c.lane;
            dev = dev || __ballot(q < b && X->r_hflag[q & (kHpRec - 1)] != 0) != 0;
        }
        if (!dev) { TM_ADD(c, 7); return; }
    }
    lds_vstore(&X->ev_s, s); lds_vstore(&X->ev_len, len);
    lds_fence();
    const uint32_t ev = lds_vload(&X->ev_seq) + 1;
    lds_vstore(&X->ev_seq, ev);
    uint32_t spins = 0;
    while (lds_vload(&X->ev_ack) != ev)
        if (!hp_spin(c, X, spins, 2)) return;
    lds_fence();
    TM_ADD(c, 7);
}

DEV bool hp_ok(const Sc &c)
{
    return c.X && c.fast_ht && c.piped && !c.bt_head && c.ht_width && umin(c.ht_width, c.ht_cyc) <= kHpW && c.ht_low && c.good_len <= 255
           && c.lz_good_len == c.good_len && c.pos < 0xFFFF0000u;
}

// LZ::compress_normal (csc_lz.cpp:156-199) over the inserter's records: lz_compress_normal (csc_kernels_lz.inc) with the match
// finder taken out
DEV void lz_compress_normal_hp(Sc &c, uint32_t size, bool lazy)
{
    HpX *X = hpx(c);
    const uint32_t pos0 = c.pos, sb0 = c.wnd_curpos;
    {
        lds_vstore(&X->sb0, sb0); lds_vstore(&X->pos0, pos0); lds_vstore(&X->size, size);
        lds_vstore(&X->m_pos, 0); lds_vstore(&X->ins_head, 0);
        dp_fence();
        const uint32_t s = lds_vload(&X->sb_seq) + 1;
        lds_vstore(&X->sb_seq, s);
        uint32_t spins = 0;
        while (lds_vload(&X->sb_ack) != s)
            if (!hp_spin(c, X, spins, 3)) return;
    }
    // the rep distances live in registers while the sub-block is parsed (the coder wavefront codes from the tokens alone)
    EncLds *L = c.L;
    uint32_t rep[4] = {UNI(L->rep[0]), UNI(L->rep[1]), UNI(L->rep[2]), UNI(L->rep[3])};
    RepCache16 rc;
    rc.wpos0 = 0; rc.res = 0; rc.r0 = rc.r1 = rc.r2 = rc.r3 = 0; rc.valid = false;
    HpNext nx;
    nx.wpos0 = 0; nx.cnt = 0; nx.cl = 0; nx.cd = 0; nx.nrow = 0; nx.valid = false;
    auto out_nonlit = [&](uint32_t ulen, uint32_t udist, uint32_t ctx_after) {        // lz_out_nonlit of a piped run: LZ::encode_nonlit's bookkeeping (:127-154) + the token
        if (udist <= 4) {
            if (!(ulen == 1 && udist == 1)) {
                const uint32_t d = udist == 1 ? rep[0] : udist == 2 ? rep[1] : udist == 3 ? rep[2] : rep[3];
                rep[3] = udist > 3 ? rep[2] : rep[3];
                rep[2] = udist > 2 ? rep[1] : rep[2];
                rep[1] = udist > 1 ? rep[0] : rep[1];
                rep[0] = d;
            }
        } else { rep[3] = rep[2]; rep[2] = rep[1]; rep[1] = rep[0]; rep[0] = udist - 4; }
        rc.valid = false; nx.valid = false;                   // (the rep distances have changed)
        tok_push(c, TOK_NONLIT | (ctx_after << 8) | (ulen << 16), udist);
    };
    uint32_t u1l = 1, u1d = 0;
    bool got_u1 = false;
    uint32_t phase = 0;
    for (uint32_t i = 0; i < size && !c.error;) {
        uint32_t fl = 1, fd = 0;
        if (phase == 1 || !got_u1) hp_find_best(c, c.wnd_curpos + phase, size - i - phase, rep, rc, nx, fl, fd);
        TM_DECL;
        if (phase == 0) {
            if (!got_u1) { u1l = fl; u1d = fd; }
            if (u1l == 1 || !lazy || u1l >= c.lz_good_len) {
                if (u1d == 0) tok_push(c, TOK_LIT | (stage_byte(c, c.wnd_curpos) << 8), 0);
                else out_nonlit(u1l, u1d, stage_byte(c, c.wnd_curpos + u1l - 1));
                TM_ADD(c, 10);
                hp_slide(c, i, u1l);
                i += u1l; c.wnd_curpos += u1l;
                got_u1 = false;
            } else {
                phase = 1;
            }
            continue;
        }
        phase = 0;
        if (second_better(u1l, u1d, fl, fd)) {
            tok_push(c, TOK_LIT | (stage_byte(c, c.wnd_curpos) << 8), 0);
            TM_ADD(c, 10);
            i++; c.wnd_curpos++;                 // SlidePos(.., 1, ..) inserts nothing (:191)
            u1l = fl; u1d = fd;
            got_u1 = true;
        } else {
            out_nonlit(u1l, u1d, stage_byte(c, c.wnd_curpos + u1l - 1));
            TM_ADD(c, 10);
            hp_slide(c, i + 1, u1l - 1);
            i += u1l; c.wnd_curpos += u1l;
            got_u1 = false;
        }
    }
    // close the sub-block: every position must be in the tables before anything else looks at them
    {
        lds_vstore(&X->m_pos, size);
        uint32_t spins = 0;
        while (lds_vload(&X->ins_head) != size)
            if (!hp_spin(c, X, spins, 4)) return;
        dp_fence();
        c.pos = pos0 + size;
    }
    if (c.lane < 4) L->rep[c.lane] = c.lane == 0 ? rep[0] : c.lane == 1 ? rep[1] : c.lane == 2 ? rep[2] : rep[3];
}

DEV void hp_init(Sc &c)               // every wavefront, before the workgroup barrier of encode_stream
{
    HpX *X = hpx(c);
    if (threadIdx.x == 0) {
        X->sb_seq = 0; X->sb_ack = 0; X->quit = 0; X->abort = 0; X->m_pos = 0; X->ins_head = 0;
        X->ev_seq = 0; X->ev_ack = 0; X->st_dev = 0; X->st_ev = 0;
        X->hS[0] = (uint32_t)(uintptr_t)c.S; X->hS[1] = (uint32_t)((uint64_t)(uintptr_t)c.S >> 32);
    }
}
DEV void hp_quit(Sc &c)               // parser wavefront, at the end of the kernel
{
    HpX *X = hpx(c);
    lds_fence();
    lds_vstore(&X->quit, 1);
    if (!c.error && lds_vload(&X->abort)) c.error = lds_vload(&X->abort);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Register allocation (round 5; see the end of csc_kernels_bt.inc): each role's loop is a function of its own that builds its own
// context -- configuration from EncState, what changes from a hand-over block in LDS -- so that no scalar register is spilled
// inside the hot loops (round 4's code object: 721 spilled SGPRs in k_encode_runs_hp).
DEV void hp_ctx(Sc &c)
{
    HpX *X = &g_ldshp.x;
    const uint64_t sp = ((uint64_t)lds_vload(&X->hS[1]) << 32) | lds_vload(&X->hS[0]);
    sc_load_regs(c, (EncState *)(uintptr_t)sp, &g_ldshp.base);
    c.X = X;
    // what encode_stream<2, true, 4> fixes at compile time
    c.bt_head = nullptr; c.bt_nodes = nullptr; c.bt_bits = 0; c.bt_size = 0; c.gmb = 0; c.fast_ht = true;
    c.pair_ok = 0; c.pipe_ok = 1;
    c.st_find = c.st_slide = c.st_bt = c.st_lit = c.st_match = 0;
}
// parser: one sub-block.  In: hand[0..7] = wnd_curpos, stage_base, stage_end, pos, tok_headl, tok_tail_seen, size, lazy;
// out: hand[0], [3..5], hand[11..13] = error, counters (to be added)
__device__ __noinline__ void hp_parser_nl()
{
    Sc c;
    hp_ctx(c);
    HpX *X = &g_ldshp.x;
    c.piped = 1;
    c.wnd_curpos = lds_vload(&X->hand[0]); c.stage_base = lds_vload(&X->hand[1]); c.stage_end = lds_vload(&X->hand[2]);
    c.pos = lds_vload(&X->hand[3]); c.tok_headl = lds_vload(&X->hand[4]); c.tok_tail_seen = lds_vload(&X->hand[5]);
    const uint32_t size = lds_vload(&X->hand[6]), lazy = lds_vload(&X->hand[7]);
    c.error = 0;
    lz_compress_normal_hp(c, size, lazy != 0);
    if (c.lane == 0) {
        X->hand[0] = c.wnd_curpos; X->hand[3] = c.pos; X->hand[4] = c.tok_headl; X->hand[5] = c.tok_tail_seen;
        X->hand[11] = c.error; X->hand[12] = c.st_find; X->hand[13] = c.st_slide;
#ifdef CSCMI_TIMERS
        for (int q = 0; q < 12; q++) atomicAdd(&c.S->stats.tm[q], c.tm[q]);
#endif
    }
    lds_fence();
}
DEV void hp_parser_call(Sc &c, uint32_t size, bool lazy)
{
    HpX *X = hpx(c);
    if (c.lane == 0) {
        X->hand[0] = c.wnd_curpos; X->hand[1] = c.stage_base; X->hand[2] = c.stage_end; X->hand[3] = c.pos;
        X->hand[4] = c.tok_headl; X->hand[5] = c.tok_tail_seen; X->hand[6] = size; X->hand[7] = lazy ? 1u : 0u;
    }
    lds_fence();
    hp_parser_nl();
    c.wnd_curpos = lds_vload(&X->hand[0]); c.pos = lds_vload(&X->hand[3]); c.tok_headl = lds_vload(&X->hand[4]); c.tok_tail_seen = lds_vload(&X->hand[5]);
    const uint32_t err = lds_vload(&X->hand[11]);
    if (err && !c.error) c.error = err;
    c.st_find += lds_vload(&X->hand[12]); c.st_slide += lds_vload(&X->hand[13]);
}
__device__ __noinline__ void hp_inserter_nl() { Sc c; hp_ctx(c); hp_inserter(c); }
__device__ __noinline__ void hp_coder_nl() { Sc c; hp_ctx(c); coder_service(c); }
DEV void hp_inserter_call(Sc &) { hp_inserter_nl(); }
DEV void hp_coder_call(Sc &) { hp_coder_nl(); }
