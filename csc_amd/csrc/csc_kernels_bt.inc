// csc_kernels_bt.inc -- the binary-tree match finder (level 5: csc_mf.cpp:159-203, :368-451) as an INSERTER wavefront that runs
// ahead of the advanced parser.  Included by csc_kernels.hip inside namespace cscmi.  tests/model/bt_model.c is this arrangement on
// the CPU, proven byte-identical to the oracle (tests/test_bt_model.py).
//
// What the one-wavefront form (mf_find_match, csc_kernels_mf.inc) does in sequence -- one tree step after the other, one
// position after the other, each step a dependent load of the node pair and of the candidate's bytes -- is not sequential:
//  * the tree insert of a position does not depend on the parse.  find_match's descent (:404-451) and SlidePos's (:159-203)
//    leave the same tree; the compare cap (limit vs good_len) only changes what is reported.  The one parse dependence is the
//    long-match skip (:145): a match longer than 129 bytes is reported to the inserter, which takes back what it inserted
//    beyond the match's first byte (undo log of every word it overwrote) and replays the range with the skip rule.
//  * the trees of different hash values share no live node: 64 positions descend AT ONCE, one per lane, every step a gather
//    of 64 node pairs and 64 candidate lines (64 dependent chains in flight instead of one); positions of a batch with the
//    same hash follow each other down their tree, a step or two apart (see "pipelined chains" in bt_insert_batch).  HT2 / HT3 / tree heads are gathered once per batch, same-key positions resolved
//    from the batch itself (as the level-3 inserter does, csc_kernels_dp4.inc).
//  * the tree ring reuses the slot of position x for position x + bt_size: a descent that reaches a candidate whose slot
//    belongs to a LATER position of its own batch (distance > bt_size - 64) sees -- and modifies -- a shadow copy of that slot
//    taken before the batch stored anything.
// Per position the inserter leaves a RECORD in LDS: HT2 / HT3 / far-head distances with their match lengths capped at
// good_len, and the (length, distance) pairs of the descent steps that raised the running maximum and pass bound[].  The
// parser (wavefront 0) compares only the four rep distances itself and runs find_match's acceptance over the record in lanes
// (bt_find_match); a capped length is extended against the window on demand (it ends the DP window anyway).
// Round 5: the hash side of that acceptance does not need the parse either.  minlen only grows and a candidate is pushed iff it is
// longer than the running minlen, so "pushed under the reps' minlen m0" == "pushed under m0 = 1, and longer than m0": the inserter
// runs find_match's HT2 / HT3 / far-head / descent walk once with minlen = 1 and leaves what it pushes -- H', strictly increasing
// lengths -- as a ROW of the record; the parser's candidate list is [rep part] + the suffix of H' longer than m0 (bt_find_match:
// with no rep candidate, the row IS the list).  The general walk (bt_find_match_slow) is kept for the cases in which a capped
// length decides what follows -- a rep of good_len, or a considered HT2 / HT3 / far candidate at the cap (`amb`): then only the
// descent's terminal pair (`r_dcap`) can still count.  tests/model/bt_model.c asserts the two equal at every call (point 4 there).

constexpr uint32_t kBtRec = 256;          // record ring (positions)
constexpr uint32_t kBtLA = 160;           // the inserter starts a batch while it is less than this far ahead of the parser (round 5: 64 -> 160 -- the parser
                                          // waited ~280 cycles a node for records, mostly behind matches that carry it past the inserter's head)
constexpr uint32_t kBtMaxE = 32;          // descent steps a record can hold (bt_cyc <= 32)
constexpr uint32_t kBtRow = 37;           // a record's row: up to 3 + kBtMaxE pushed candidates; odd, so that lanes = positions fall into different banks
constexpr uint32_t kBtULog = 36;          // undo log entries per position: one store a step + two at the end
constexpr uint32_t kBtNone = 0xFFFFFFFFu;
constexpr uint32_t kBtMultiMax = 256;     // launches with at most this many streams use this form (~115 KiB of LDS a stream: one stream a CU)
constexpr uint32_t ERR_BT_STALL = 0x40300000u;
static_assert(kBtLA + 64 <= kBtRec, "a batch must not overwrite the record the parser is reading");
static_assert(kBtRec * kBtULog * 8 <= kBtUndoBytes, "the undo log must fit the region CSCEnc_Create carves for it");

typedef uint32_t __attribute__((ext_vector_type(2))) raw_vec2;
typedef GLOBAL_AS raw_vec2 gvec2;

struct BtX {
    uint32_t sb_seq, sb_ack, quit, abort;
    uint32_t sb0, pos0, btpos0, size;     // the open sub-block: window position / pos_ / bt_pos_ of its first byte, length
    uint32_t m_pos, ins_head;             // parser's position (sub-block offset); positions [0, ins_head) are in the tables and have records
    uint32_t ev_seq, ev_s, ev_len, ev_ack;   // "a match of ev_len > 129 bytes was coded at offset ev_s"
    uint32_t st_bt, st_undo;
    // parser -> post wavefront (bt_post): the nodes whose lengths are to be priced and relaxed, numbered 1, 2, ... through the kernel
    uint32_t sb_ack2, post_done, lp_int, has_post, has_coder;
    uint32_t hS[2], h_reset, hand[20];    // what the roles' own functions build their contexts from (end of this file)
    // The words of round 5's finder wavefront (request, answer, two answer slots).  Its code is gone and nothing reads them; bt_init still zeroes nine of
    // them.  Taking the words and those stores out leaves every instruction of the level-5 kernels but bt_init's as it is and only moves what lies behind
    // them in LDS -- and silesia -m5 ran 0.85 % slower in that layout, alternating with this one, three runs each, in one call (profiles/encoder_residue.md; two builds of
    // identical kernels differed by up to 0.3 % there).  So they stay until a change that measures level 5 in several calls takes them out.
    uint32_t fq_seq, fq_pos, fq_epoch, fq_sb, fq_rep[4];
    uint32_t fa_seq, sb_ack3, has_finder, f_hits, f_reqs, f_pad[3];
    struct Found { uint32_t tag[8]; uint32_t n, a0l, a0d, has1, valid, pad[3]; uint32_t cl[64], cd[64]; } found[2];
    struct Post { uint32_t seq, k, n, a0l, state, base_price, flags, pad, r[4], cl[64], cd[64]; } post[4];
    uint32_t shadow[64][2];               // the batch's own ring slots as they were before the batch
    uint32_t r_d2[kBtRec], r_d3[kBtRec], r_dfar[kBtRec], r_dhead[kBtRec];   // distances: HT2, HT3, far head (0 = none), tree head as the position saw it
    uint32_t r_l23[kBtRec], r_lfn[kBtRec];   // capped lengths HT2 | HT3 << 16; far head | entries of the row << 16 | amb << 24
    uint32_t r_un[kBtRec];                // undo log entries of the position's insert
    uint32_t r_dcap[kBtRec];              // distance of the descent's pair that reached good_len (0 = none)
    uint32_t e_dist[kBtRec][kBtRow];      // H' (see the header): the candidates find_match pushes from HT2 / HT3 / far head / descent with minlen = 1,
    uint16_t e_len[kBtRec][kBtRow];       // one row per position: the parser reads a row with neighbouring lanes
};
struct EncLdsBt { EncLds base; BtX x; CoderQ q; };
// the LDS image of a stream in this form, file-scope so that the roles' own functions (end of this file) address it directly
__shared__ EncLdsBt g_ldsbt;
static_assert(sizeof(EncLdsBt) <= kLdsPerCU, "a stream of this form has a CU's LDS to itself at the most");
struct BtSb { uint32_t sb0, pos0, btpos0, size; };

DEV BtX *btx(Sc &c) { return reinterpret_cast<BtX *>(c.X); }

DEV bool bt_spin(Sc &c, BtX *X, uint32_t &spins, uint32_t site)
{
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 1023u) == 0 && (spins > (kDpSpinLimit << 2) || lds_vload(&X->abort))) {
        if (!lds_vload(&X->abort)) lds_vstore(&X->abort, ERR_BT_STALL | (site << 16) | (spins & 0xFFFFu));
        c.error = lds_vload(&X->abort);
        return false;
    }
    return true;
}

// Per lane: min(common prefix, lim) of the staged position (stage byte index ai) and the window bytes at b, the first `start`
// bytes known equal; lt = the candidate's first differing byte is the smaller one (what the descent branches on, :194, :439).
DEV uint32_t bt_lane_prefix(const uint32_t *stage, uint32_t ai, const gu8 *b, uint32_t start, uint32_t lim, bool on, bool &lt)
{
    uint32_t n = start;
    lt = false;
    bool go = on && n < lim;
    while (go) {
        const uint64_t va = stage_load8(stage, ai + n), vb = load8u(b + n);
        const uint64_t x = va ^ vb;
        if (x) {
            const uint32_t t = (uint32_t)__builtin_ctzll(x) >> 3;
            n += t;
            lt = ((uint32_t)(vb >> (t * 8)) & 0xFFu) < ((uint32_t)(va >> (t * 8)) & 0xFFu);
            go = false;
        } else {
            n += 8;
            go = n < lim;
        }
    }
    return on ? umin(n, lim) : 0u;
}

// positions [i0, i0 + n), n <= 64, of the open sub-block: HT2 / HT3 inserts (:365-366) and the tree insert, all at once
DEV void bt_insert_batch(Sc &c, BtX *X, const BtSb &sb, uint32_t i0, uint32_t n)
{
    EncLds *L = c.L;
    const uint32_t lane = c.lane;
    const bool act = lane < n;
    const uint32_t p = i0 + lane, ai = p + 16;
    const uint64_t v = stage_load8(L->stage, ai);
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    const uint32_t h2 = hash2_of(lo), h3 = hash3_of(lo), hb = hash6_mul(lo, hi) >> (32 - c.bt_bits);
    const uint32_t pos = sb.pos0 + p, btp = sb.btpos0 + p, wpos = sb.sb0 + p, limit = sb.size - p;
    const uint32_t vld = c.vld_rge, good = c.good_len, wsz = c.wnd_size, btsz = c.bt_size;
    gu32 *nodes = c.bt_nodes;
    TM_DECL;
    // one gather, before any store of this batch
    uint32_t o2 = 0, o3 = 0, oh = 0;
    raw_vec2 own = {0u, 0u};
    if (act) { o2 = c.ht2[h2]; o3 = c.ht3[h3]; oh = c.bt_head[hb]; own = ((gvec2 *)nodes)[btp]; }
    X->shadow[lane][0] = own.x; X->shadow[lane][1] = own.y;
    // same-key positions inside the batch: the latest earlier lane of a key, and whether a later lane has it (that one stores)
    uint32_t p2 = 64, p3 = 64, pb = 64;
    bool l2 = false, l3 = false, lb = false;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t k2 = rdlane(h2, j), k3 = rdlane(h3, j), kb = rdlane(hb, j);
        const bool below = lane > j, above = lane < j;
        p2 = (below && h2 == k2) ? j : p2;
        p3 = (below && h3 == k3) ? j : p3;
        pb = (below && hb == kb) ? j : pb;
        l2 = l2 || (above && h2 == k2);
        l3 = l3 || (above && h3 == k3);
        lb = lb || (above && hb == kb);
    }
    const uint32_t d2 = pos - (p2 < 64 ? sb.pos0 + i0 + p2 : o2);
    const uint32_t d3 = pos - (p3 < 64 ? sb.pos0 + i0 + p3 : o3);
    const uint32_t dh = pos - (pb < 64 ? sb.pos0 + i0 + pb : oh);
    if (act) {
        if (!l2) c.ht2[h2] = pos;
        if (!l3) c.ht3[h3] = pos;
        if (!lb) c.bt_head[hb] = pos;
    }
    TM_ADD(c, 0);
    // HT2 / HT3 / far-head match lengths, capped at good_len
    uint32_t len2, len3, lenf, dfar = 0;
    {
        bool lt_;
        const uint32_t cp2 = wpos > d2 ? wpos - d2 : wpos + wsz - d2;          // strict, :306
        len2 = bt_lane_prefix(L->stage, ai, c.wnd + cp2, 0, umin(umin(limit, wsz - cp2), good), act && d2 < vld, lt_);
        const uint32_t cp3 = wpos >= d3 ? wpos - d3 : wpos + wsz - d3;
        len3 = bt_lane_prefix(L->stage, ai, c.wnd + cp3, 0, umin(umin(limit, wsz - cp3), good), act && d3 < vld, lt_);
        const bool far = act && dh >= btsz && dh < vld;                        // :373
        const uint32_t cpf = wpos >= dh ? wpos - dh : wpos + wsz - dh;
        lenf = bt_lane_prefix(L->stage, ai, c.wnd + cpf, 0, umin(umin(limit, wsz - cpf), good), far, lt_);
        dfar = far ? dh : 0u;
    }
    TM_ADD(c, 1);
    const uint32_t slot = p & (kBtRec - 1);
    // H', its HT2 / HT3 / far-head part (csc_mf.cpp:297-402 with minlen = 1, dist = 0, on the capped lengths); m3 = minlen when the tree is reached
    uint32_t nh = 0, m3 = 1, amb = 0, dcap = 0;
    {
        bool kill = false;
        if (act && d2 < vld) {
            amb |= len2 >= good ? 1u : 0u;
            if (len2 > m3) {
                m3 = len2;
                if (!(len2 <= 6 && d2 >= len_bound(umin(len2, 6u)))) { X->e_len[slot][nh] = (uint16_t)len2; X->e_dist[slot][nh] = d2; nh++; kill = len2 >= good; }
            }
        }
        if (act && !kill && d3 > d2 && d3 < vld) {
            amb |= len3 >= good ? 1u : 0u;
            if (len3 > m3) {
                m3 = len3;
                if (!(len3 <= 6 && d3 >= len_bound(umin(len3, 6u)))) { X->e_len[slot][nh] = (uint16_t)len3; X->e_dist[slot][nh] = d3; nh++; }
            }
        }
        if (dfar) {
            amb |= lenf >= good ? 1u : 0u;
            if (lenf > m3) {
                m3 = lenf;
                if (!(lenf <= 6 && dfar >= len_bound(umin(lenf, 6u)))) { X->e_len[slot][nh] = (uint16_t)lenf; X->e_dist[slot][nh] = dfar; nh++; }
            }
        }
    }
    // the descents: one step of every running lane per round
    uint32_t dist = dh, l = btp * 2, r = btp * 2 + 1, lold = 0, rold = 0, lenl = 0, lenr = 0, cyc = 0, runmax = 1, un = 0, steps = 0;
    uint32_t lsh = kBtNone, rsh = kBtNone;
    gvec2 *ulog = (gvec2 *)c.swapbuf + slot * kBtULog;      // (c.swapbuf of the inserter wavefront = EncState::bt_undo, bt_inserter)
    const uint32_t base = sb.btpos0 + i0;
    // PIPELINED CHAINS.  Positions of the batch with the same hash do not wait for each other to finish: a descent rewrites its
    // tree top-down and only ever stores into its two open slots (l, r) -- everything above them on its path is final, everything
    // off its path untouched -- so a later position of the tree follows right behind.  It only must not use a child slot that is
    // an open slot of an unfinished earlier position (snapshot when the round starts: the registers, before anybody moves).
    // Which child a step needs is known from the window bytes alone (both when the step ends the descent by copying the node's
    // children, :185 / :433; none when it ends with empty children).  tests/model/bt_model.c: 6.8 x fewer rounds on the silesia
    // stand-in, same bytes.
    const bool has_pred = act && pb < 64, has_succ = act && lb;
    bool running = act;
    auto put_l = [&](uint32_t val) {
        if (lsh != kBtNone) X->shadow[lsh][1] = val;
        else { raw_vec2 e; e.x = l; e.y = lold; ulog[un] = e; un++; nodes[l] = val; }
    };
    auto put_r = [&](uint32_t val) {
        if (rsh != kBtNone) X->shadow[rsh][0] = val;
        else { raw_vec2 e; e.x = r; e.y = rold; ulog[un] = e; un++; nodes[r] = val; }
    };
    for (;;) {
        const uint64_t runm = __ballot(running);
        if (!runm) break;
        const uint64_t predm = __ballot(running && has_succ);      // unfinished positions whose open slots a later lane may meet
        if (predm) wave_fence();                                    // last round's stores, for this round's loads
        if (running) {
            bool fin = false;
            const uint32_t cp = wpos >= dist ? wpos - dist : wpos + wsz - dist;
            uint32_t clen = umin(lenl, lenr);
            const uint32_t climit = umin(limit, wsz - cp);
            if (cyc >= c.bt_cyc || dist >= btsz || dist >= vld || clen >= climit) {
                put_l(0); put_r(0); fin = true;
            } else {
                const uint32_t npos = btp >= dist ? btp - dist : btp + btsz - dist;
                const uint32_t rel = npos - base;
                const bool shd = rel < n && rel > lane;
                raw_vec2 t = ((gvec2 *)nodes)[npos];
                const uint32_t climit2 = umin(good, climit);
                bool lt;
                const uint32_t full = bt_lane_prefix(L->stage, ai, c.wnd + cp, clen, climit2, true, lt);
                bool blocked = false;
                if (has_pred && predm) {
                    const bool both = full >= good;
                    const bool none = full > clen && full < good && full >= climit2;
                    const uint32_t need = lt ? npos * 2 + 1 : npos * 2;
                    for (uint64_t m = predm; m; m &= m - 1) {
                        const uint32_t jj = (uint32_t)__builtin_ctzll(m);
                        const uint32_t hl = rdlane(l, jj), hr = rdlane(r, jj);
                        const bool hit = both ? ((hl >> 1) == npos || (hr >> 1) == npos) : (hl == need || hr == need);
                        blocked = blocked || (jj < lane && hit && !none);
                    }
                }
                if (!blocked) {
                    if (shd) { t.x = X->shadow[rel][0]; t.y = X->shadow[rel][1]; }
                    steps++;
                    if (full > clen) {
                        clen = full;
                        if (clen > runmax) {
                            runmax = clen;
                            if (clen > 6 || dist < len_bound(umin(clen, 6u))) {      // :429: a pair bound[] drops is never pushed
                                if (clen > m3) { X->e_len[slot][nh] = (uint16_t)clen; X->e_dist[slot][nh] = dist; nh++; }
                                if (clen >= good) dcap = dist;                        // (the terminal pair: the descent ends here)
                            }
                        }
                        if (clen >= good) { put_l(t.x); put_r(t.y); fin = true; }
                        else if (clen >= climit2) { put_l(0); put_r(0); fin = true; }
                    }
                    if (!fin) {
                        if (lt) { put_l(pos - dist); l = npos * 2 + 1; lold = t.y; lsh = shd ? rel : kBtNone; dist = pos - t.y; lenl = clen; }
                        else { put_r(pos - dist); r = npos * 2; rold = t.x; rsh = shd ? rel : kBtNone; dist = pos - t.x; lenr = clen; }
                        cyc++;
                    }
                }
            }
            if (fin) running = false;
        }
    }
    if (act) {
        X->r_d2[slot] = d2; X->r_d3[slot] = d3; X->r_dfar[slot] = dfar; X->r_dhead[slot] = dh;
        X->r_l23[slot] = len2 | (len3 << 16); X->r_lfn[slot] = lenf | (nh << 16) | (amb << 24); X->r_un[slot] = un; X->r_dcap[slot] = dcap;
    }
    for (int o = 32; o > 0; o >>= 1) steps += (uint32_t)__shfl_xor((int)steps, o);
    c.st_bt += UNI(steps);
    TM_ADD(c, 2);
}

// take back the inserts of positions [a, head), newest first
DEV void bt_undo(Sc &c, BtX *X, const BtSb &sb, uint32_t a, uint32_t head)
{
    EncLds *L = c.L;
    for (uint32_t q = head; q-- > a;) {
        const uint32_t slot = q & (kBtRec - 1);
        const uint32_t un = UNI(X->r_un[slot]);
        const gvec2 *ulog = (const gvec2 *)c.swapbuf + slot * kBtULog;
        if (c.lane < un) { const raw_vec2 e = ulog[c.lane]; c.bt_nodes[e.x] = e.y; }     // one insert writes a word at most once
        const uint64_t v = stage_load8(L->stage, q + 16);
        const uint32_t lo = UNI((uint32_t)v), hi = UNI((uint32_t)(v >> 32));
        const uint32_t pos = sb.pos0 + q;
        if (c.lane == 0) {
            c.bt_head[hash6_mul(lo, hi) >> (32 - c.bt_bits)] = pos - X->r_dhead[slot];
            c.ht2[hash2_of(lo)] = pos - X->r_d2[slot];
            c.ht3[hash3_of(lo)] = pos - X->r_d3[slot];
        }
        wave_fence();      // the next (older) position may restore the same words: its values must land last
    }
}

DEV void bt_inserter(Sc &c)
{
    BtX *X = btx(c);
    EncLds *L = c.L;
    uint32_t seen_sb = 0, ev_done = 0;
    c.swapbuf = (gu8 *)c.S->bt_undo;      // this wavefront never filters: its scratch pointer is the undo log's own region
    for (;;) {
        uint32_t s;
        while ((s = lds_vload(&X->sb_seq)) == seen_sb) {
            if (lds_vload(&X->quit) || lds_vload(&X->abort)) goto out;
            __builtin_amdgcn_s_sleep(2);
        }
        seen_sb = s;
        dp_fence();
        BtSb sb;
        sb.sb0 = lds_vload(&X->sb0); sb.pos0 = lds_vload(&X->pos0); sb.btpos0 = lds_vload(&X->btpos0); sb.size = lds_vload(&X->size);
        c.stage_base = sb.sb0; c.stage_end = sb.sb0 + sb.size + 40;
        uint32_t head = 0;
        ev_done = lds_vload(&X->ev_seq);
        lds_vstore(&X->sb_ack, s);
        for (;;) {
            if (lds_vload(&X->abort)) goto out;
            if (lds_vload(&X->sb_seq) != seen_sb || lds_vload(&X->quit)) break;
            const uint32_t ev = lds_vload(&X->ev_seq);
            if (ev != ev_done) {
                // SlidePos(s, len) with len > 129 (:134-206): every fourth position of the first len - 129 gets HT2 / HT3 only
                lds_fence();
                const uint32_t es = lds_vload(&X->ev_s), len = lds_vload(&X->ev_len);
                const uint32_t a = es + 1;
                TM_DECL;
                if (head > a) {
                    bt_undo(c, X, sb, a, head);
                    if (c.lane == 0) X->st_undo += head - a;
                }
                const uint32_t nskip = (len - 129 + 3) / 4;           // # of i = 1 + 4k with i + 128 < len
                for (uint32_t k0 = 0; k0 < nskip; k0 += 64) {
                    const uint32_t k = k0 + c.lane;
                    if (k < nskip) {
                        const uint64_t v = stage_load8(L->stage, a + 4 * k + 16);
                        const uint32_t lo = (uint32_t)v;
                        // pos_ only grows: "the last writer of a slot wins" == max
                        __hip_atomic_fetch_max(c.ht2 + hash2_of(lo), sb.pos0 + a + 4 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_max(c.ht3 + hash3_of(lo), sb.pos0 + a + 4 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                wave_fence();
                head = a + 4 * nskip;
                lds_vstore(&X->ins_head, head);
                lds_fence();
                ev_done = ev;
                lds_vstore(&X->ev_ack, ev);
                TM_ADD(c, 3);
                continue;
            }
            const uint32_t mp = lds_vload(&X->m_pos);
            if (head < sb.size && head < mp + kBtLA) {
                const uint32_t n = umin(64u, sb.size - head);
                bt_insert_batch(c, X, sb, head, n);
                wave_fence();
                head += n;
                X->st_bt = c.st_bt;
                lds_fence();
                lds_vstore(&X->ins_head, head);
            } else {
                __builtin_amdgcn_s_sleep(4);
            }
        }
    }
out:
#ifdef CSCMI_TIMERS
    if (c.lane == 0) for (int q = 0; q < 8; q++) atomicAdd(&c.S->stats.tm[8 + q], c.tm[q]);
#endif
    return;
}

// ------------------------------------------------------------------------------------------------------------------------------
// parser side (wavefront 0)

// MatchFinder::find_match (csc_mf.cpp:243-495 with bt_head_ != 0, ht_width_ == 0) over the record of the position, the general walk:
// lanes 0-3 the rep distances (lengths in `res`), 4 HT2, 5 HT3, 6 the far head, 7 the descent's terminal pair -- the cases in which a
// capped length decides what follows (see the header); everything else goes through the row (bt_find_match below).
DEV uint32_t bt_find_match_slow(Sc &c, BtX *X, uint32_t slot, uint32_t wpos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3, uint32_t res)
{
    const uint32_t lane = c.lane, k = lane & 15;
    const uint32_t vld = c.vld_rge, good = c.good_len, wsz = c.wnd_size;
    const uint32_t d2 = UNI(X->r_d2[slot]), d3 = UNI(X->r_d3[slot]), dfar = UNI(X->r_dfar[slot]), dcap = UNI(X->r_dcap[slot]);
    const uint32_t l23 = UNI(X->r_l23[slot]), lfn = UNI(X->r_lfn[slot]);
    const uint32_t ne = dcap ? 1u : 0u;
    const uint32_t j = lane - 7;
    const uint32_t el = j < ne ? good : 0u, ed = j < ne ? dcap : 0u;
    const uint32_t rv = k == 0 ? rep0 : k == 1 ? rep1 : k == 2 ? rep2 : rep3;
    const bool repok = k < 4 && rv < vld;
    const uint32_t l2 = l23 & 0xFFFFu, l3 = l23 >> 16, lf = lfn & 0xFFFFu;
    const bool g2 = d2 < vld, g3 = d3 > d2 && d3 < vld;          // HT3 is looked at only behind HT2's distance (:334)
    // rep / HT2 / HT3: acceptance on one candidate per lane (as mf_find_match_ht); everything behind the first pushed candidate
    // that reaches good_len is not looked at (:292, :326, :357) -- the tree is (dist is reloaded from the head, :369)
    uint32_t Lk = lane < 4 ? res : lane == 4 ? l2 : lane == 5 ? l3 : lane == 6 ? lf : el;
    const uint32_t dk = lane == 4 ? d2 : lane == 5 ? d3 : lane == 6 ? dfar : ed;
    const bool cons = lane < 4 ? repok : lane == 4 ? g2 : lane == 5 ? g3 : false;
    {
        // capped lengths (HT2, HT3, far head, the descent's last pair): the real ones -- such a candidate ends the DP window
        uint64_t em = __ballot(Lk >= good && ((lane == 4 && g2) || (lane == 5 && g3) || (lane == 6 && dfar != 0) || (lane >= 7 && j < ne)));
        while (__builtin_expect(em != 0, 0)) {
            const uint32_t jj = (uint32_t)__builtin_ctzll(em);
            em &= em - 1;
            const uint32_t d = rdlane(dk, jj);
            const bool fwd = jj == 4 ? wpos > d : wpos >= d;                   // HT2 wraps with `>` (:306)
            const uint32_t cp = fwd ? wpos - d : wpos + wsz - d;
            const uint32_t ext = wave_prefix_from(c, wpos, cp, good, umin(limit, wsz - cp));
            if (lane == jj) Lk = ext;
        }
    }
    const uint32_t Lc = (lane < 6 && cons) ? Lk : 0u;
    uint32_t x = Lc;                                  // inclusive prefix max over lanes 0..15
    x = max(x, dpp_row_shr<1>(0, x));
    x = max(x, dpp_row_shr<2>(0, x));
    x = max(x, dpp_row_shr<4>(0, x));
    x = max(x, dpp_row_shr<8>(0, x));
    const uint32_t premax = max(1u, dpp_row_shr<1>(0, x));
    const bool dropped = Lk <= 6 && dk >= len_bound(umin(Lk, 6u));
    bool push = lane < 6 && cons && Lk > premax && !(lane >= 4 && dropped);
    const uint32_t killm = (uint32_t)__ballot(push && Lk >= good) & 0x3Fu;
    const uint32_t kl = killm ? (uint32_t)__builtin_ctz(killm) : 5u;
    push = push && lane <= kl;
    const uint32_t mB = max(1u, rdlane(x, kl));       // minlen when the tree is reached
    const uint32_t L6 = rdlane(Lk, 6);
    const bool acc6 = dfar != 0 && L6 > mB;
    const uint32_t mE = acc6 ? L6 : mB;
    if (lane == 6) push = acc6 && !dropped;
    if (lane >= 7) push = j < ne && Lk > mE;
    const uint64_t pm = __ballot(push);
    const uint32_t has1 = (rep0 < vld && rdlane(res, 0) >= 2) ? 1u : 0u;      // rep0len1, :280-286
    const uint32_t total = (uint32_t)__builtin_popcountll(pm) + has1;
    const uint32_t n = umin(total, kMFCandLimit - 2);                          // `if (cnt + 2 < MF_CAND_LIMIT) cnt++`
    const uint32_t my_idx = (uint32_t)__builtin_popcountll(pm & ((1ull << lane) - 1ull)) + has1;
    const uint32_t tgt = ((push && my_idx < kMFCandLimit - 2) ? my_idx : 63u) * 4u;
    uint32_t clen = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)Lk);
    uint32_t cdst = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)(lane < 4 ? 1u + lane : 4u + dk));
    if (has1 && lane == 0) { clen = 1; cdst = 1; }
    c.cand_len_v = clen;
    c.cand_dist_v = cdst;
    return n;
}

// find_match over the record of the position: the rep candidates here, the hash side from the record's row
DEV uint32_t bt_find_match(Sc &c, uint32_t wpos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3, RepCache16 &rc)
{
    BtX *X = btx(c);
    TM_DECL;
    const uint32_t p = wpos - c.stage_base;
    lds_vstore(&X->m_pos, p);
    uint32_t spins = 0;
    while (lds_vload(&X->ins_head) <= p)
        if (!bt_spin(c, X, spins, 1)) return 0;
    lds_fence();
    TM_ADD(c, 0);
    const uint32_t slot = p & (kBtRec - 1);
    const uint32_t lane = c.lane, k = lane & 15;
    const uint32_t vld = c.vld_rge, good = c.good_len, wsz = c.wnd_size;
    const uint32_t lfn = UNI(X->r_lfn[slot]);
    const uint32_t hn = (lfn >> 16) & 0xFFu, amb = lfn >> 24;
    // (no lane-dependent branch in this loop: the blocks in which its two sides meet make per-lane data of every scalar that is
    // merged there -- csc_dec_kernels.hip, DNOINL; the lanes behind the row read its last entry and drop it)
    const uint32_t rl_ = umin(lane, kBtRow - 1);
    const uint32_t el = lane < hn ? (uint32_t)X->e_len[slot][rl_] : 0u, ed = lane < hn ? X->e_dist[slot][rl_] : 0u;
    const uint32_t rv = k == 0 ? rep0 : k == 1 ? rep1 : k == 2 ? rep2 : rep3;
    const bool repok = k < 4 && rv < vld;
    // the rep lengths of sixteen positions under one set of rep distances come out of one round trip: a node reached by a literal
    // or rep0len1 edge (csc_lz.cpp:301-313) keeps its predecessor's distances and finds its lengths there
    if (!(rc.valid && wpos - rc.wpos0 < 16u && rc.r0 == rep0 && rc.r1 == rep1 && rc.r2 == rep2 && rc.r3 == rep3)) {
        rc.res = mf_rep_prefix16(c, wpos, limit, rep0, rep1, rep2, rep3);
        rc.wpos0 = wpos; rc.r0 = rep0; rc.r1 = rep1; rc.r2 = rep2; rc.r3 = rep3; rc.valid = true;
    }
    uint32_t res = (uint32_t)__shfl((int)rc.res, (int)((wpos - rc.wpos0) * 4u + (k & 3u)));
    {
        uint32_t em = (uint32_t)__ballot(lane < 4 && repok && res >= kRepCap16) & 0xFu;      // a capped rep length: the real one
        while (__builtin_expect(em != 0, 0)) {
            const uint32_t jj = (uint32_t)__builtin_ctz(em);
            em &= em - 1;
            const uint32_t d = jj == 0 ? rep0 : jj == 1 ? rep1 : jj == 2 ? rep2 : rep3;
            const uint32_t cp = wpos >= d ? wpos - d : wpos + wsz - d;
            const uint32_t ext = wave_prefix_from(c, wpos, cp, kRepCap16, umin(limit, wsz - cp));
            if ((k & 3u) == jj) res = ext;
        }
    }
    TM_ADD(c, 1);
    // the rep part (csc_mf.cpp:266-295): rep i is pushed iff it is longer than every rep before it (and than 1)
    const uint32_t Lc = (lane < 4 && repok) ? res : 0u;
    uint32_t x = Lc;
    x = max(x, dpp_row_shr<1>(0, x));
    x = max(x, dpp_row_shr<2>(0, x));                 // inclusive prefix max over lanes 0..3
    const uint32_t premax = max(1u, dpp_row_shr<1>(0, x));
    const bool acc = lane < 4 && repok && res > premax;
    const uint32_t accm = (uint32_t)__ballot(acc) & 0xFu;
    const uint32_t killm = (uint32_t)__ballot(acc && res >= good) & 0xFu;
    uint32_t n;
    if (__builtin_expect((killm | amb) != 0, 0)) {
        n = bt_find_match_slow(c, X, slot, wpos, limit, rep0, rep1, rep2, rep3, res);
        TM_ADD(c, 2);
        return n;
    }
    if (accm == 0) {
        // no rep candidate (nine positions in ten): the row is the list
        n = umin(hn, kMFCandLimit - 2);
        c.cand_len_v = el;
        c.cand_dist_v = ed + 4u;
    } else {
        const uint32_t m0 = max(1u, rdlane(x, 3));                             // minlen after the reps
        const uint32_t has1 = accm & 1u;                                       // rep0 of length >= 2: the rep0len1 entry first (:280-286)
        const uint32_t nrep = has1 + (uint32_t)__builtin_popcount(accm);
        const uint32_t keepn = (uint32_t)__builtin_popcountll(__ballot(lane < hn && el > m0));    // H' increases strictly: a suffix
        const uint32_t s = hn - keepn;
        n = umin(nrep + keepn, kMFCandLimit - 2);
        const uint32_t ridx = has1 + (uint32_t)__builtin_popcount(accm & ((1u << (lane & 3u)) - 1u));
        const uint32_t tgt = (acc ? ridx : 63u) * 4u;
        const uint32_t rl = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)res);
        const uint32_t rd = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)(1u + lane));
        const uint32_t pull = (lane - nrep + s) * 4u;
        const uint32_t hl = (uint32_t)__builtin_amdgcn_ds_bpermute((int)pull, (int)el);
        const uint32_t hd = (uint32_t)__builtin_amdgcn_ds_bpermute((int)pull, (int)ed);
        uint32_t clen = lane < nrep ? rl : hl, cdst = lane < nrep ? rd : hd + 4u;
        if (has1 && lane == 0) { clen = 1; cdst = 1; }
        c.cand_len_v = clen;
        c.cand_dist_v = cdst;
    }
    if (n) {
        // the descent's terminal pair is the one entry of a row that can stand at the cap: its real length (it ends the DP window)
        const uint32_t al = rdlane(c.cand_len_v, n - 1);
        if (__builtin_expect(al >= good, 0)) {
            const uint32_t d = rdlane(c.cand_dist_v, n - 1) - 4u;
            const uint32_t cp = wpos >= d ? wpos - d : wpos + wsz - d;
            const uint32_t ext = wave_prefix_from(c, wpos, cp, good, umin(limit, wsz - cp));
            if (lane == n - 1) c.cand_len_v = ext;
        }
    }
    TM_ADD(c, 2);
    return n;
}

DEV void bt_find_priced(Sc &c, uint32_t state, uint32_t wnd_pos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3, RepCache16 &rc,
                        uint32_t &a0_len, uint32_t &a0_dist, bool &has1, uint32_t &p1, uint32_t &lane_dist, uint32_t &lane_price, uint32_t &t_lit0)
{
    c.st_find++;
    uint32_t n = bt_find_match(c, wnd_pos, limit, rep0, rep1, rep2, rep3, rc);
    TM_DECL;
    has1 = false; p1 = 0; lane_dist = 0; lane_price = 0;
    const uint32_t t = mf_state_prices(c, state);
    t_lit0 = rdlane(t, 11);
    if (n == 0) { a0_len = 1; a0_dist = 0; TM_ADD(c, 3); return; }
    a0_len = rdlane(c.cand_len_v, n - 1); a0_dist = rdlane(c.cand_dist_v, n - 1);
    if (a0_len >= c.good_len) { TM_ADD(c, 3); return; }   // :595-596, before anything is priced
    if (rdlane(c.cand_len_v, 0) == 1 && rdlane(c.cand_dist_v, 0) == 1) { has1 = true; p1 = rdlane(t, 0) + rdlane(t, 1) + rdlane(t, 3); }
    mf_price_lengths(c, n, t, a0_len, lane_dist, lane_price);
    TM_ADD(c, 3);
}

// the parser coded a match of `len` bytes at sub-block offset s: SlidePos(s, len)
DEV void bt_slide(Sc &c, uint32_t s, uint32_t len)
{
    BtX *X = btx(c);
    if (len > 1) c.st_slide += len - 1;
    if (len <= 129) return;                    // no skip phase: the inserter's inserts ARE SlidePos's
    lds_vstore(&X->ev_s, s); lds_vstore(&X->ev_len, len);
    lds_fence();
    const uint32_t ev = lds_vload(&X->ev_seq) + 1;
    lds_vstore(&X->ev_seq, ev);
    uint32_t spins = 0;
    while (lds_vload(&X->ev_ack) != ev)
        if (!bt_spin(c, X, spins, 2)) return;
    lds_fence();
}

// the relaxation of a node's edges of length 2 .. len, one per lane (csc_lz.cpp:319-326; targets are distinct); lane_dist / lane_price
// from mf_price_lengths, cd2[wv][0..3] = the node's rep distances
DEV void bt_relax(Sc &c, uint32_t apcur, uint32_t len, uint32_t cur_state, uint32_t base_price, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3,
                  uint32_t lane_dist, uint32_t lane_price)
{
    EncLds *L = c.L;
    for (uint32_t l0 = 2; l0 <= len; l0 += 64) {
        uint32_t ll = l0 + c.lane;
        if (ll <= len) {
            uint32_t ad = l0 == 2 ? lane_dist : L->appt_dist[ll];
            uint32_t pr = l0 == 2 ? lane_price : L->appt_price[ll];
            uint32_t t = (apcur + ll) & 255u;
            if (ad && pr + base_price < L->rg_price[t]) {
                L->rg_dist[t] = ad;
                L->rg_back[t] = (uint16_t)apcur;
                L->rg_price[t] = pr + base_price;
                // rep match: move-to-front (:246-259); ordinary match: push (:261-266) -- as selects
                const bool isrep = ad <= 4;
                const uint32_t rsel0 = L->cd2[c.wv][(ad - 1) & 3u];
                const uint32_t ns = (cur_state * 4 + (isrep ? 3u : 1u)) & 0x3F;
                const uint32_t n0 = isrep ? rsel0 : ad - 4;
                const uint32_t n1 = (isrep && ad == 1) ? r1 : r0;
                const uint32_t n2 = (isrep && ad <= 2) ? r2 : r1;
                const uint32_t n3 = (isrep && ad <= 3) ? r3 : r2;
                L->rg_state[t] = (uint8_t)ns;
                L->rg_rep[t * 4 + 0] = n0; L->rg_rep[t * 4 + 1] = n1; L->rg_rep[t * 4 + 2] = n2; L->rg_rep[t * 4 + 3] = n3;
            }
        }
    }
}

// POST wavefront (wavefront 2 of k_encode_runs_bt): FindMatchWithPrice's per-length table (csc_mf.cpp:600-624) and the relaxation of
// the edges of length >= 2 (csc_lz.cpp:315-326) of the nodes the parser hands on, in node order -- GetMatchLenPrice's refresh
// countdown (csc_model.cpp:286-299) lives here while a sub-block is open.  Node k's edges land on k + 2 or later, so the parser
// is already searching node k + 1 meanwhile; it waits for this wavefront before it forms node k + 2's label and at every way out.
DEV void bt_post(Sc &c)
{
    BtX *X = btx(c);
    EncLds *L = c.L;
    uint32_t seen_sb = 0, done = 0;
    for (;;) {
        uint32_t s;
        while ((s = lds_vload(&X->sb_seq)) == seen_sb) {
            if (lds_vload(&X->quit) || lds_vload(&X->abort)) goto out;
            __builtin_amdgcn_s_sleep(2);
        }
        seen_sb = s;
        dp_fence();
        c.lp_rebuild_int = lds_vload(&X->lp_int);
        lds_vstore(&X->sb_ack2, s);
        for (;;) {
            if (lds_vload(&X->abort)) goto out;
            if (lds_vload(&X->sb_seq) != seen_sb || lds_vload(&X->quit)) break;
            BtX::Post *Q = &X->post[(done + 1) & 3u];
            if (lds_vload(&Q->seq) != done + 1) { __builtin_amdgcn_s_sleep(1); continue; }
            lds_fence();
            TM_DECL;
            const uint32_t k = UNI(Q->k), n = UNI(Q->n), a0l = UNI(Q->a0l), state = UNI(Q->state), base_price = UNI(Q->base_price), flags = UNI(Q->flags);
            const uint32_t r0 = UNI(Q->r[0]), r1 = UNI(Q->r[1]), r2 = UNI(Q->r[2]), r3 = UNI(Q->r[3]);
            c.cand_len_v = Q->cl[c.lane]; c.cand_dist_v = Q->cd[c.lane];
            L->cd2[c.wv][0] = r0; L->cd2[c.wv][1] = r1; L->cd2[c.wv][2] = r2; L->cd2[c.wv][3] = r3;
            const uint32_t t = mf_state_prices(c, state);
            uint32_t lane_dist = 0, lane_price = 0;
            mf_price_lengths(c, n, t, a0l, lane_dist, lane_price);
            TM_ADD(c, 0);
            if (!(flags & 1u)) bt_relax(c, k, a0l, state, base_price, r0, r1, r2, r3, lane_dist, lane_price);
            done++;
            lds_vstore(&X->lp_int, c.lp_rebuild_int);
            lds_fence();
            lds_vstore(&X->post_done, done);
            TM_ADD(c, 1);
        }
    }
out:
#ifdef CSCMI_TIMERS
    if (c.lane == 0) for (int q = 0; q < 2; q++) atomicAdd(&c.S->stats.tm[12 + q], c.tm[q]);
#endif
    return;
}

// may this sub-block go through the pipeline?  Not around the tree ring's wrap (bt_pos_ may stand at bt_size_ there, csc_mf.cpp:201
// vs :405) and not when pos_ is about to be renormalised: the one-wavefront form takes those
DEV bool bt_ok(const Sc &c, uint32_t size)
{
    return c.X && c.bt_head && !c.ht_width && c.ht_low && c.bt_cyc <= kBtMaxE && c.good_len <= 255 && c.good_len > 6 && c.lz_good_len == c.good_len
           && c.bt_pos + size + 8 < c.bt_size && c.pos < 0xFFFF0000u;
}

// LZ::compress_advanced (csc_lz.cpp:207-333) over the inserter's records: lz_compress_advanced (csc_kernels_lz.inc) with the
// match finder taken out
DEV void lz_compress_advanced_bt(Sc &c, uint32_t size)
{
    EncLds *L = c.L;
    BtX *X = btx(c);
    // the post wavefront takes the per-length pricing and the relaxation when the kernel has one and a node's length table fits
    // its lanes (FindMatchWithPrice beyond 64 lengths goes through the appt arrays, which alias the back-trace's)
    const bool split = lds_vload(&X->has_post) != 0 && c.good_len <= 64;
    RepCache16 rc;
    rc.wpos0 = 0; rc.res = 0; rc.r0 = rc.r1 = rc.r2 = rc.r3 = 0; rc.valid = false;
    uint32_t pseq = lds_vload(&X->post_done);
    // open the sub-block
    const uint32_t pos0 = c.pos, btpos0 = c.bt_pos;
    {
        lds_vstore(&X->lp_int, c.lp_rebuild_int);
        lds_vstore(&X->sb0, c.wnd_curpos); lds_vstore(&X->pos0, pos0); lds_vstore(&X->btpos0, btpos0); lds_vstore(&X->size, size);
        lds_vstore(&X->m_pos, 0); lds_vstore(&X->ins_head, 0);
        dp_fence();
        const uint32_t s = lds_vload(&X->sb_seq) + 1;
        lds_vstore(&X->sb_seq, s);
        uint32_t spins = 0;
        while (lds_vload(&X->sb_ack) != s || (split && lds_vload(&X->sb_ack2) != s))
            if (!bt_spin(c, X, spins, 3)) return;
    }
    for (uint32_t i = 0; i < size && !c.error;) {
        uint32_t a0l = 1, a0d = 0;
        uint32_t apcur = 0, apend = 1;
        const uint32_t aplimit = umin(kAPLimit, size - i);
        for (;;) {
            TM_DECL;
            const uint32_t sidx = c.wnd_curpos - c.stage_base + 16;
            const uint64_t v9 = stage_load8(L->stage, sidx - 1);
            const uint32_t b01 = UNI((uint32_t)v9);
            const uint32_t lit_ctx = c.wnd_curpos ? (b01 & 0xFFu) : 0u;
            const uint32_t cur_lit = (b01 >> 8) & 0xFFu;
            const uint32_t lk = c.lane & 7, lcc = cur_lit | 0x100u;
            const uint32_t plit_raw = c.p_lit[lit_ctx * 256 + (lcc >> (8 - lk))];
            const uint32_t slot = apcur & 255u;
            uint32_t cur_state, r0, r1, r2, r3, base_price;
            if (apcur) {
                cur_state = UNI(L->rg_state[slot]);
                r0 = UNI(L->rg_rep[slot * 4 + 0]); r1 = UNI(L->rg_rep[slot * 4 + 1]);
                r2 = UNI(L->rg_rep[slot * 4 + 2]); r3 = UNI(L->rg_rep[slot * 4 + 3]);
                base_price = UNI(L->rg_price[slot]);
                L->fin_dist[apcur] = UNI(L->rg_dist[slot]);
                L->fin_back[apcur] = (uint16_t)UNI(L->rg_back[slot]);
            } else {
                cur_state = c.state;
                r0 = UNI(L->rep[0]); r1 = UNI(L->rep[1]); r2 = UNI(L->rep[2]); r3 = UNI(L->rep[3]);
                base_price = 0;
                L->rg_price[0] = 0;
                L->fin_back[0] = 0;
                L->rg_rep[0] = r0; L->rg_rep[1] = r1; L->rg_rep[2] = r2; L->rg_rep[3] = r3;
            }
            L->fin_lit[apcur] = (uint8_t)cur_lit;
            bool has1 = false;
            uint32_t p1 = 0, lane_dist = 0, lane_price = 0, t_lit0 = 0;
            bool posted = false;
            if (apcur < aplimit) {
                TM_ADD(c, 4);
                if (split) {
                    // FindMatchWithPrice (:584-625) in two halves: the candidates and what the ways out / the two length-1 edges need
                    // here, the per-length prices and their relaxation on the post wavefront
                    c.st_find++;
                    const uint32_t n = bt_find_match(c, c.wnd_curpos, size - i - apcur, r0, r1, r2, r3, rc);
                    if (c.error) return;
                    TM_DECL;
                    const uint32_t t = mf_state_prices(c, cur_state);
                    t_lit0 = rdlane(t, 11);
                    if (n == 0) { a0l = 1; a0d = 0; }
                    else {
                        a0l = rdlane(c.cand_len_v, n - 1); a0d = rdlane(c.cand_dist_v, n - 1);
                        if (a0l < c.good_len) {
                            if (rdlane(c.cand_len_v, 0) == 1 && rdlane(c.cand_dist_v, 0) == 1) { has1 = true; p1 = rdlane(t, 0) + rdlane(t, 1) + rdlane(t, 3); }
                            if (a0l >= 2) {
                                BtX::Post *Q = &X->post[(pseq + 1) & 3u];
                                Q->cl[c.lane] = c.cand_len_v; Q->cd[c.lane] = c.cand_dist_v;
                                // (every lane the same words to the same places: no lane-dependent branch in the node loop)
                                Q->k = apcur; Q->n = n; Q->a0l = a0l; Q->state = cur_state; Q->base_price = base_price; Q->flags = 0;
                                Q->r[0] = r0; Q->r[1] = r1; Q->r[2] = r2; Q->r[3] = r3;
                                posted = true;          // (published below, once the ring slots it relaxes into are initialised)
                            }
                        }
                    }
                    TM_ADD(c, 3);
                } else {
                    // the relaxation below reads this node's rep distances from cd2[0..3] (as mf_find_match leaves them)
                    L->cd2[c.wv][0] = r0; L->cd2[c.wv][1] = r1; L->cd2[c.wv][2] = r2; L->cd2[c.wv][3] = r3;
                    bt_find_priced(c, cur_state, c.wnd_curpos, size - i - apcur, r0, r1, r2, r3, rc, a0l, a0d, has1, p1, lane_dist, lane_price, t_lit0);
                    if (c.error) return;
                }
                TM_RESET;
            }
            uint32_t exit_kind = 0;
            if (apcur == 0 && a0d == 0) exit_kind = 2;
            else if (apcur == aplimit) exit_kind = 1;
            else if (a0l == 1 && apcur + 1 == apend) exit_kind = 2;
            else {
                if (apcur + 1 >= apend) { L->rg_price[apend & 255u] = 0xFFFFFFFFu; apend++; }
                if (a0l >= c.lz_good_len || (a0l > 1 && a0l + apcur >= aplimit)) exit_kind = 3;
            }
            if (exit_kind) {
                if (split) {
                    // a node that leaves by a match below good_len was priced before the way out was tested (:267 precedes :290): the
                    // refresh countdown ticks, and a refresh must see the model as it is before the way out is coded
                    if (posted) { lds_fence(); X->post[(pseq + 1) & 3u].flags = 1; lds_fence(); pseq++; lds_vstore(&X->post[pseq & 3u].seq, pseq); }
                    TM_ADD(c, 5);
                    uint32_t spins = 0;
                    while (lds_vload(&X->post_done) != pseq)
                        if (!bt_spin(c, X, spins, 5)) return;
                    lds_fence();
                    TM_ADD(c, 7);
                }
                lz_ap_backward(c, apcur);
                i += apcur;
                if (exit_kind == 2) {
                    encode_literal(c, cur_lit);
                    c.wnd_curpos++;
                    i++;
                } else if (exit_kind == 3) {
                    lz_encode_nonlit(c, a0l, a0d);
                    bt_slide(c, i, a0l);
                    i += a0l;
                    c.wnd_curpos += a0l;
                    c.ctx = stage_byte(c, c.wnd_curpos - 1);
                }
                TM_ADD(c, 6);
                break;
            }
            const uint32_t len = a0l;
            // while (apcur + len >= apend) apunits_[apend++].price = 0xFFFFFFFF;  (:316-317) -- before the node is handed on
            if (apcur + len >= apend) {
                // (a loop under one count; the lanes behind the last node write its slot once more)
                for (uint32_t t0 = apend; t0 <= apcur + len; t0 += 64) L->rg_price[umin(t0 + c.lane, apcur + len) & 255u] = 0xFFFFFFFFu;
                apend = apcur + len + 1;
            }
            const uint32_t prev_seq = pseq;
            if (posted) { lds_fence(); pseq++; lds_vstore(&X->post[pseq & 3u].seq, pseq); }
            uint32_t cprice;
            {
                uint32_t bit = (lcc >> (7 - lk)) & 1;
                uint32_t pr = L->p2b[(bit ? plit_raw : 4096u - plit_raw) >> 3];
                pr += dpp_row_shr<1>(0, pr);
                pr += dpp_row_shr<2>(0, pr);
                pr += dpp_row_shr<4>(0, pr);
                cprice = rdlane(pr, 7) + t_lit0;
            }
            if (split) {
                // node apcur + 1's label so far needs the relaxations of every node before this one (strict `<`, in node order)
                TM_ADD(c, 5);
                uint32_t spins = 0;
                while ((int32_t)(lds_vload(&X->post_done) - prev_seq) < 0)
                    if (!bt_spin(c, X, spins, 6)) return;
                lds_fence();
                TM_ADD(c, 7);
            }
            const uint32_t s1slot = (apcur + 1) & 255u;
            uint32_t nprice = UNI(L->rg_price[s1slot]);
            uint32_t n_dist = 0xFFFFFFFFu;
            if (cprice + base_price < nprice) { nprice = cprice + base_price; n_dist = 0; }
            if (has1 && p1 + base_price < nprice) { nprice = p1 + base_price; n_dist = 1; }
            if (n_dist != 0xFFFFFFFFu) {
                L->rg_dist[s1slot] = n_dist;
                L->rg_back[s1slot] = (uint16_t)apcur;
                L->rg_price[s1slot] = nprice;
                L->rg_state[s1slot] = (uint8_t)((cur_state * 4 + (n_dist ? 2 : 0)) & 0x3F);
                L->rg_rep[s1slot * 4 + 0] = r0; L->rg_rep[s1slot * 4 + 1] = r1;
                L->rg_rep[s1slot * 4 + 2] = r2; L->rg_rep[s1slot * 4 + 3] = r3;
            }
            if (!split) bt_relax(c, apcur, len, cur_state, base_price, r0, r1, r2, r3, lane_dist, lane_price);
            apcur++;
            c.wnd_curpos++;
            TM_ADD(c, 5);
        }
    }
    // close the sub-block: every position must be in the tables before anything else looks at them
    {
        lds_vstore(&X->m_pos, size);
        uint32_t spins = 0;
        while (lds_vload(&X->ins_head) != size)
            if (!bt_spin(c, X, spins, 4)) return;
        dp_fence();
        c.pos = pos0 + size;
        c.bt_pos = btpos0 + size;
        if (split) c.lp_rebuild_int = lds_vload(&X->lp_int);     // (every post has been waited for at its window's way out)
    }
}

DEV void bt_init(Sc &c, uint32_t reset_arena)               // every wavefront, before the workgroup barrier of encode_stream
{
    BtX *X = btx(c);
    if (threadIdx.x == 0) {
        X->hS[0] = (uint32_t)(uintptr_t)c.S; X->hS[1] = (uint32_t)((uint64_t)(uintptr_t)c.S >> 32); X->h_reset = reset_arena;
        X->sb_seq = 0; X->sb_ack = 0; X->quit = 0; X->abort = 0; X->m_pos = 0; X->ins_head = 0;
        X->ev_seq = 0; X->ev_ack = 0; X->st_bt = 0; X->st_undo = 0;
        X->sb_ack2 = 0; X->post_done = 0; X->lp_int = 0; X->has_post = blockDim.x >= 192 ? 1u : 0u; X->has_coder = blockDim.x >= 256 ? 1u : 0u;
        X->fq_seq = 0; X->fa_seq = 0; X->sb_ack3 = 0; X->has_finder = 0; X->f_hits = 0; X->f_reqs = 0;      // (see BtX)
        X->found[0].valid = 0; X->found[1].valid = 0;
        for (int q = 0; q < 4; q++) X->post[q].seq = 0;
        CoderQ *Q = &g_ldsbt.q;
        Q->pub = 0; Q->tail = 0; Q->done = 0;
    }
}
// the parser wavefront's coded bits go to the coder wavefront (wavefront 3) when the kernel has one: what the model needs from a
// coded bit is its probability update; the carry-less range arithmetic and the byte output are a serial chain of their own
// (unconditional: both instances of the kernel are launched with four wavefronts -- a compile-time fact keeps ONE form of every coding routine in the parser's code)
DEV CoderQ *bt_coderq(Sc &c) { (void)c; return &g_ldsbt.q; }
DEV void bt_coder(Sc &c)
{
    BtX *X = btx(c);
    CoderQ *Q = &g_ldsbt.q;
    uint32_t tail = 0;
    for (;;) {
        uint32_t pub;
        while ((pub = lds_vload(&Q->pub)) == tail) {
            if (lds_vload(&X->quit)) {
                // nothing left: hand the coder's state back (CSCEncoder's coder lives across launches)
                // (every lane the same words: a lane-dependent branch in this loop would put the coder's state into vector registers)
                EncState *S = c.S;
                S->rc_low = c.rc_low; S->rc_range = c.rc_range; S->rc_cache = c.rc_cache; S->rc_cachesize = c.rc_cachesize;
                S->rc_size = c.rc_size; S->bc_size = c.bc_size; S->bc_curbits = c.bc_curbits; S->bc_curval = c.bc_curval;
                S->arena_used = c.arena_used;
                if (c.error) S->error = c.error;
                return;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        lds_acquire();
        while (tail != pub) {
            const uint32_t n = umin(pub - tail, 64u);
            const uint32_t ev = Q->e[(tail + c.lane) & (kCoderQ - 1)];
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t e = rdlane(ev, j);
                if (e & 0x80000000u) rc_code(c, (e >> 12) & 1u, e & 0xFFFu);
                else if (e & 0x40000000u) enc_direct16(c, e & 0xFFFFu, (e >> 16) & 0x1Fu);
                else coder_flush(c);
            }
            tail += n;
            lds_vstore(&Q->tail, tail);
        }
    }
}
DEV void bt_quit(Sc &c)               // parser wavefront, at the end of the kernel
{
    BtX *X = btx(c);
    if (c.Q) {
        // everything queued must be coded before the launch ends (the host reads the arena next)
        q_publish(c);
        uint32_t spins = 0;
        while (lds_vload(&c.Q->tail) != c.q_head) if (!bt_spin(c, X, spins, 7)) break;
    }
    lds_fence();
    c.st_bt += lds_vload(&X->st_bt);
    lds_vstore(&X->quit, 1);
    if (!c.error && lds_vload(&X->abort)) c.error = lds_vload(&X->abort);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Register allocation.  encode_stream is one inlined function around the 100-odd scalars of `Sc`; the compiler keeps all of them
// alive through every loop of every role and spills scalar registers INSIDE the hot loops (round 4's code objects: 1 114 spilled
// SGPRs in k_encode_runs_bt; a fifth of the parser loop's instructions were v_writelane / v_readlane).  Each role's loop therefore
// is a function of its own (__noinline__, as d5_spine of the level-3 form): it builds a context of its own -- the configuration
// from EncState, what changes from a hand-over block in LDS, every field the role does not use a compile-time constant -- so that
// inside it only what the loop uses occupies registers.  Nothing travels through private memory (a load from there counts as
// divergent: every scalar would turn into a vector register and every branch into an exec-mask branch).
DEV void bt_ctx(Sc &c)
{
    BtX *X = &g_ldsbt.x;
    const uint64_t sp = ((uint64_t)lds_vload(&X->hS[1]) << 32) | lds_vload(&X->hS[0]);
    const GLOBAL_AS EncState *G = (const GLOBAL_AS EncState *)(uintptr_t)sp;
    c.S = (EncState *)(uintptr_t)sp; c.L = &g_ldsbt.base; c.X = X; c.Q = nullptr; c.q_head = 0; c.q_room = 0;
    c.lane = threadIdx.x & 63;
    c.wnd = (gu8 *)uni_gptr(G->wnd); c.wnd_size = UNI(G->wnd_size); c.vld_rge = UNI(G->vld_rge);
    c.ht2 = (gu32 *)uni_gptr(G->ht2); c.ht3 = (gu32 *)uni_gptr(G->ht3); c.ht6 = nullptr;
    c.bt_head = (gu32 *)uni_gptr(G->bt_head); c.bt_nodes = (gu32 *)uni_gptr(G->bt_nodes);
    c.p_lit = (gu32 *)uni_gptr(G->p_lit); c.p_delta = nullptr; c.mfbuf = nullptr; c.swapbuf = (gu8 *)uni_gptr(G->bt_undo);
    c.ht6_off = 0; c.bth_off = 0; c.fast_ht = false;
    c.gm6 = c.gm2 = c.gm3 = c.gmb = 0; c.gslot = 31;
    {   // the 12-term state price gather's per-lane constants, as sc_load lays them out
        const uint32_t i = c.lane < 12 ? c.lane : 0;
        c.pr_off = (i == 0 || i == 11) ? 0u : (i <= 4 ? (i + 1) / 2 : (i - 5) / 2);
        c.pr_rmask = (i >= 5 && i <= 10) ? 0xFFFFFFFFu : 0u;
        c.pr_pol = i == 0 ? 1u : i == 11 ? 0u : ((i - 1) & 1u);
    }
    c.ht_bits = 0; c.ht_width = 0; c.ht_low = 1; c.ht_cyc = 0;
    c.bt_bits = UNI(G->bt_bits); c.bt_size = UNI(G->bt_size);
    c.lz_good_len = UNI(G->lz_good_len); c.lz_bt_cyc = UNI(G->lz_bt_cyc); c.lz_ht_cyc = 0;
    c.bt_cyc = c.lz_bt_cyc; c.good_len = c.lz_good_len;
    c.bt_pos = 0; c.pos = 0; c.wnd_curpos = 0; c.state = 0; c.ctx = 0; c.lp_rebuild_int = 0;
    c.rc_low = 0; c.rc_range = 0; c.rc_cache = 0; c.rc_cachesize = 0; c.rc_size = 0; c.bc_size = 0; c.bc_curbits = 0; c.bc_curval = 0; c.bsize = 0;
    c.rc_buf = nullptr; c.bc_buf = nullptr; c.arena = nullptr; c.arena_used = 0; c.arena_cap = 0; c.error = 0;
    c.stage_base = 0; c.stage_end = 0; c.cand_len_v = 0; c.cand_dist_v = 0;
    c.wv = 0; c.dp_seq = 0; c.dp_idle = 0; c.dp_seq_seen = 0;
    c.st_find = c.st_slide = c.st_bt = c.st_lit = c.st_match = 0;
    c.pipe_ok = 0; c.piped = 0; c.tok_headl = 0; c.tok_tail_seen = 0; c.pipe_seq = 0; c.pair_ok = 0;
#ifdef CSCMI_TIMERS
    for (int k = 0; k < 16; k++) c.tm[k] = 0;
#endif
}
// parser: one sub-block.  In: hand[0..10] = wnd_curpos, stage_base, stage_end, pos, bt_pos, state, ctx, lp_rebuild_int, q_head, q_room, size;
// out: hand[0], [3..9], hand[11..16] = error, counters (to be added)
__device__ __noinline__ void bt_parser_nl()
{
    Sc c;
    bt_ctx(c);
    BtX *X = &g_ldsbt.x;
    c.Q = &g_ldsbt.q;
    c.wnd_curpos = lds_vload(&X->hand[0]); c.stage_base = lds_vload(&X->hand[1]); c.stage_end = lds_vload(&X->hand[2]);
    c.pos = lds_vload(&X->hand[3]); c.bt_pos = lds_vload(&X->hand[4]); c.state = lds_vload(&X->hand[5]); c.ctx = lds_vload(&X->hand[6]);
    c.lp_rebuild_int = lds_vload(&X->hand[7]); c.q_head = lds_vload(&X->hand[8]); c.q_room = lds_vload(&X->hand[9]);
    const uint32_t size = lds_vload(&X->hand[10]);
    lz_compress_advanced_bt(c, size);
    if (c.lane == 0) {
        X->hand[0] = c.wnd_curpos; X->hand[3] = c.pos; X->hand[4] = c.bt_pos; X->hand[5] = c.state; X->hand[6] = c.ctx;
        X->hand[7] = c.lp_rebuild_int; X->hand[8] = c.q_head; X->hand[9] = c.q_room; X->hand[11] = c.error;
        X->hand[12] = c.st_find; X->hand[13] = c.st_slide; X->hand[14] = c.st_bt; X->hand[15] = c.st_lit; X->hand[16] = c.st_match;
#ifdef CSCMI_TIMERS
        for (int q = 0; q < 8; q++) atomicAdd(&c.S->stats.tm[q], c.tm[q]);
#endif
    }
    lds_fence();
}
DEV void bt_parser_call(Sc &c, uint32_t size)
{
    BtX *X = btx(c);
    if (c.lane == 0) {
        X->hand[0] = c.wnd_curpos; X->hand[1] = c.stage_base; X->hand[2] = c.stage_end; X->hand[3] = c.pos; X->hand[4] = c.bt_pos;
        X->hand[5] = c.state; X->hand[6] = c.ctx; X->hand[7] = c.lp_rebuild_int; X->hand[8] = c.q_head; X->hand[9] = c.q_room; X->hand[10] = size;
    }
    lds_fence();
    bt_parser_nl();
    c.wnd_curpos = lds_vload(&X->hand[0]); c.pos = lds_vload(&X->hand[3]); c.bt_pos = lds_vload(&X->hand[4]); c.state = lds_vload(&X->hand[5]);
    c.ctx = lds_vload(&X->hand[6]); c.lp_rebuild_int = lds_vload(&X->hand[7]); c.q_head = lds_vload(&X->hand[8]); c.q_room = lds_vload(&X->hand[9]);
    const uint32_t err = lds_vload(&X->hand[11]);
    if (err && !c.error) c.error = err;
    c.st_find += lds_vload(&X->hand[12]); c.st_slide += lds_vload(&X->hand[13]); c.st_bt += lds_vload(&X->hand[14]);
    c.st_lit += lds_vload(&X->hand[15]); c.st_match += lds_vload(&X->hand[16]);
}
__device__ __noinline__ void bt_inserter_nl() { Sc c; bt_ctx(c); bt_inserter(c); }
__device__ __noinline__ void bt_post_nl() { Sc c; bt_ctx(c); c.wv = 2; bt_post(c); }
__device__ __noinline__ void bt_coder_nl()
{
    Sc c;
    bt_ctx(c);
    const GLOBAL_AS EncState *G = (const GLOBAL_AS EncState *)c.S;
    // the coder's own state (Coder::Init / what the previous launch's coder wavefront left), as sc_load reads it
    c.rc_low = uni64(G->rc_low); c.rc_range = UNI(G->rc_range); c.rc_cache = UNI(G->rc_cache); c.rc_cachesize = UNI(G->rc_cachesize);
    c.rc_size = UNI(G->rc_size); c.bc_size = UNI(G->bc_size); c.bc_curbits = UNI(G->bc_curbits); c.bc_curval = UNI(G->bc_curval);
    c.bsize = UNI(G->bsize);
    c.rc_buf = (gu8 *)uni_gptr(G->rc_buf); c.bc_buf = (gu8 *)uni_gptr(G->bc_buf); c.arena = (gu8 *)uni_gptr(G->arena);
    c.arena_used = lds_vload(&g_ldsbt.x.h_reset) ? 0u : UNI(G->arena_used); c.arena_cap = UNI(G->arena_cap); c.error = UNI(G->error);
    bt_coder(c);
}
DEV void bt_inserter_call(Sc &) { bt_inserter_nl(); }
DEV void bt_post_call(Sc &) { bt_post_nl(); }
DEV void bt_coder_call(Sc &) { bt_coder_nl(); }
