// csc_kernels_mf.inc -- match finder (csc_mf.cpp) as wave-cooperative device code.
// Included by csc_kernels.hip inside namespace cscmi.

// ------------------------------------------------------------------------------------------
// hashes of csc_mf.cpp:23-42 from the 8 bytes at a window position
DEV uint32_t hash2_of(uint32_t lo) { return ((lo & 0xFFFFu) * 65521u) & 0x3FFFu; }
DEV uint32_t hash3_of(uint32_t lo) { return ((lo & 0xFFu) << 8) ^ (((lo >> 8) & 0xFFu) << 5) ^ ((lo >> 16) & 0xFFu); }
DEV uint32_t hash6_mul(uint32_t lo, uint32_t hi) { return (lo ^ ((hi & 0xFFFFu) << 13)) * 2654435761u; }

DEV uint32_t wrap_back(const Sc &c, uint32_t wpos, uint32_t dist)
{
    return wpos >= dist ? wpos - dist : wpos + c.wnd_size - dist;
}
// bound[] of csc_mf.cpp:245 = {0, 0, 64, 1 Ki, 16 Ki, 256 Ki, 4 Mi}
DEV uint32_t len_bound(uint32_t len) { return len < 2 ? 0u : (64u << (4 * (len - 2))); }

// MatchFinder::normalize, csc_mf.cpp:108-114 (reached only after ~4 G positions of one stream)
// (the table walk is a function of its own: a lane-strided loop inside the callers' serial loops would make per-lane data of their
// scalars -- csc_kernels.hip, emit_block; it runs once in 4 Gi positions)
__device__ __noinline__ void mf_normalize_lanes(gu32 *t, uint64_t n, uint32_t diff)
{
    for (uint64_t i = threadIdx.x & 63u; i < n; i += 64) { uint32_t v = t[i]; t[i] = v > diff ? v - diff : 0; }
}
DEV void mf_normalize(Sc &c)
{
    uint32_t diff = c.pos - c.vld_rge + 1;
    wave_fence();
    mf_normalize_lanes((gu32 *)c.S->mfbuf, c.S->mf_size, diff);
    wave_fence();
    c.pos -= diff;
}

// ------------------------------------------------------------------------------------------
// Extend up to 16 candidates at once.  Uniform code filled L->cmp_pos/cmp_lim (lim 0 = skip);
// candidate k is owned by lanes 4k..4k+3, each comparing 8 bytes per round (32 B / candidate /
// round).  L->cmp_res[k] = min(common prefix, lim).  Exactly the values the reference's
// sequential `while (pmatch < pend && *pcur == *pmatch)` loops produce (csc_mf.cpp:279,316,...).
DEV void batch_prefix(Sc &c, uint32_t wpos)
{
    EncLds *L = c.L;
    uint32_t k = c.lane >> 2, sub = c.lane & 3;
    uint32_t lim = L->cmp_lim[k], cp = L->cmp_pos[k];
    const gu8 *a = c.wnd + wpos, *b = c.wnd + cp;
    uint32_t res = 0, base = 0;
    bool active = lim > 0;
    while (__ballot(active)) {
        uint32_t off = base + sub * 8;
        bool stop = false;
        uint32_t here = lim;
        if (active) {
            if (off < lim) {
                uint64_t x = load8u(a + off) ^ load8u(b + off);
                uint32_t nm = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
                here = umin(off + nm, lim);
                stop = (nm < 8) || (off + 8 >= lim);
            } else {
                stop = true;
            }
        }
        uint64_t m = __ballot(active && stop);
        uint32_t grp = (uint32_t)(m >> (k * 4)) & 0xFu;
        uint32_t first = grp ? (uint32_t)__builtin_ctz(grp) : 0u;
        uint32_t v = (uint32_t)__shfl((int)here, (int)(k * 4 + first));
        if (active && grp) { res = v; active = false; }
        base += 32;
    }
    if (sub == 0) L->cmp_res[k] = res;
}

// One candidate, comparison resumed at `start` (binary-tree descent keeps min(lenl,lenr) bytes
// known equal): 8 x 8 bytes per round, replicated over the wave.  Returns min(prefix, lim) >= start.
DEV uint32_t wave_prefix_from(Sc &c, uint32_t wpos, uint32_t cp, uint32_t start, uint32_t lim)
{
    const gu8 *a = c.wnd + wpos, *b = c.wnd + cp;
    uint32_t sub = c.lane & 7;
    for (uint32_t base = start; base < lim; base += 64) {
        uint32_t off = base + sub * 8;
        bool stop = true;
        uint32_t here = lim;
        if (off < lim) {
            uint64_t x = load8u(a + off) ^ load8u(b + off);
            uint32_t nm = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
            here = umin(off + nm, lim);
            stop = (nm < 8) || (off + 8 >= lim);
        }
        uint32_t m = (uint32_t)__ballot(stop) & 0xFFu;
        if (m) return rdlane(here, (uint32_t)__builtin_ctz(m));
    }
    return lim > start ? lim : start;
}


// wave_prefix_from that also says how the first differing byte compares (candidate < current?), which is what the
// binary-tree descent branches on (csc_mf.cpp:439, :194): the byte pair is in the registers of the lane that found it, so
// the two dependent byte loads of the reference form are not needed.  `less` is meaningful when the result is < lim.
DEV uint32_t wave_prefix_cmp(Sc &c, uint32_t wpos, uint32_t cp, uint32_t start, uint32_t lim, bool &less)
{
    const gu8 *a = c.wnd + wpos, *b = c.wnd + cp;
    uint32_t sub = c.lane & 7;
    less = false;
    for (uint32_t base = start; base < lim; base += 64) {
        uint32_t off = base + sub * 8;
        bool stop = true;
        uint32_t here = lim, lt = 0;
        if (off < lim) {
            const uint64_t va = load8u(a + off), vb = load8u(b + off);
            const uint64_t x = va ^ vb;
            const uint32_t nm = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
            here = umin(off + nm, lim);
            stop = (nm < 8) || (off + 8 >= lim);
            const uint32_t sh = (nm & 7u) * 8u;
            lt = ((uint32_t)(vb >> sh) & 0xFFu) < ((uint32_t)(va >> sh) & 0xFFu) ? 1u : 0u;
        }
        uint32_t m = (uint32_t)__ballot(stop) & 0xFFu;
        if (m) {
            const uint32_t f = (uint32_t)__builtin_ctz(m);
            less = rdlane(lt, f) != 0;
            return rdlane(here, f);
        }
    }
    return lim > start ? lim : start;
}

// byte at window position wpos of the staged sub-block (uniform)
DEV uint32_t stage_byte(const Sc &c, uint32_t wpos)
{
    uint32_t idx = wpos - c.stage_base + 16;
    return UNI((c.L->stage[idx >> 2] >> ((idx & 3) * 8)) & 0xFFu);
}

// Register form of batch_prefix: lane group k (lanes 4k..4k+3) owns the candidate whose distance
// is `cdist` in those lanes (0 = none); `strict` marks the HT2 slot (csc_mf.cpp:306 wraps with `>`).
// The current-position side comes from the LDS stage, the candidate side from the window in HBM.
// Returns, in every lane of group k, min(common prefix, climit) of candidate k.
DEV uint32_t batch_prefix_reg(Sc &c, uint32_t wpos, uint32_t limit, uint32_t cdist, bool strict)
{
    uint32_t k = c.lane >> 2, sub = c.lane & 3;
    bool fwd = strict ? (wpos > cdist) : (wpos >= cdist);
    uint32_t cp = fwd ? wpos - cdist : wpos + c.wnd_size - cdist;
    uint32_t lim = cdist ? umin(limit, c.wnd_size - cp) : 0u;
    const gu8 *b = c.wnd + cp;
    const uint32_t abase = wpos - c.stage_base + 16;
    uint32_t res = 0, base = 0;
    bool active = lim > 0;
    while (__ballot(active)) {
        uint32_t off = base + sub * 8;
        bool stop = false;
        uint32_t here = lim;
        if (active) {
            if (off < lim) {
                uint64_t x = stage_load8(c.L->stage, abase + off) ^ load8u(b + off);
                uint32_t nm = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
                here = umin(off + nm, lim);
                stop = (nm < 8) || (off + 8 >= lim);
            } else {
                stop = true;
            }
        }
        uint64_t m = __ballot(active && stop);
        uint32_t grp = (uint32_t)(m >> (k * 4)) & 0xFu;
        uint32_t first = grp ? (uint32_t)__builtin_ctz(grp) : 0u;
        uint32_t v = (uint32_t)__shfl((int)here, (int)(k * 4 + first));
        if (active && grp) { res = v; active = false; }
        base += 32;
    }
    return res;
}

// row_shr:n inside each 16-lane row; lanes without a source lane get `old`
template <int N>
DEV uint32_t dpp_row_shr(uint32_t old, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x110 | N, 0xF, 0xF, false);
}

// batch_prefix_reg with slot = lane & 15, segment = lane >> 4 (so that lanes 0..15 -- one DPP row --
// end up holding one candidate each for the vector replay below)
DEV uint32_t batch_prefix16(Sc &c, uint32_t wpos, uint32_t limit, uint32_t cdist, bool strict)
{
    const uint32_t k = c.lane & 15, sub = c.lane >> 4;
    bool fwd = strict ? (wpos > cdist) : (wpos >= cdist);
    uint32_t cp = fwd ? wpos - cdist : wpos + c.wnd_size - cdist;
    uint32_t lim = cdist ? umin(limit, c.wnd_size - cp) : 0u;
    const gu8 *b = c.wnd + cp;
    const uint32_t abase = wpos - c.stage_base + 16;
    uint32_t res = 0, base = 0;
    bool active = lim > 0;
    while (__ballot(active)) {
        uint32_t off = base + sub * 8;
        bool stop = false;
        uint32_t here = lim;
        if (active) {
            if (off < lim) {
                uint64_t x = stage_load8(c.L->stage, abase + off) ^ load8u(b + off);
                uint32_t nm = x ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
                here = umin(off + nm, lim);
                stop = (nm < 8) || (off + 8 >= lim);
            } else {
                stop = true;
            }
        }
        uint64_t m = __ballot(active && stop);
        uint64_t g = (m >> k) & 0x0001000100010001ull;      // this slot's four segments
        uint32_t first = g ? ((uint32_t)__builtin_ctzll(g) >> 4) : 0u;
        uint32_t v = (uint32_t)__shfl((int)here, (int)(first * 16 + k));
        if (active && g) { res = v; active = false; }
        base += 32;
    }
    return res;
}

// find_match for the hash-table-only configurations (levels 1-4: no binary tree, bucket <= 9 wide).
// Same results as the general routine below; the difference is that the acceptance replay of
// csc_mf.cpp:266-299,301-363,453-485 is done on one candidate per lane:
//   accepted_k  <=>  considered_k and L_k > max(1, L_j of considered j < k)        (DPP prefix max)
//   pushed_k    <=>  accepted_k and not (hash candidate with L_k <= 6 and dist_k >= bound[L_k])
//   everything after the first pushed candidate with L >= good_len is ignored     (ballot + ctz)
// and the candidate list is the pushed slots compacted in slot order (ballot prefix + ds_permute).
// The three table inserts (HT2, HT3, bucket shift) are one vector store over the gather's lanes.
// what can be started before the node's rep distances are known: hashes + the entry gather
struct MfPre { uint32_t h2, h3, hv, gidx, ent; };
DEV MfPre mf_pre(Sc &c, uint32_t lo, uint32_t hi)
{
    MfPre p;
    p.h2 = hash2_of(lo); p.h3 = hash3_of(lo); p.hv = hash6_mul(lo, hi);
    uint32_t h6 = c.ht_width ? p.hv >> (32 - c.ht_bits) : 0;
    uint32_t hbt = c.bt_head ? p.hv >> (32 - c.bt_bits) : 0;
    p.gidx = (c.gm6 & (c.ht6_off + h6 * c.ht_width + c.lane)) | (c.gm2 & p.h2) | (c.gm3 & (kHT2Size + p.h3))
           | (c.gmb & (c.bth_off + hbt));
    p.ent = c.mfbuf[p.gidx];
    return p;
}

DEV uint32_t mf_find_match_ht(Sc &c, uint32_t wpos, uint32_t limit, const MfPre &pre,
                              uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3)
{
    EncLds *L = c.L;
    c.st_find++;
    TM_DECL;
    const uint32_t cands = umin(c.ht_width, c.ht_cyc);
    const uint32_t pos = c.pos, vld = c.vld_rge;
    const uint32_t gidx = pre.gidx, ent = pre.ent;
    L->cd2[c.wv][c.gslot] = pos - ent;       // slots 4 (HT2), 5 (HT3), 7.. (bucket); 0..3 are the rep distances
    L->cd2[c.wv][0] = rep0; L->cd2[c.wv][1] = rep1; L->cd2[c.wv][2] = rep2; L->cd2[c.wv][3] = rep3;
    const uint32_t d2 = pos - rdlane(ent, 32), d3 = pos - rdlane(ent, 33);
    // inserts: HT2/HT3 <- pos, bucket shifted by one with pos in front (:365-366, :487-491).  Issued as soon as the old
    // entries are in registers -- nothing below reads the tables -- so that the store has long completed when the next
    // position's gather (possibly by the other parse wavefront) is issued
    {
        const uint32_t val = c.gm6 ? dpp_row_shr<1>(pos, ent) : pos;
        if (c.gm6 | c.gm2 | c.gm3) c.mfbuf[gidx] = val;
    }
    TM_ADD(c, 0);
    // which slots are looked at: valid rep distances; hash candidates in strictly increasing distance
    uint32_t vmask = (rep0 < vld ? 1u : 0u) | (rep1 < vld ? 2u : 0u) | (rep2 < vld ? 4u : 0u) | (rep3 < vld ? 8u : 0u);
    uint32_t M = 0;
    if (d2 > M) { M = d2; if (d2 < vld) vmask |= 1u << 4; }
    if (d3 > M) { M = d3; if (d3 < vld) vmask |= 1u << 5; }
    for (uint32_t i = 0; i < cands; i++) {
        uint32_t d = pos - rdlane(ent, i);
        if (d <= M) continue;
        M = d;
        if (d < vld) vmask |= 1u << (7 + i);
    }
    const uint32_t k = c.lane & 15;
    const uint32_t dk = L->cd2[c.wv][k];
    const bool considered = c.lane < 16 && ((vmask >> k) & 1u);
    const uint32_t res = batch_prefix16(c, wpos, limit, ((vmask >> k) & 1u) ? dk : 0u, k == 4);
    TM_ADD(c, 1);

    const uint32_t Lk = considered ? res : 0u;
    uint32_t x = Lk;                                  // inclusive prefix max over lanes 0..15
    x = max(x, dpp_row_shr<1>(0, x));
    x = max(x, dpp_row_shr<2>(0, x));
    x = max(x, dpp_row_shr<4>(0, x));
    x = max(x, dpp_row_shr<8>(0, x));
    const uint32_t premax = max(1u, dpp_row_shr<1>(0, x));
    const bool isht = k >= 4;
    const bool acc = considered && Lk > premax;
    const bool dropped = isht && Lk <= 6 && dk >= len_bound(Lk);
    bool push = acc && !dropped;
    const uint32_t killm = (uint32_t)__ballot(push && Lk >= c.good_len) & 0xFFFFu;
    if (killm) push = push && k <= (uint32_t)__builtin_ctz(killm);
    const uint32_t pm = (uint32_t)__ballot(push) & 0xFFFFu;
    const uint32_t has1 = ((vmask & 1u) && rdlane(res, 0) >= 2) ? 1u : 0u;      // rep0len1, :280-286
    const uint32_t n = (uint32_t)__builtin_popcount(pm) + has1;
    const uint32_t my_idx = (uint32_t)__builtin_popcount(pm & ((1u << k) - 1u)) + has1;
    const uint32_t tgt = (push ? my_idx : 63u) * 4u;
    uint32_t clen = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)Lk);
    uint32_t cdst = (uint32_t)__builtin_amdgcn_ds_permute((int)tgt, (int)(isht ? 4u + dk : 1u + k));
    if (has1 && c.lane == 0) { clen = 1; cdst = 1; }
    c.cand_len_v = clen;
    c.cand_dist_v = cdst;

    TM_ADD(c, 2);
    if (++c.pos >= 0xFFFFFFF0u) mf_normalize(c);
    return n;
}

DEV void cand_push(Sc &c, uint32_t &cnt, uint32_t len, uint32_t dist)   // ret[cnt] = ..; csc_mf.cpp:283-286
{
    c.cand_len_v = wrlane(len, cnt, c.cand_len_v);
    c.cand_dist_v = wrlane(dist, cnt, c.cand_dist_v);
    if (cnt + 2 < kMFCandLimit) cnt++;
}

// ------------------------------------------------------------------------------------------
// MatchFinder::find_match, csc_mf.cpp:243-495.  Candidates go to L->cand_*[1..cnt].
//
// Equivalence used (SURVEY App. D): the reference probes pmatch[minlen] and then extends; a
// candidate is accepted iff its full common-prefix length L exceeds the running minlen.  So all
// L are computed first (batch_prefix), then the acceptance order, the distance guards, bound[]
// and the good_len early-out are replayed in scalar code in the reference's order.
DEV uint32_t mf_find_match(Sc &c, uint32_t wpos, uint32_t limit, const MfPre &pre,
                          uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3)
{
    if (c.fast_ht) return mf_find_match_ht(c, wpos, limit, pre, rep0, rep1, rep2, rep3);
    EncLds *L = c.L;
    c.st_find++;
    TM_DECL;
    const uint32_t h2 = pre.h2, h3 = pre.h3, hv = pre.hv;
    uint32_t h6 = c.ht_width ? hv >> (32 - c.ht_bits) : 0;
    uint32_t hbt = c.bt_head ? hv >> (32 - c.bt_bits) : 0;
    uint32_t cands = umin(c.ht_width, c.ht_cyc);
    const uint32_t pos = c.pos, vld = c.vld_rge;
    const uint32_t ent = pre.ent;
    // candidate distances: slot 4 HT2, 5 HT3, 6 BT head, 7.. HT6; 0..3 the rep distances
    L->cd2[c.wv][c.gslot] = pos - ent;
    L->cd2[c.wv][0] = rep0; L->cd2[c.wv][1] = rep1; L->cd2[c.wv][2] = rep2; L->cd2[c.wv][3] = rep3;
    const uint32_t d2 = pos - rdlane(ent, 32), d3 = pos - rdlane(ent, 33), dbt = pos - rdlane(ent, 34);
    const bool merge_ht6 = (c.bt_head == nullptr) && cands <= 9;
    TM_ADD(c, 0);

    // ---- slots: 0-3 rep, 4 HT2, 5 HT3, 6 BT far head, 7.. HT6 (when merged); vmask = slots to extend ----
    uint32_t vmask = (rep0 < vld ? 1u : 0u) | (rep1 < vld ? 2u : 0u) | (rep2 < vld ? 4u : 0u) | (rep3 < vld ? 8u : 0u);
    uint32_t M = 0;   // running max distance of the HT chain, assuming no good_len hit
    if (c.ht_low) {
        if (d2 > M) { M = d2; if (d2 < vld) vmask |= 1u << 4; }
        if (d3 > M) { M = d3; if (d3 < vld) vmask |= 1u << 5; }
    }
    if (c.bt_head && dbt >= c.bt_size && dbt < vld) vmask |= 1u << 6;
    if (merge_ht6) {
        for (uint32_t i = 0; i < cands; i++) {
            uint32_t d = pos - rdlane(ent, i);
            if (d <= M) continue;
            M = d;
            if (d < vld) vmask |= 1u << (7 + i);
        }
    }
    uint32_t res;
    {
        uint32_t k = c.lane >> 2;
        uint32_t cd = L->cd2[c.wv][k];
        cd = ((vmask >> k) & 1u) ? cd : 0u;
        res = batch_prefix_reg(c, wpos, limit, cd, k == 4);
    }
#define RES(slot) rdlane(res, (slot) * 4)
    TM_ADD(c, 1);

    // ---- replay, csc_mf.cpp:266-299 ----
    uint32_t minlen = 1, cnt = 0, dist = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (!((vmask >> i) & 1u)) continue;
        uint32_t ml = RES(i);
        if (i == 0 && ml >= 2) cand_push(c, cnt, 1, 1);          // rep0len1
        if (ml > minlen) {
            minlen = ml;
            cand_push(c, cnt, ml, 1 + (uint32_t)i);
            if (ml >= c.good_len) { dist = 0xFFFFFFFFu; break; }
        }
    }
    if (c.ht_low) {   // :301-366
        if (d2 > dist) {
            dist = d2;
            if (d2 < vld) {
                uint32_t ml = RES(4);
                if (ml > minlen) {
                    minlen = ml;
                    if (!(ml <= 6 && d2 >= len_bound(ml))) {
                        cand_push(c, cnt, ml, 4 + d2);
                        if (ml >= c.good_len) dist = 0xFFFFFFFFu;
                    }
                }
            }
        }
        if (d3 > dist) {
            dist = d3;
            if (d3 < vld) {
                uint32_t ml = RES(5);
                if (ml > minlen) {
                    minlen = ml;
                    if (!(ml <= 6 && d3 >= len_bound(ml))) {
                        cand_push(c, cnt, ml, 4 + d3);
                        if (ml >= c.good_len) dist = 0xFFFFFFFFu;
                    }
                }
            }
        }
        c.ht2[h2] = pos;
        c.ht3[h3] = pos;
    }

    if (c.bt_head) {   // :368-451
        dist = dbt;
        uint32_t l = c.bt_pos * 2, r = c.bt_pos * 2 + 1;   // indices into bt_nodes
        gu32 *nodes = c.bt_nodes;
        if (dist >= c.bt_size && dist < vld) {
            uint32_t ml = RES(6);
            if (ml > minlen) {
                minlen = ml;
                if (!(ml <= 6 && dist >= len_bound(ml))) {
                    cand_push(c, cnt, ml, 4 + dist);
                    if (ml >= c.good_len) dist = 0xFFFFFFFFu;
                }
            }
        }
        uint32_t lenl = 0, lenr = 0;
        for (uint32_t cyc = 0;; cyc++) {
            if (cyc >= c.bt_cyc || dist >= c.bt_size || dist >= vld) { nodes[l] = 0; nodes[r] = 0; break; }
            uint32_t cp = wrap_back(c, wpos, dist);
            uint32_t clen = umin(lenl, lenr);
            uint32_t climit = umin(limit, c.wnd_size - cp);
            if (clen >= climit) { nodes[l] = 0; nodes[r] = 0; break; }
            uint32_t npos = c.bt_pos >= dist ? c.bt_pos - dist : c.bt_pos + c.bt_size - dist;
            uint32_t t0 = nodes[npos * 2], t1 = nodes[npos * 2 + 1];
            bool cand_less;
            uint32_t full = wave_prefix_cmp(c, wpos, cp, clen, climit, cand_less);
            t0 = UNI(t0); t1 = UNI(t1);
            c.st_bt++;
            if (full > clen) {
                clen = full;
                if (clen > minlen) {
                    minlen = clen;
                    if (clen > 6 || dist < len_bound(clen)) cand_push(c, cnt, clen, 4 + dist);
                }
                if (clen >= c.good_len) { nodes[l] = t0; nodes[r] = t1; dist = 0xFFFFFFFFu; break; }
                else if (clen >= climit) { nodes[l] = 0; nodes[r] = 0; break; }
            }
            if (cand_less) {               // wnd[cp + clen] < wnd[wpos + clen]: clen < climit here, so that pair was compared
                nodes[l] = pos - dist;
                l = npos * 2 + 1;
                dist = pos - t1;
                lenl = clen;
            } else {
                nodes[r] = pos - dist;
                r = npos * 2;
                dist = pos - t0;
                lenr = clen;
            }
        }
        c.bt_head[hbt] = pos;
        if (++c.bt_pos >= c.bt_size) c.bt_pos -= c.bt_size;
    }

    if (cands) {   // :453-491
        if (!merge_ht6) {
            // bucket wider than the merged batch (or BT + HT6 hybrid): extend in groups of 16
            for (uint32_t g = 0; g < cands; g += 16) {
                L->cmp_lim[c.lane & 15u] = 0;          // (every lane: no lane-dependent branch)
                uint32_t dd = dist;
                uint32_t n = umin(16u, cands - g);
                for (uint32_t i = 0; i < n; i++) {
                    uint32_t d = pos - rdlane(ent, g + i);
                    if (d <= dd) continue;
                    dd = d;
                    if (d >= vld) continue;
                    uint32_t cp = wrap_back(c, wpos, d);
                    L->cmp_pos[i] = cp;
                    L->cmp_lim[i] = umin(limit, c.wnd_size - cp);
                }
                batch_prefix(c, wpos);
                bool stop = false;
                for (uint32_t i = 0; i < n; i++) {
                    uint32_t d = pos - rdlane(ent, g + i);
                    if (d <= dist) continue;
                    dist = d;
                    if (d >= vld) continue;
                    uint32_t ml = UNI(L->cmp_res[i]);
                    if (ml > minlen) {
                        minlen = ml;
                        if (ml <= 6 && d >= len_bound(ml)) continue;
                        cand_push(c, cnt, ml, 4 + d);
                        if (ml >= c.good_len) { dist = 0xFFFFFFFFu; stop = true; break; }
                    }
                }
                if (stop) break;
            }
        } else {
            for (uint32_t i = 0; i < cands; i++) {
                uint32_t d = pos - rdlane(ent, i);
                if (d <= dist) continue;
                dist = d;
                if (d >= vld) continue;
                uint32_t ml = RES(7 + i);
                if (ml > minlen) {
                    minlen = ml;
                    if (ml <= 6 && d >= len_bound(ml)) continue;
                    cand_push(c, cnt, ml, 4 + d);
                    if (ml >= c.good_len) { dist = 0xFFFFFFFFu; break; }
                }
            }
        }
        // shift the bucket and insert: one vector store (lane i <- old entry i-1, lane 0 <- pos)
        uint32_t up = (uint32_t)__shfl_up((int)ent, 1);
        // (the lanes behind the bucket store to the dump: no lane-dependent branch, csc_kernels.hip / emit_block)
        *(c.lane < cands ? c.ht6 + (size_t)h6 * c.ht_width + c.lane : (gu32 *)c.S->pf_sink + c.lane) = c.lane == 0 ? pos : up;
        // no fence: every later access to slot i of a bucket is issued by lane i again (or by all lanes)
    }
#undef RES
    TM_ADD(c, 2);
    if (++c.pos >= 0xFFFFFFF0u) mf_normalize(c);
    return cnt;
}

// ------------------------------------------------------------------------------------------
// MatchFinder::SlidePos, csc_mf.cpp:134-206: insert positions wnd_pos+1 .. wnd_pos+len-1.
// Hashes of 64 positions are computed one per lane; the table protocol (same-hash no-shift rule,
// long-match skip, tree insert) is then replayed in order.
// (start_i, lasth6_in: resume inside a call -- used by the speculative inserter of csc_kernels_dp4.inc for the part of a slid
// range it had not reached yet; only for len <= 129, where the reference has no skip phase.  c.pos = pos_ of wnd_pos + start_i.)
DEV void mf_slide_pos(Sc &c, uint32_t wnd_pos, uint32_t len, uint32_t limit, uint32_t start_i = 1, uint32_t lasth6_in = 0)
{
    if (len <= start_i) return;
    EncLds *L = c.L;
    (void)L;
    TM_DECL;
    c.st_slide += len - start_i;
    uint32_t lasth6 = lasth6_in;
    uint32_t cands = umin(c.ht_width, c.ht_cyc);
    uint32_t i = start_i;

    // long-match skip phase (:145): every 4th position gets HT2/HT3 only.  pos_ is strictly
    // increasing, so "last writer wins" == atomicMax and the inserts can go 64 at a time.
    if (len > 129 && start_i == 1 && c.pos < 0xFFFF0000u) {
        uint32_t nskip = (len - 129 + 3) / 4;   // # of i = 1 + 4k with i + 128 < len
        for (uint32_t k0 = 0; k0 < nskip; k0 += 64) {
            uint32_t k = k0 + c.lane;
            if (k < nskip) {
                uint64_t v = stage_load8(L->stage, wnd_pos + 1 + 4 * k - c.stage_base + 16);
                uint32_t lo = (uint32_t)v;
                __hip_atomic_fetch_max(c.ht2 + hash2_of(lo), c.pos + 4 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_max(c.ht3 + hash3_of(lo), c.pos + 4 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        wave_fence();
        i += 4 * nskip; c.pos += 4 * nskip; c.bt_pos += 4 * nskip;
    }

    while (i < len) {
        // hashes for up to 64 consecutive positions
        uint32_t n = umin(64u, len - i);
        uint32_t my_lo, my_hi;
        {   // (every lane loads -- the lanes behind the batch its first position -- and drops what it does not need: no lane-dependent branch)
            const uint64_t v = stage_load8(L->stage, wnd_pos + i + (c.lane < n ? c.lane : 0u) - c.stage_base + 16);
            my_lo = c.lane < n ? (uint32_t)v : 0u; my_hi = c.lane < n ? (uint32_t)(v >> 32) : 0u;
        }
        uint32_t my_h2 = hash2_of(my_lo), my_h3 = hash3_of(my_lo), my_hv = hash6_mul(my_lo, my_hi);
        uint32_t j = 0;
        // Hash-table-only configurations past the skip phase: positions whose bucket nobody else in the batch touches
        // are inserted together, one lane each -- one HBM round trip for the whole stretch instead of one per position.
        // The stretch ends in front of the first position whose bucket was already touched in this batch (or equals the
        // previous position's: the no-shift rule, :150-156); that one goes through the ordered code below.
        if (!c.bt_head && c.ht_width && cands <= 10 && i + 128 >= len && c.pos < 0xFFFF0000u) {
            const uint32_t my_h6 = my_hv >> (32 - c.ht_bits);
            bool dup = c.lane == 0 && my_h6 == lasth6;
            for (uint32_t k = 0; k + 1 < n; k++) dup = dup | ((c.lane > k) & (my_h6 == rdlane(my_h6, k)));      // (`||` / `&&` here are lane-dependent branches)
            const uint64_t dm = __ballot(dup && c.lane < n);
            const uint32_t m = dm ? (uint32_t)__builtin_ctzll(dm) : n;
            if (m) {
                {
                    // (no lane-dependent branch: the lanes behind the stretch do all of it on the dump words -- sixteen of pf_sink,
                    // the same for all of them; their values are never read)
                    const bool on = c.lane < m;
                    gu32 *const dump = (gu32 *)c.S->pf_sink;
                    // HT2/HT3: the last writer of a slot must win and pos_ only grows: max == last
                    __hip_atomic_fetch_max(on ? c.ht2 + my_h2 : dump + 16, c.pos + c.lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(on ? c.ht3 + my_h3 : dump + 17, c.pos + c.lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    gu32 *b = on ? c.ht6 + (size_t)my_h6 * c.ht_width : dump;
                    // shift by one, pos in front: all loads first (one round trip), then the stores
                    uint32_t e[9];
#pragma unroll
                    for (uint32_t t = 0; t < 9; t++) e[t] = t + 1 < cands ? b[t] : 0u;
                    b[0] = c.pos + c.lane;
#pragma unroll
                    for (uint32_t t = 0; t < 9; t++) if (t + 1 < cands) b[t + 1] = e[t];
                }
                wave_fence();
                lasth6 = rdlane(my_h6, m - 1);
                i += m; c.pos += m;
                continue;      // the next batch starts at the conflicting position (hashes are recomputed)
            }
            n = 1;             // the conflicting position itself: one ordered step, then batch again
        }
        for (; j < n; j++) {
            uint32_t wpos = wnd_pos + i;
            if (c.pos >= 0xFFFFFFF0u) mf_normalize(c);
            c.ht2[rdlane(my_h2, j)] = c.pos;
            c.ht3[rdlane(my_h3, j)] = c.pos;
            if (i + 128 < len) {   // only reachable when the vector skip phase above was bypassed
                i += 4; c.pos += 4; c.bt_pos += 4;
                break;              // hashes of the batch are stale now: recompute
            }
            uint32_t hv = rdlane(my_hv, j);
            if (c.ht_width) {
                uint32_t h6 = hv >> (32 - c.ht_bits);
                gu32 *b = c.ht6 + (size_t)h6 * c.ht_width;
                if (h6 != lasth6 && cands > 1) {
                    // (loads by every lane, the stores of the lanes outside the bucket to the dump: no lane-dependent branch)
                    const uint32_t e = b[c.lane < cands ? c.lane : 0u];
                    uint32_t up = (uint32_t)__shfl_up((int)e, 1);
                    *((c.lane >= 1 && c.lane < cands) ? b + c.lane : (gu32 *)c.S->pf_sink + c.lane) = up;
                }
                b[0] = c.pos;
                lasth6 = h6;
            }
            if (!c.bt_head) { c.pos++; i++; continue; }

            // binary-tree insert, :159-203 (compare capped at good_len)
            uint32_t hbt = hv >> (32 - c.bt_bits);
            if (c.bt_pos >= c.bt_size) c.bt_pos -= c.bt_size;
            uint32_t pos = c.pos;
            uint32_t dist = pos - UNI(c.bt_head[hbt]);
            gu32 *nodes = c.bt_nodes;
            uint32_t l = c.bt_pos * 2, r = c.bt_pos * 2 + 1, lenl = 0, lenr = 0;
            for (uint32_t cyc = 0;; cyc++) {
                if (cyc >= c.bt_cyc || dist >= c.bt_size || dist >= c.vld_rge) { nodes[l] = 0; nodes[r] = 0; break; }
                uint32_t cp = wrap_back(c, wpos, dist);
                uint32_t clen = umin(lenl, lenr);
                uint32_t climit = umin(limit - i, c.wnd_size - cp);
                if (clen >= climit) { nodes[l] = 0; nodes[r] = 0; break; }
                uint32_t npos = c.bt_pos >= dist ? c.bt_pos - dist : c.bt_pos + c.bt_size - dist;
                uint32_t t0 = nodes[npos * 2], t1 = nodes[npos * 2 + 1];
                uint32_t climit2 = umin(c.good_len, climit);
                bool cand_less;
                uint32_t full = wave_prefix_cmp(c, wpos, cp, clen, climit2, cand_less);
                t0 = UNI(t0); t1 = UNI(t1);
                c.st_bt++;
                if (full > clen) {
                    clen = full;
                    if (clen >= c.good_len) { nodes[l] = t0; nodes[r] = t1; break; }
                    else if (clen >= climit2) { nodes[l] = 0; nodes[r] = 0; break; }
                }
                if (cand_less) {           // clen < climit2: the differing byte pair was inside the compare
                    nodes[l] = pos - dist;
                    l = npos * 2 + 1;
                    dist = pos - t1;
                    lenl = clen;
                } else {
                    nodes[r] = pos - dist;
                    r = npos * 2;
                    dist = pos - t0;
                    lenr = clen;
                }
            }
            c.bt_head[hbt] = pos;
            c.bt_pos++;
            c.pos++;
            i++;
        }
    }
    TM_ADD(c, 7);
}

// MatchFinder::SlidePosFast, csc_mf.cpp:208-241 (lz_mode 5: sparse insert, no output)
DEV void mf_slide_pos_fast(Sc &c, uint32_t wnd_pos, uint32_t len)
{
    for (uint32_t i = 0; i < len;) {
        uint32_t n = umin(64u, len - i);
        uint32_t my_lo = 0, my_hi = 0;
        if (c.lane < n) {
            uint64_t v = load8u(c.wnd + wnd_pos + i + c.lane);
            my_lo = (uint32_t)v; my_hi = (uint32_t)(v >> 32);
        }
        uint32_t my_h2 = hash2_of(my_lo), my_hv = hash6_mul(my_lo, my_hi);
        for (uint32_t j = 0; j < n; j++, i++) {
            if (c.pos >= 0xFFFFFFF0u) mf_normalize(c);
            if (rdlane(my_h2, j) % 16) {
                c.pos++;
                if (++c.bt_pos >= c.bt_size) c.bt_pos -= c.bt_size;
                continue;
            }
            uint32_t hv = rdlane(my_hv, j);
            if (c.ht_width) {
                gu32 *b = c.ht6 + (size_t)(hv >> (32 - c.ht_bits)) * c.ht_width;
                uint32_t e = 0;
                if (c.lane < c.ht_width) e = b[c.lane];
                uint32_t up = (uint32_t)__shfl_up((int)e, 1);
                if (c.lane < c.ht_width) b[c.lane] = c.lane == 0 ? c.pos : up;
                wave_fence();
            }
            if (c.bt_head) {
                c.bt_nodes[c.bt_pos * 2] = 0;
                c.bt_nodes[c.bt_pos * 2 + 1] = 0;
                c.bt_head[hv >> (32 - c.bt_bits)] = c.pos;
                if (++c.bt_pos >= c.bt_size) c.bt_pos -= c.bt_size;
            }
            c.pos++;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The rep candidates of SIXTEEN positions in one round trip: lane = position offset * 4 + rep index, every lane compares its own
// candidate (up to kRepCap16 bytes).  The lazy parser searches position after position with the same four rep distances until
// it codes a match (csc_lz.cpp:156-199: 4.3 searches per match on the configs[4] mix): those searches find their rep lengths here.
constexpr uint32_t kRepCap16 = 32;
struct RepCache16 { uint32_t wpos0, res, r0, r1, r2, r3; bool valid; };
struct Rep16At { uint32_t lim, ai, sh; const gu32 *q; };
DEV Rep16At rep16_at(Sc &c, uint32_t wpos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3)
{
    Rep16At t;
    const uint32_t po = c.lane >> 2, r = c.lane & 3u;
    const uint32_t cdist = r == 0 ? rep0 : r == 1 ? rep1 : r == 2 ? rep2 : rep3;
    const uint32_t wp = wpos + po, lm = limit > po ? limit - po : 0u;
    const uint32_t cp = wp >= cdist ? wp - cdist : wp + c.wnd_size - cdist;
    t.lim = cdist < c.vld_rge ? umin(umin(lm, c.wnd_size - cp), kRepCap16) : 0u;
    t.ai = wp - c.stage_base + 16;
    // (the window has 256 bytes of slack behind it, csc_host.cpp; a lane with nothing to compare reads the window's first bytes)
    const uintptr_t a = (uintptr_t)(c.wnd + (t.lim ? cp : 0u));
    t.sh = (uint32_t)a & 3u;
    t.q = (const gu32 *)(a & ~(uintptr_t)3);
    return t;
}
DEV uint32_t mf_rep_prefix16(Sc &c, uint32_t wpos, uint32_t limit, uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3)
{
    const Rep16At t = rep16_at(c, wpos, limit, rep0, rep1, rep2, rep3);
    const uint32_t lim = t.lim, ai = t.ai;
    // At most TWO round trips (round 6): the first 8 bytes of every candidate; then, if any candidate is still equal, the other 24 bytes of all of them at
    // once (six more aligned words a lane from the window, six from the stage, three 8-byte comparisons, the first difference by selects).  The loop this
    // replaces fetched 8 bytes a turn and turned as long as ANY of the 64 candidates was still equal -- on text three or four dependent HBM / L2 round trips a
    // call (timers: 3 000 cycles a call, 44 % of the parser wavefront's time at level 2).  All 32 bytes in the first trip cost the data with few rep matches
    // more than it gave the rest (mix5 -m2: - 3.7 %); asking for the first trip where the new rep distances become known (the lazy parser's out_nonlit) cost more
    // than the overlap gave (mix5 -m2 - 3.3 %, text -m2 - 1.6 %).
    static_assert(kRepCap16 == 32, "four 8-byte comparisons");
    const uint32_t sh = t.sh, shs = ai & 3u;
    const gu32 *q = t.q;
    const uint32_t *sq = c.L->stage + (ai >> 2);
    uint32_t w[9], s[9];
#pragma unroll
    for (int k = 0; k < 3; k++) { w[k] = q[k]; s[k] = sq[k]; }
    auto diff = [&](int k, uint32_t &lo, uint32_t &hi) {
        lo = __builtin_amdgcn_alignbyte(w[2 * k + 1], w[2 * k], sh) ^ __builtin_amdgcn_alignbyte(s[2 * k + 1], s[2 * k], shs);
        hi = __builtin_amdgcn_alignbyte(w[2 * k + 2], w[2 * k + 1], sh) ^ __builtin_amdgcn_alignbyte(s[2 * k + 2], s[2 * k + 1], shs);
    };
    uint32_t lo, hi;
    diff(0, lo, hi);
    uint32_t n = lo ? (uint32_t)__builtin_ctz(lo) >> 3 : hi ? 4u + ((uint32_t)__builtin_ctz(hi) >> 3) : 8u;
    if (__ballot(n == 8u && lim > 8u)) {
#pragma unroll
        for (int k = 3; k < 9; k++) { w[k] = q[k]; s[k] = sq[k]; }
        uint32_t m = kRepCap16;
#pragma unroll
        for (int k = 3; k >= 1; k--) {
            diff(k, lo, hi);
            const uint32_t d = lo ? (uint32_t)__builtin_ctz(lo) >> 3 : 4u + ((uint32_t)__builtin_ctz(hi | 0x80000000u) >> 3);
            m = (lo | hi) ? 8u * (uint32_t)k + d : m;
        }
        n = n == 8u ? m : n;
    }
    return umin(n, lim);
}

// the lazy parser's preference predicate, csc_mf.cpp:508-516 and :570-582
DEV bool second_better(uint32_t l1, uint32_t d1, uint32_t l2, uint32_t d2)
{
    if (l2 <= 1) return false;
    if (l2 > l1 + 3) return true;
    if (l2 > l1 && d2 <= 4) return true;
    if (l2 + 2 > l1 && d2 <= 4 && d1 > 4) return true;
    if (l2 >= l1 && (d2 >> (4 * (l2 - l1))) <= d1) return true;    // cof[] = {0,4,8,12}: only reached with l2-l1 <= 3
    if (l2 < l1 && l2 + 2 >= l1 && d1 > 4 && (d1 >> (4 * (l1 - l2))) > d2) return true;
    return false;
}

// MatchFinder::FindMatch, csc_mf.cpp:497-524
DEV void mf_find_best(Sc &c, uint32_t wnd_pos, uint32_t limit, uint32_t &out_len, uint32_t &out_dist)
{
    EncLds *L = c.L;
    uint64_t cur8 = stage_load8(L->stage, wnd_pos - c.stage_base + 16);
    MfPre pre = mf_pre(c, UNI((uint32_t)cur8), UNI((uint32_t)(cur8 >> 32)));
    uint32_t n = mf_find_match(c, wnd_pos, limit, pre, UNI(L->rep[0]), UNI(L->rep[1]), UNI(L->rep[2]), UNI(L->rep[3]));
    TM_DECL;
    uint32_t bl = 1, bd = 0;
    bool have = false;
    for (uint32_t i = 1; i <= n; i++) {
        uint32_t l2 = rdlane(c.cand_len_v, i - 1), d2 = rdlane(c.cand_dist_v, i - 1);
        if (!have) { bl = l2; bd = d2; have = true; continue; }
        if (second_better(bl, bd, l2, d2)) { bl = l2; bd = d2; }
    }
    out_len = bl; out_dist = bd;
    TM_ADD(c, 11);
}

// MatchFinder::FindMatchWithPrice, csc_mf.cpp:584-625, register form.
//   a0_len/a0_dist       = appt[0], the longest candidate
//   has1/p1              = appt[1] (rep0len1) present / its price
//   lane_dist/lane_price = appt[2 + lane] for the first 64 lengths (dist 0 = no entry); lengths
//                          beyond 65 (only with custom good_len > 66) also go to L->appt_*
//   t_lit0               = price of the "literal" flag bit under `state` (for GetLiteralPrice)
// All state-dependent binary prices of this position come from ONE lane-parallel LDS gather; each
// length finds its owner candidate in its own lane; the 4097-call refresh cadence of
// GetMatchLenPrice (csc_model.cpp:286-299) is kept by numbering priced lengths with a ballot prefix.

// the 12 state-dependent bit prices: lane i -> price of (probability index, bit) as laid out in sc_load
DEV uint32_t mf_state_prices(Sc &c, uint32_t state)
{
    EncLds *L = c.L;
    const uint32_t S0 = P_STATE + state * 3;
    const uint32_t idx = S0 + c.pr_off + (c.pr_rmask & (P_REPDIST - P_STATE));
    uint32_t p = L->P[idx];
    return L->p2b[(c.pr_pol ? p : 4096u - p) >> 3];
}

// the per-length price table of a position from its n >= 1 candidates (csc_mf.cpp:600-624); t = mf_state_prices
DEV void mf_price_lengths(Sc &c, uint32_t n, uint32_t t, uint32_t maxlen, uint32_t &lane_dist, uint32_t &lane_price)
{
    EncLds *L = c.L;
    const uint32_t T0 = rdlane(t, 0), T1 = rdlane(t, 1), T2 = rdlane(t, 2), T4 = rdlane(t, 4);
    const uint32_t match_base = T0 + T2;                  // flags 1,1      (csc_model.cpp:371-372)
    const uint32_t rep_base = T0 + T1 + T4;               // flags 1,0,1    (:276-278)
    const uint32_t rp0 = rdlane(t, 5) + rdlane(t, 7), rp1 = rdlane(t, 5) + rdlane(t, 8);
    const uint32_t rp2 = rdlane(t, 6) + rdlane(t, 9), rp3 = rdlane(t, 6) + rdlane(t, 10);   // :280-282
    uint32_t calls_before = 0;
    bool rebuilt = false;
    // per-candidate prices, candidate j in lane j (csc_mf.cpp:603-613)
    const uint32_t cl = c.cand_len_v, cdv = c.cand_dist_v;
    L->rp42[c.wv][0] = rp0; L->rp42[c.wv][1] = rp1; L->rp42[c.wv][2] = rp2; L->rp42[c.wv][3] = rp3;
    const uint32_t rsel = L->rp42[c.wv][(cdv - 1) & 3u];
    const uint32_t sl = dist_slot(cdv - 5);
    const uint32_t dprice_j = cdv <= 4 ? rep_base + rsel : match_base + (sl > 2 ? sl + 2 : 2) * 128;
    for (uint32_t l0 = 2; l0 <= maxlen; l0 += 64) {
        uint32_t lp = l0 + c.lane;
        bool valid = lp <= maxlen;
        // owner = first candidate whose length reaches lp = number of candidates shorter than lp
        // (lengths increase strictly; the rep0len1 entry, length 1, is always shorter)
        uint32_t own = 0;
        for (uint32_t j = 0; j < n; j++) own += rdlane(cl, j) < lp ? 1u : 0u;
        if (!valid) own = 0;
        uint32_t odist = (uint32_t)__shfl((int)cdv, (int)own);
        uint32_t psel = (uint32_t)__shfl((int)dprice_j, (int)own);
        uint32_t rdist = odist <= 4 ? 0u : odist - 4;
        bool skip = lp <= 6 && rdist >= len_bound(lp);
        uint32_t dsel = (valid && !skip) ? odist : 0u;
        // length price with the refresh cadence
        bool priced = valid && dsel != 0;
        bool ticks = priced && (lp - 2) < 32;
        uint64_t tm = __ballot(ticks);
        uint32_t nt = (uint32_t)__builtin_popcountll(tm);
        uint32_t lenp = 128u * 6u;
        if (!rebuilt && nt && c.lp_rebuild_int >= calls_before && c.lp_rebuild_int - calls_before < nt) {
            L->len_price_old[c.lane & 31u] = L->len_price[c.lane & 31u];      // (every lane: no lane-dependent branch)
            uint32_t trigger = c.lp_rebuild_int - calls_before;   // index of the call that hits 0
            len_price_rebuild(c);                                  // sets lp_rebuild_int = 4096
            rebuilt = true;
            uint32_t my_idx = (uint32_t)__builtin_popcountll(tm & ((1ull << c.lane) - 1ull));
            if (ticks) lenp = my_idx < trigger ? L->len_price_old[lp - 2] : L->len_price[lp - 2];
            c.lp_rebuild_int = 4096 - (nt - trigger - 1);
        } else {
            if (ticks) lenp = L->len_price[lp - 2];
            if (rebuilt) c.lp_rebuild_int -= nt; else calls_before += nt;
        }
        uint32_t price = psel + lenp;
        if (l0 == 2) { lane_dist = dsel; lane_price = price; }
        if (maxlen > 65 && valid) { L->appt_dist[lp] = dsel; L->appt_price[lp] = price; }
    }
    if (!rebuilt) c.lp_rebuild_int -= calls_before;
}

DEV void mf_find_priced(Sc &c, uint32_t state, uint32_t wnd_pos, uint32_t limit, const MfPre &pre,
                        uint32_t rep0, uint32_t rep1, uint32_t rep2, uint32_t rep3, uint32_t &a0_len, uint32_t &a0_dist,
                        bool &has1, uint32_t &p1, uint32_t &lane_dist, uint32_t &lane_price, uint32_t &t_lit0)
{
    uint32_t n = mf_find_match(c, wnd_pos, limit, pre, rep0, rep1, rep2, rep3);
    TM_DECL;
    has1 = false; p1 = 0; lane_dist = 0; lane_price = 0;
    const uint32_t t = mf_state_prices(c, state);
    t_lit0 = rdlane(t, 11);
    if (n == 0) { a0_len = 1; a0_dist = 0; TM_ADD(c, 3); return; }
    a0_len = rdlane(c.cand_len_v, n - 1); a0_dist = rdlane(c.cand_dist_v, n - 1);
    if (a0_len >= c.good_len) { TM_ADD(c, 3); return; }   // :595-596, before anything is priced
    if (rdlane(c.cand_len_v, 0) == 1 && rdlane(c.cand_dist_v, 0) == 1) { has1 = true; p1 = rdlane(t, 0) + rdlane(t, 1) + rdlane(t, 3); }   // rep0len1: flags 1,0,0
    mf_price_lengths(c, n, t, a0_len, lane_dist, lane_price);
    TM_ADD(c, 3);
}
