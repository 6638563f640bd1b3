// csc_kernels_lz.inc -- LZ parsers (csc_lz.cpp): the one-wavefront forms and the token pipe (parse wavefront -> coder
// wavefront) of the lazy levels.  The many-wavefront forms of the advanced parser are csc_kernels_dp4.inc (level-3 geometry) and csc_kernels_bt.inc (binary tree).
// Included by csc_kernels.hip inside namespace cscmi.

// LZ::encode_nonlit, csc_lz.cpp:127-154 (u.dist: 1..4 = rep index+1, >= 5 = distance+4)
DEV void lz_encode_nonlit(Sc &c, uint32_t ulen, uint32_t udist)
{
    EncLds *L = c.L;
    if (udist <= 4) {
        if (ulen == 1 && udist == 1) encode_rep0len1(c);
        else {
            encode_rep_match(c, udist - 1, ulen - 2);
            uint32_t d = UNI(L->rep[udist - 1]);
            for (uint32_t k = udist - 1; k > 0; k--) L->rep[k] = UNI(L->rep[k - 1]);
            L->rep[0] = d;
        }
    } else {
        encode_match(c, udist - 5, ulen - 2);
        uint32_t r0 = UNI(L->rep[0]), r1 = UNI(L->rep[1]), r2 = UNI(L->rep[2]);
        L->rep[3] = r2; L->rep[2] = r1; L->rep[1] = r0; L->rep[0] = udist - 4;
    }
}

// ------------------------------------------------------------------------------------------
// Token pipe (lazy-parser kernels).  The greedy/lazy parse (csc_lz.cpp:156-199) never reads the model: which
// literal / match comes next depends on the match finder and the rep distances only.  So the kernels of the lazy
// levels run TWO wavefronts per stream: wavefront 0 parses and feeds (kind, length, distance, context) tokens into an
// LDS ring, wavefront 1 owns the model + range coder for the duration of an LZ pass and codes them.  The bit stream is
// the same -- the coder sees the same packets in the same order -- only the two halves of the work overlap in time.
// Hand-over of the coder-side scalars at the start and end of an LZ pass goes through L->hand[].
typedef volatile __attribute__((address_space(3))) uint32_t lds_vu32;
DEV uint32_t lds_vload(uint32_t *p) { return UNI(*(lds_vu32 *)p); }
DEV void lds_vstore(uint32_t *p, uint32_t v) { *(lds_vu32 *)p = v; }
DEV void lds_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
DEV void lds_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }

enum : uint32_t { TOK_LIT = 0, TOK_NONLIT = 1, TOK_END = 2, TOK_NONLIT_KEEPCTX = 3 };   // 3: EncodeMatch without SetLiteralCtx (the terminator)
constexpr uint32_t kPipeQuit = 0xFFFFFFFFu;

DEV void hand_put(Sc &c)
{
    EncLds *L = c.L;
    uint32_t *h = L->hand;
    h[0] = c.state; h[1] = c.ctx; h[2] = (uint32_t)c.rc_low; h[3] = (uint32_t)(c.rc_low >> 32); h[4] = c.rc_range;
    h[5] = c.rc_cache; h[6] = c.rc_cachesize; h[7] = c.rc_size; h[8] = c.bc_size; h[9] = c.bc_curbits; h[10] = c.bc_curval;
    h[11] = c.arena_used; h[12] = c.error; h[13] = c.st_lit; h[14] = c.st_match;
}
DEV void hand_get(Sc &c)
{
    uint32_t *h = c.L->hand;
    c.state = UNI(h[0]); c.ctx = UNI(h[1]); c.rc_low = ((uint64_t)UNI(h[3]) << 32) | UNI(h[2]); c.rc_range = UNI(h[4]);
    c.rc_cache = UNI(h[5]); c.rc_cachesize = UNI(h[6]); c.rc_size = UNI(h[7]); c.bc_size = UNI(h[8]); c.bc_curbits = UNI(h[9]);
    c.bc_curval = UNI(h[10]); c.arena_used = UNI(h[11]); c.error = UNI(h[12]); c.st_lit = UNI(h[13]); c.st_match = UNI(h[14]);
}

// parse side
DEV void tok_push(Sc &c, uint32_t x, uint32_t y)
{
    EncLds *L = c.L;
    while (c.tok_headl - c.tok_tail_seen >= kTokRing) {
        c.tok_tail_seen = lds_vload(&L->tok_tail);
        if (c.tok_headl - c.tok_tail_seen >= kTokRing) __builtin_amdgcn_s_sleep(8);
    }
    // token, then count: both are LDS stores of this wavefront, which the LDS of this target (gfx9 family: one in-order LDS pipeline per
    // CU, a wavefront's ds_* operations complete in issue order) carries out in order -- no wait is needed between them, only that
    // the compiler keeps the order: a release fence at WAVEFRONT scope says exactly that and emits no instruction (a workgroup-scope
    // release also waited for every global access the parser had in flight: - 2.6 %).  The consumer reads tok_head, then the token.
#if !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__) && defined(__HIP_DEVICE_COMPILE__)
#error "tok_push relies on in-order LDS: check the target before reusing it"
#endif
    typedef uint32_t __attribute__((ext_vector_type(2))) tok_vec2;      // (one 64-bit LDS store, no type punning through an integer)
    tok_vec2 tk; tk.x = x; tk.y = y;
    *(volatile __attribute__((address_space(3))) tok_vec2 *)&L->tok[c.tok_headl & (kTokRing - 1)] = tk;
    c.tok_headl++;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    lds_vstore(&L->tok_head, c.tok_headl);
}
DEV void pipe_begin(Sc &c)          // wavefront 0: the coder wavefront takes over model + range coder
{
    EncLds *L = c.L;
    hand_put(c);
    c.tok_headl = 0; c.tok_tail_seen = 0;
    lds_vstore(&L->tok_head, 0); lds_vstore(&L->tok_tail, 0);
    c.pipe_seq++;
    lds_release();
    lds_vstore(&L->pipe_cmd, c.pipe_seq);
    c.piped = 1;
}
DEV void pipe_end(Sc &c)            // wavefront 0: all tokens pushed; wait for the coder wavefront, take the scalars back
{
    EncLds *L = c.L;
    tok_push(c, TOK_END, 0);
    while (lds_vload(&L->pipe_ack) != c.pipe_seq) __builtin_amdgcn_s_sleep(8);
    lds_acquire();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // its stores to p_lit / RC / BC buffers / arena, too
    hand_get(c);
    c.piped = 0;
}

// LZ::encode_nonlit's rep-distance bookkeeping (csc_lz.cpp:127-154), parse side of a piped run
DEV void lz_rep_update(Sc &c, uint32_t ulen, uint32_t udist)
{
    EncLds *L = c.L;
    if (udist <= 4) {
        if (!(ulen == 1 && udist == 1)) {
            uint32_t d = UNI(L->rep[udist - 1]);
            for (uint32_t k = udist - 1; k > 0; k--) L->rep[k] = UNI(L->rep[k - 1]);
            L->rep[0] = d;
        }
    } else {
        uint32_t r0 = UNI(L->rep[0]), r1 = UNI(L->rep[1]), r2 = UNI(L->rep[2]);
        L->rep[3] = r2; L->rep[2] = r1; L->rep[1] = r0; L->rep[0] = udist - 4;
    }
}
// the two things the lazy parser emits: directly, or as tokens for the coder wavefront
DEV void lz_out_literal(Sc &c, uint32_t byte)
{
    if (c.piped) tok_push(c, TOK_LIT | (byte << 8), 0);
    else encode_literal(c, byte);
}
DEV void lz_out_nonlit(Sc &c, uint32_t ulen, uint32_t udist, uint32_t ctx_after)
{
    if (c.piped) { lz_rep_update(c, ulen, udist); tok_push(c, TOK_NONLIT | (ctx_after << 8) | (ulen << 16), udist); }
    else { lz_encode_nonlit(c, ulen, udist); c.ctx = ctx_after; }
}

// coder side: wavefront 1 of a lazy-parser kernel
DEV void coder_service(Sc &c)
{
    EncLds *L = c.L;
    uint32_t seen = 0;
    for (;;) {
        uint32_t cmd;
        while ((cmd = lds_vload(&L->pipe_cmd)) == seen) __builtin_amdgcn_s_sleep(16);
        if (cmd == kPipeQuit) return;
        seen = cmd;
        lds_acquire();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        hand_get(c);
        uint32_t tail = 0;
        bool end = false;
        // (round 6, measured and not kept: the NEXT literal's p_lit gather issued a token ahead -- its context is known from this token -- with the common
        // nodes of the two walks forwarded in registers: bit-exact, mix5 -m2 2.61 -> 2.35 MB/s.  The wait in front of the first use is s_waitcnt vmcnt(0),
        // which on this target also waits for the acknowledgement of the coder's own latest byte store: the round trip moves, it does not go away.)
        while (!end) {
            uint32_t h;
            while ((h = lds_vload(&L->tok_head)) == tail) __builtin_amdgcn_s_sleep(4);
            lds_acquire();
            for (; tail != h && !end; tail++) {
                uint2 t = L->tok[tail & (kTokRing - 1)];
                const uint32_t x = UNI(t.x), y = UNI(t.y), kind = x & 3u;
#ifdef HP_PAD_CODER
                for (int q = 0; q < HP_PAD_CODER / 16; q++) asm volatile("s_nop 15");
#endif
                if (kind == TOK_LIT) encode_literal(c, (x >> 8) & 0xFFu);
                else if (kind == TOK_NONLIT || kind == TOK_NONLIT_KEEPCTX) {
                    const uint32_t ulen = x >> 16, udist = y;
                    if (udist <= 4) {
                        if (ulen == 1 && udist == 1) encode_rep0len1(c);
                        else encode_rep_match(c, udist - 1, ulen - 2);
                    } else encode_match(c, udist - 5, ulen - 2);
                    if (kind == TOK_NONLIT) c.ctx = (x >> 8) & 0xFFu;
                } else end = true;
            }
            lds_vstore(&L->tok_tail, tail);
        }
        hand_put(c);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        lds_release();
        lds_vstore(&L->pipe_ack, seen);
    }
}

// LZ::compress_normal, csc_lz.cpp:156-199 (lz_mode 1 = greedy, 2 = lazy).  Written as a
// two-phase loop (phase 0 looks at the current position, phase 1 at the next one) so that
// FindMatch has a single call site.
DEV void lz_compress_normal(Sc &c, uint32_t size, bool lazy)
{
    uint32_t u1l = 1, u1d = 0;
    bool got_u1 = false;
    uint32_t phase = 0;
    for (uint32_t i = 0; i < size;) {
        uint32_t fl = 1, fd = 0;
        if (phase == 1 || !got_u1) mf_find_best(c, c.wnd_curpos + phase, size - i - phase, fl, fd);
        TM_DECL;
        if (phase == 0) {
            if (!got_u1) { u1l = fl; u1d = fd; }
            if (u1l == 1 || !lazy || u1l >= c.lz_good_len) {
                if (u1d == 0) lz_out_literal(c, stage_byte(c, c.wnd_curpos));
                else lz_out_nonlit(c, u1l, u1d, stage_byte(c, c.wnd_curpos + u1l - 1));
                TM_ADD(c, 10);
                mf_slide_pos(c, c.wnd_curpos, u1l, size - i);
                i += u1l; c.wnd_curpos += u1l;
                got_u1 = false;
            } else {
                phase = 1;
            }
            continue;
        }
        phase = 0;
        if (second_better(u1l, u1d, fl, fd)) {
            lz_out_literal(c, stage_byte(c, c.wnd_curpos));
            TM_ADD(c, 10);
            i++; c.wnd_curpos++;                 // SlidePos(.., 1, ..) inserts nothing (:191)
            u1l = fl; u1d = fd;
            got_u1 = true;
        } else {
            lz_out_nonlit(c, u1l, u1d, stage_byte(c, c.wnd_curpos + u1l - 1));
            TM_ADD(c, 10);
            mf_slide_pos(c, c.wnd_curpos + 1, u1l - 1, size - i - 1);
            i += u1l; c.wnd_curpos += u1l;
            got_u1 = false;
        }
    }
}

// LZ::ap_backward, csc_lz.cpp:335-362 (over the per-node log; node `end` is still in the ring)
DEV void lz_ap_backward(Sc &c, uint32_t end)
{
    EncLds *L = c.L;
    for (uint32_t i = end; i;) {
        uint32_t b = UNI(L->fin_back[i]);
        L->fin_next[b] = (uint16_t)i;
        i = b;
    }
    for (uint32_t i = 0; i != end;) {
        uint32_t next = UNI(L->fin_next[i]);
        uint32_t nd = UNI(L->fin_dist[next]);
        if (nd == 0) {
            encode_literal(c, UNI(L->fin_lit[i]));
        } else if (nd <= 4) {
            if (next - i == 1 && nd == 1) encode_rep0len1(c);
            else encode_rep_match(c, nd - 1, next - i - 2);
            c.ctx = UNI(L->fin_lit[next - 1]);
        } else {
            encode_match(c, nd - 5, next - i - 2);
            c.ctx = UNI(L->fin_lit[next - 1]);
        }
        i = next;
    }
    L->rep[c.lane & 3u] = L->rg_rep[(end & 255u) * 4 + (c.lane & 3u)];      // (every lane: no lane-dependent branch, csc_kernels.hip / emit_block)
}

// LZ::compress_advanced, csc_lz.cpp:207-333.
//
// Differences in FORM from the reference, none in result:
//  * a node's coder state and rep distances are written when the node is (re)labelled -- by the
//    lane that relaxes it, from the predecessor's final state -- instead of being derived at visit
//    time from (back_pos, dist) (:231-268); the predecessor is final when it relaxes, so the values
//    are the same, and a visit becomes one LDS round trip;
//  * nodes live in a 256-slot LDS ring + a per-node log (see EncLds): four streams fit one CU;
//  * node 0 is the live coder state, so the reference's first FindMatchWithPrice (:211) and the
//    in-loop one (:267) share one call site; the three ways out share one ap_backward;
//  * the per-length price table never leaves registers (length 2 + lane lives in lane `lane`);
//  * the 8 probability fetches of GetLiteralPrice are issued before the match search and consumed
//    after it (p_lit cannot change inside a DP run: nothing is coded until the way out).
DEV void lz_compress_advanced(Sc &c, uint32_t size)
{
    EncLds *L = c.L;
    size = UNI(size);
    for (uint32_t i = 0; i < size;) {
        sc_uniform(c);                  // (once a DP window: see there)
        i = UNI(i);
        uint32_t a0l = 1, a0d = 0;
        uint32_t apcur = 0, apend = 1;
        const uint32_t aplimit = umin(kAPLimit, size - i);
        for (;;) {
            TM_DECL;
            // bytes wpos-1 .. wpos+6 in one LDS fetch: literal context, literal, hash input
            const uint32_t sidx = c.wnd_curpos - c.stage_base + 16;
            uint64_t v9 = stage_load8(L->stage, sidx - 1);
            const uint32_t b01 = UNI((uint32_t)v9), b45 = UNI((uint32_t)(v9 >> 32));
            const uint32_t lit_ctx = c.wnd_curpos ? (b01 & 0xFFu) : 0u;
            const uint32_t cur_lit = (b01 >> 8) & 0xFFu;
            // hashes + table gather of this position start now; the entries are needed only after the node is read
            const MfPre pre = mf_pre(c, (b01 >> 8) | (b45 << 24), b45 >> 8);
            // GetLiteralPrice's probabilities (:301), in flight during the match search
            const uint32_t lk = c.lane & 7, lcc = cur_lit | 0x100u;
            const uint32_t plit_raw = c.p_lit[lit_ctx * 256 + (lcc >> (8 - lk))];
            // this node's coder state, rep distances and price so far; log what the back-trace needs
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
            if (apcur < aplimit) {
                TM_ADD(c, 4);
                mf_find_priced(c, cur_state, c.wnd_curpos, size - i - apcur, pre, r0, r1, r2, r3, a0l, a0d, has1, p1, lane_dist, lane_price, t_lit0);
                TM_RESET;
            }
            // ---- ways out of the DP ----
            uint32_t exit_kind = 0;   // 1 = window limit (:271), 2 = dead end -> literal (:277, and :213 when apcur == 0), 3 = match (:290)
            if (apcur == 0 && a0d == 0) exit_kind = 2;
            else if (apcur == aplimit) exit_kind = 1;
            else if (a0l == 1 && apcur + 1 == apend) exit_kind = 2;
            else {
                if (apcur + 1 >= apend) { L->rg_price[apend & 255u] = 0xFFFFFFFFu; apend++; }
                if (a0l >= c.lz_good_len || (a0l > 1 && a0l + apcur >= aplimit)) exit_kind = 3;
            }
            if (exit_kind) {
                lz_ap_backward(c, apcur);
                i += apcur;
                if (exit_kind == 2) {
                    encode_literal(c, cur_lit);
                    c.wnd_curpos++;
                    i++;
                } else if (exit_kind == 3) {
                    lz_encode_nonlit(c, a0l, a0d);
                    mf_slide_pos(c, c.wnd_curpos, a0l, size - i);
                    i += a0l;
                    c.wnd_curpos += a0l;
                    c.ctx = stage_byte(c, c.wnd_curpos - 1);
                }
                TM_ADD(c, 6);
                break;
            }
            // literal step (:300-307): price = flag + 8 tree bits
            uint32_t cprice;
            {
                uint32_t bit = (lcc >> (7 - lk)) & 1;
                uint32_t pr = L->p2b[(bit ? plit_raw : 4096u - plit_raw) >> 3];
                pr += dpp_row_shr<1>(0, pr);
                pr += dpp_row_shr<2>(0, pr);
                pr += dpp_row_shr<4>(0, pr);
                cprice = rdlane(pr, 7) + t_lit0;   // lanes 0..7 hold the 8 tree bits
            }
            const uint32_t s1slot = (apcur + 1) & 255u;
            uint32_t nprice = UNI(L->rg_price[s1slot]);
            uint32_t n_dist = 0xFFFFFFFFu;   // what node apcur+1 gets relabelled with (0 literal, 1 rep0len1)
            if (cprice + base_price < nprice) { nprice = cprice + base_price; n_dist = 0; }
            if (has1 && p1 + base_price < nprice) { nprice = p1 + base_price; n_dist = 1; }   // :309-313
            if (n_dist != 0xFFFFFFFFu) {
                L->rg_dist[s1slot] = n_dist;
                L->rg_back[s1slot] = (uint16_t)apcur;
                L->rg_price[s1slot] = nprice;
                L->rg_state[s1slot] = (uint8_t)((cur_state * 4 + (n_dist ? 2 : 0)) & 0x3F);
                L->rg_rep[s1slot * 4 + 0] = r0; L->rg_rep[s1slot * 4 + 1] = r1;
                L->rg_rep[s1slot * 4 + 2] = r2; L->rg_rep[s1slot * 4 + 3] = r3;
            }
            const uint32_t len = a0l;
            // while (apcur + len >= apend) apunits_[apend++].price = 0xFFFFFFFF;  (:316-317)
            if (apcur + len >= apend) {
                // (a loop under one count; the lanes behind the last node write its slot once more)
                for (uint32_t t0 = apend; t0 <= apcur + len; t0 += 64) L->rg_price[umin(t0 + c.lane, apcur + len) & 255u] = 0xFFFFFFFFu;
                apend = apcur + len + 1;
            }
            // relax every length 2..len, one per lane (:319-326; targets are distinct).  No lane-dependent branch: a lane whose edge
            // does not win stores into the ring slot of the node being visited -- dead once the node has been read (it is labelled
            // anew, every field, before the ring comes round to it)
            for (uint32_t l0 = 2; l0 <= len; l0 += 64) {
                const uint32_t ll = l0 + c.lane;
                const bool in = ll <= len;
                const uint32_t lli = in ? ll : 2u;
                const uint32_t ad = l0 == 2 ? lane_dist : L->appt_dist[lli];
                const uint32_t pr = l0 == 2 ? lane_price : L->appt_price[lli];
                const uint32_t t0 = (apcur + ll) & 255u;
                const uint32_t was = L->rg_price[t0];                                  // (read by every lane: `&&` would make the load a branch)
                const bool win = in & (ad != 0) & (pr + base_price < was);
                const uint32_t t = win ? t0 : slot;
                L->rg_dist[t] = ad;
                L->rg_back[t] = (uint16_t)apcur;
                L->rg_price[t] = pr + base_price;
                // rep match: move-to-front (:246-259); ordinary match: push (:261-266) -- as selects
                const bool isrep = ad <= 4;
                const uint32_t rsel0 = L->cd2[c.wv][(ad - 1) & 3u];          // cd[0..3] = this node's rep distances
                const uint32_t ns = (cur_state * 4 + (isrep ? 3u : 1u)) & 0x3F;
                const uint32_t n0 = isrep ? rsel0 : ad - 4;
                const uint32_t n1 = (isrep && ad == 1) ? r1 : r0;
                const uint32_t n2 = (isrep && ad <= 2) ? r2 : r1;
                const uint32_t n3 = (isrep && ad <= 3) ? r3 : r2;
                L->rg_state[t] = (uint8_t)ns;
                L->rg_rep[t * 4 + 0] = n0; L->rg_rep[t * 4 + 1] = n1; L->rg_rep[t * 4 + 2] = n2; L->rg_rep[t * 4 + 3] = n3;
            }
            apcur++;
            c.wnd_curpos++;   // SlidePos(.., 1, ..) inserts nothing (:329)
            TM_ADD(c, 5);
        }
    }
}

DEV void lz_compress_advanced_dp4(Sc &c, uint32_t size);    // csc_kernels_dp4.inc
DEV void d4_master_call(Sc &c, uint32_t size);              // the same as a function of its own
DEV void lz_compress_advanced_bt(Sc &c, uint32_t size);     // csc_kernels_bt.inc
DEV void bt_parser_call(Sc &c, uint32_t size);              // the same as a function of its own (see the end of csc_kernels_bt.inc)
DEV bool bt_ok(const Sc &c, uint32_t size);
DEV void lz_compress_normal_hp(Sc &c, uint32_t size, bool lazy);   // csc_kernels_hp.inc
DEV void hp_parser_call(Sc &c, uint32_t size, bool lazy);          // the same as a function of its own
DEV bool hp_ok(const Sc &c);

// LZ::EncodeNormal, csc_lz.cpp:61-100
// FORM of the advanced parser on hash-table configurations: 0 / 5 one wavefront, 2 pipeline around a register-resident DP (dp4); binary-tree
// configurations: 3 inserter wavefront ahead of the parser (csc_kernels_bt.inc); lazy levels: 4 the same for the hash bucket (csc_kernels_hp.inc)
template <int PARSER, int FORM>
DEV void lz_encode_normal(Sc &c, const gu8 *src, uint32_t size, uint32_t lz_mode)
{
    // lazy levels, kernel launched with a coder wavefront: the model + range coder go to wavefront 1 for this pass
    const bool two_waves = PARSER == 2 && lz_mode != 5 && c.pipe_ok;
    if (two_waves) pipe_begin(c);
    for (uint32_t i = 0; i < size;) {
        uint32_t cur = umin(c.wnd_size - c.wnd_curpos, size - i);
        cur = umin(cur, kMinBlock);
        // memcpy(wnd_ + wnd_curpos_, src + i, cur), 64 lanes
        {
            const gu8 *s = src + i;
            TM_DECL;
            // stage the sub-block (+16 bytes of history, +48 of whatever the window holds after it:
            // hashes at the tail read those stale bytes, SURVEY App. C #4) in LDS
            c.stage_base = c.wnd_curpos;
            c.stage_end = c.wnd_curpos + cur + 40;
            uint32_t first = c.wnd_curpos >= 16 ? 0u : 16u - c.wnd_curpos;   // nothing before window position 0
            uint8_t *sb = (uint8_t *)c.L->stage;
            lanes_copy_stage(c.wnd, s, sb, c.wnd_curpos, first, cur);      // (copy and stage in one: both take the sub-block from s)
            wave_fence();
            TM_ADD(c, 9);
        }
        if (lz_mode == 5) {
            // compress_mf_skip (:201-205) under SetArg(1, 1, 0, good_len) (:82-84)
            mf_slide_pos_fast(c, c.wnd_curpos, cur);
            c.wnd_curpos += cur;
        } else {
            if (PARSER == 3) {
                // the many-wavefront forms where the kernel has them; the one-wavefront form otherwise and for the corner cases they do not
                // cover (pos_ about to be renormalised)
                if (FORM == 3 && bt_ok(c, cur)) bt_parser_call(c, cur);
                else if (FORM == 2 && c.pair_ok && c.pos < 0xFFFF0000u) d4_master_call(c, cur);
                else lz_compress_advanced(c, cur);
            }
            else if (FORM == 4 && hp_ok(c)) hp_parser_call(c, cur, lz_mode == 2);
            else lz_compress_normal(c, cur, lz_mode == 2);
        }
        if (c.wnd_curpos >= c.wnd_size) c.wnd_curpos = 0;
        i += cur;
    }
    if (lz_mode != 5) {
        if (c.piped) tok_push(c, TOK_NONLIT_KEEPCTX | (2u << 16), 64 + 5);   // EncodeMatch(64, 0), csc_lz.cpp:97
        else encode_match(c, 64, 0);
    }
    if (two_waves) pipe_end(c);
}
