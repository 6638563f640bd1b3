// csc_kernels_blocks.inc -- filters, block dispatch and the __global__ entry points.
// Included by csc_kernels.hip inside namespace cscmi.

// ==========================================================================================
// Filters (csc_filters.cpp), executed by the stream's wavefront on the chunk buffer in place

// Filters::Forward_E89, csc_filters.cpp:508-598.  The reference drives an 8-byte delay line;
// unrolled, it is: scan j upward, at an E8/E9 opcode (with >= 5 bytes after it) look at the
// little-endian operand at j+1; if its top byte is 00/FF rewrite it as xswap((x + j+5) & 0x1FFFFFF);
// then skip to j+4 (`k = i+4`, :545).  Opcode candidates are found 64 at a time with a ballot;
// only the skip chain is serial.  (A rewritten operand's top byte stays 00/FF, so rewriting
// never creates or destroys a later candidate.)
DEV uint32_t e89_xswap(uint32_t x)   // :527-531
{
    x <<= 7;
    return (x >> 24) | (((x >> 16) & 0xFFu) << 8) | (((x >> 8) & 0xFFu) << 16) | ((x & 0xFFu) << (24 - 7));
}
DEV void flt_forward_e89(Sc &c, gu8 *src, uint32_t size)
{
    uint32_t next_ok = 0;
    for (uint32_t base = 0; base + 5 < size; base += 64) {
        uint32_t j0 = base + c.lane;
        bool cand = false;
        if (j0 + 5 < size) cand = (src[j0] & 0xFEu) == 0xE8u;
        uint64_t m = __ballot(cand);
        while (m) {
            uint32_t bit = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            uint32_t j = base + bit;
            if (j < next_ok) continue;
            next_ok = j + 4;
            uint64_t v = load8u(src + j + 1);
            uint32_t x = UNI((uint32_t)v) - 0xFF000000u;
            if (x < 0x02000000u) {
                x = (x + (j + 5)) & 0x01FFFFFFu;
                x = e89_xswap(x) + 0xFF000000u;
                src[j + 1] = (uint8_t)x; src[j + 2] = (uint8_t)(x >> 8);
                src[j + 3] = (uint8_t)(x >> 16); src[j + 4] = (uint8_t)(x >> 24);
            }
        }
        wave_fence();
    }
}

// Filters::Forward_Delta, csc_filters.cpp:132-164: de-interleave chn channels, byte-difference
// against the previously EMITTED byte (the predecessor is not reset between channels).
DEV void flt_forward_delta(Sc &c, gu8 *src, uint32_t size, uint32_t chn)
{
    if (size < 512) return;
    gu8 *copy = c.swapbuf;
    for (uint32_t t = c.lane; t < size; t += 64) copy[t] = src[t];
    wave_fence();
    for (uint32_t j = c.lane; j < size; j += 64) {
        uint32_t ch = j % chn, idx = j / chn;
        uint32_t dst = idx;
        for (uint32_t k = 0; k < ch; k++) dst += (size - k + chn - 1) / chn;
        uint32_t prev = 0;
        if (idx > 0) prev = copy[j - chn];
        else if (ch > 0) {
            uint32_t nprev = (size - (ch - 1) + chn - 1) / chn;
            prev = copy[(ch - 1) + (nprev - 1) * chn];
        }
        src[dst] = (uint8_t)(copy[j] - prev);
    }
    wave_fence();
}

// Filters::Foward_Dict, csc_filters.cpp:256-335, kDictW steps of 64 positions a pass (lane l of group g stands for position base + 64 g + l), in ONE pass
// over the run:
//  * every position's longest trie word from the eight bytes the lane has loaded.  The trie is packed into one word an edge while it is loaded into LDS --
//    next node | (word index + 1) << 9, the word's symbol being 0x81 + that field -- so a level is one dependent LDS read, and the groups walk their levels in
//    lock step: kDictW reads are in flight a level;
//  * which positions are real token starts -- the greedy chain p -> p + advance(p) -- without walking it: with advances of 1..4
//    "how far is the next token start" is a four-state automaton, a position is a function on its states (state 0: a token starts
//    here, new state = advance - 1; else state - 1), and function composition is associative: a scan over a group's 64 functions
//    (a byte per state: composing two is ONE v_perm_b32) gives every lane the function from the group's entry to itself.  The scans do not depend on the
//    state the chain arrives in, so the groups' scans run side by side (DPP row shifts and row broadcasts: no LDS round trip); group g's entry state is
//    group g - 1's total applied to its own, a lane read and a byte select a group, and the last group's carries the chain into the next pass;
//  * the chosen lanes emit 1 or 2 bytes at ballot-prefix offsets.  Every lane stores -- one with nothing to emit into a dump slot beyond the
//    2 * size bytes the output can take in the scratch -- so the stores of a pass are a fixed number and the wait for the next pass's bytes can count them instead of draining them.
// Returns 1 if the run was replaced.
DEV uint32_t umax16(uint32_t a, uint32_t b) { return a > b ? a : b; }
// state -> B(A(state)) for functions kept as four bytes (byte s = image of state s): the later function's bytes selected by the earlier one's
DEV uint32_t flt_compose(uint32_t A, uint32_t B) { return __builtin_amdgcn_perm(0u, B, A); }
constexpr int kDictW = 2;                        // (measured against 4 and 8: profiles/dict_wide.md)
constexpr uint32_t kFltIdent = 0x03020100u;      // the identity: what a position beyond the run's, or a lane a DPP shift brings nothing to, stands for
constexpr uint32_t kTrieEdges = 300 * 26;
// the lane's function moved along the wavefront: CTRL row_shr:n (0x110 + n), row_bcast:15 (0x142, ROWS 0xA), row_bcast:31 (0x143, ROWS 0xC), wave_shr:1 (0x138)
template <int CTRL, int ROWS> DEV uint32_t flt_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)kFltIdent, (int)v, CTRL, ROWS, 0xF, false); }
DEV uint32_t flt_mbcnt(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
#define FLT_SCAN(CTRL, ROWS) _Pragma("unroll") for (int g = 0; g < W; g++) inc[g] = flt_compose(flt_dpp<CTRL, ROWS>(inc[g]), inc[g])
DEV uint32_t flt_forward_dict(Sc &c, gu8 *src, uint32_t size)
{
    size = UNI(size);                                     // (arguments of the function-call form arrive in vector registers)
    src = uni_gptr(src);
    if (size < 16384) return 0;
    constexpr int W = kDictW;
    EncLds *L = c.L;
    const GLOBAL_AS EncState *G = (const GLOBAL_AS EncState *)uni_gptr(c.S);
    gu8 *dst = uni_gptr(c.swapbuf);
    const uint32_t n5 = size - 5;
    // the trie borrows the LDS of the (idle) DP nodes for the duration of the filter; eight edges a lane are in flight
    {
        const gu16 *tn = (const gu16 *)G->trie_next;
        const gu8 *ts = (const gu8 *)G->trie_sym;
        for (uint32_t i0 = c.lane; i0 < kTrieEdges; i0 += 64u * 8u) {
            uint32_t nx[8], sy[8];
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = tn[umin(i0 + 64u * k, kTrieEdges - 1u)];
#pragma unroll
            for (int k = 0; k < 8; k++) sy[k] = ts[nx[k]];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (i0 + 64u * k < kTrieEdges) L->trie_next[i0 + 64u * k] = (uint16_t)((nx[k] && sy[k]) ? nx[k] | ((sy[k] - 0x81u) << 9) : nx[k]);
        }
    }
    uint32_t s_in = 0, dst_size = 0;
    // The dump slot: 64 bytes at 3 * size.  The output is at most 2 * size bytes (every byte escaped), so anything from there on is free; 3 * size keeps the
    // slot a whole `size` clear of it and inside the scratch, which the host allocates as 4 * raw_blocksize + 512 bytes (csc_host.cpp, o_swap) for runs of
    // at most raw_blocksize + 256 bytes (the chunk buffer's size): 3 * size + 64 <= 3 * raw_blocksize + 832 < 4 * raw_blocksize + 512 from 16 384 up.
    gu8 *const dump = dst + 3u * (size_t)size + c.lane;
    // a lane's eight bytes: three aligned dwords + v_alignbyte.  The next pass's dwords travel while this pass works and are put together
    // at its head; the byte offset inside the dword is the lane's own in every pass (a pass is 64 W positions on).  Positions beyond
    // the walked range load the dwords of position n5 instead and are never looked at.
    const uint32_t sh = (uint32_t)(uintptr_t)(src + c.lane) & 3u;
    uint32_t rawn[W][3];
#pragma unroll
    for (int g = 0; g < W; g++) {
        const gu32 *q = (const gu32 *)((uintptr_t)(src + umin(64u * g + c.lane, n5)) & ~(uintptr_t)3);
        rawn[g][0] = q[0]; rawn[g][1] = q[1]; rawn[g][2] = q[2];
    }
    for (uint32_t base = 0; base < n5; base += 64u * W) {
        uint64_t v8[W];
        uint32_t b[W], sym[W], adv[W], node[W], inc[W];
        bool valid[W], go[W];
#pragma unroll
        for (int g = 0; g < W; g++)
            v8[g] = ((uint64_t)__builtin_amdgcn_alignbyte(rawn[g][2], rawn[g][1], sh) << 32) | __builtin_amdgcn_alignbyte(rawn[g][1], rawn[g][0], sh);
#pragma unroll
        for (int g = 0; g < W; g++) {
            const gu32 *q = (const gu32 *)((uintptr_t)(src + umin(base + 64u * (W + g) + c.lane, n5)) & ~(uintptr_t)3);
            rawn[g][0] = q[0]; rawn[g][1] = q[1]; rawn[g][2] = q[2];
        }
#pragma unroll
        for (int g = 0; g < W; g++) {
            valid[g] = base + 64u * g + c.lane < n5;
            b[g] = (uint32_t)v8[g] & 0xFFu;
            sym[g] = 0; adv[g] = 1; node[g] = 0; go[g] = valid[g];
        }
        // the groups' trie walks, level by level, until no lane of any group continues (a lane that has stopped reads edge 0 and ignores it)
        for (uint32_t j = 1; j <= 8; j++) {
            uint32_t e[W];
#pragma unroll
            for (int g = 0; g < W; g++) {
                const uint32_t idx = ((uint32_t)v8[g] & 0xFFu) - 'a';
                go[g] = go[g] && idx <= 25u;
                e[g] = L->trie_next[go[g] ? node[g] * 26u + idx : 0u];
                v8[g] >>= 8;
            }
            bool any = false;
#pragma unroll
            for (int g = 0; g < W; g++) {
                const uint32_t nx = e[g] & 511u, f = e[g] >> 9;
                go[g] = go[g] && nx != 0;
                node[g] = go[g] ? nx : node[g];
                const bool word = go[g] && f != 0;
                sym[g] = word ? 0x81u + f : sym[g];
                adv[g] = word ? j : adv[g];
                any = any || go[g];
            }
            if (!__ballot(any)) break;
        }
#pragma unroll
        for (int g = 0; g < W; g++) inc[g] = valid[g] ? (((adv[g] - 1u) & 3u) | 0x02010000u) : kFltIdent;      // beyond the run's positions: the identity
        // inclusive scans, the groups side by side: inside the rows of 16, row 0 into row 1 and row 2 into row 3, rows 0-1 into rows 2-3
        FLT_SCAN(0x111, 0xF); FLT_SCAN(0x112, 0xF); FLT_SCAN(0x114, 0xF); FLT_SCAN(0x118, 0xF);
        FLT_SCAN(0x142, 0xA); FLT_SCAN(0x143, 0xC);
        uint32_t s = s_in;                                   // distance to the next token start on entry to the group
#pragma unroll
        for (int g = 0; g < W; g++) {
            const uint32_t prev = flt_dpp<0x138, 0xF>(inc[g]);                    // the function up to the position before this one (lane 0: the identity)
            const uint32_t sb = (prev >> (8u * s)) & 3u;                          // distance to the next token start, before this position
            const bool mine = valid[g] && sb == 0;
            const uint64_t on = __ballot(mine);
            const bool two = mine && sym[g] == 0 && b[g] >= 0x82;
            const uint64_t m2 = __ballot(two);
            const uint32_t off = dst_size + flt_mbcnt(on) + flt_mbcnt(m2);
            gu8 *const a1 = mine ? dst + off : dump, *const a2 = two ? dst + off + 1 : dump;
            *a1 = (uint8_t)(sym[g] ? sym[g] : two ? 254u : b[g]);
            *a2 = (uint8_t)b[g];
            dst_size += (uint32_t)__builtin_popcountll(on) + (uint32_t)__builtin_popcountll(m2);
            s = (rdlane(inc[g], 63) >> (8u * s)) & 3u;                             // (positions beyond the run's are the identity: lane 63 holds the group's total)
        }
        s_in = s;
    }
    const uint32_t p = n5 + s_in;                           // where the chain leaves the walked range
    wave_fence();
    for (uint32_t i = p; i < size; i++) {   // last bytes: escape only (:319-326)
        uint32_t b = ldb(src + i);
        if (b >= 0x82) { dst[dst_size++] = 254; dst[dst_size++] = (uint8_t)b; }
        else dst[dst_size++] = (uint8_t)b;
    }
    if ((double)dst_size > (double)size * 0.82) return 0;   // :328
    wave_fence();
    // the run is replaced, padded with blanks to its size (:332): 16 bytes a lane (src and the scratch are 16-byte aligned, and do not overlap)
    {
        const uint32_t full = dst_size & ~15u;
        gvec4 *d4 = (gvec4 *)src;
        raw_vec4 blanks; blanks.x = blanks.y = blanks.z = blanks.w = 0x20202020u;
        lanes_copy16_far(d4, (const gvec4 *)dst, full >> 4);
        for (uint32_t t = full + c.lane; t < umin(full + 16u, size); t += 64) src[t] = t < dst_size ? dst[t] : (uint8_t)0x20;
        for (uint32_t t = full + 16u + c.lane * 16u; t + 16u <= size; t += 1024u) d4[t >> 4] = blanks;
        for (uint32_t t = umax16(full + 16u, size & ~15u) + c.lane; t < size; t += 64) src[t] = (uint8_t)0x20;
    }
    wave_fence();
    return 1;
}
#undef FLT_SCAN

// ==========================================================================================
// CSCEncoder::compress_block, csc_encoder_main.cpp:35-83.  Same order of effects as the
// reference's if-chain, arranged as pre-step / one LZ pass / post-step so that the parser is
// instantiated once.
// The pipeline form's kernel (FORM 2) runs its filters as functions of their own (round 5's review): inlined into the kernel body -- twelve wavefronts, i.e. 170
// VGPRs a lane -- they were where its 722 spilled VGPRs and 1 272 scratch instructions sat.  Plain arguments (nothing travels through private memory) and the LDS
// image by name (a generic pointer would turn the trie walk's loads into flat ones); the context is rebuilt from them, every field the filter does not use dead.
#if CSCMI_TU != 2
template <int WHICH>
__device__ __noinline__ uint32_t flt_dp4_nl(EncState *S, gu8 *swapbuf, gu8 *src, uint32_t size, uint32_t chn)
{
    Sc c;
    c.S = S; c.L = &g_lds4.base; c.swapbuf = swapbuf; c.lane = threadIdx.x & 63u;
    if (WHICH == 0) { flt_forward_e89(c, src, size); return 0; }
    if (WHICH == 1) return flt_forward_dict(c, src, size);
    flt_forward_delta(c, src, size, chn);
    return 0;
}
#endif
template <int PARSER, int FORM>
DEV void enc_compress_block(Sc &c, gu8 *src, uint32_t size, uint32_t type)
{
    if (size == 0) return;
    uint32_t mode = c.S->lz_mode;
    const bool is_dlt = type >= DT_DLT && type < DT_DLT + 5;
    if (type == DT_NORMAL) {
        encode_int(c, type);
    } else if (type == DT_EXE) {
        encode_int(c, type);
#if CSCMI_TU != 2
        if (FORM == 2) (void)flt_dp4_nl<0>(uni_gptr(c.S), uni_gptr(c.swapbuf), uni_gptr(src), UNI(size), 0);
        else
#endif
        flt_forward_e89(c, src, size);
    } else if (type == DT_ENGTXT) {
        TM_DECL;
        uint32_t ok;
#if CSCMI_TU != 2
        if (FORM == 2) ok = UNI(flt_dp4_nl<1>(uni_gptr(c.S), uni_gptr(c.swapbuf), uni_gptr(src), UNI(size), 0));
        else
#endif
        ok = flt_forward_dict(c, src, size);
        TM_ADD(c, 8);
        c.S->dict_result = ok;
        if (ok) { encode_int(c, type); encode_int(c, size); }
        else encode_int(c, DT_NORMAL);
    } else if (type == DT_FAST) {
        encode_int(c, DT_NORMAL);          // "fast mode" is disabled in the reference (:56-59)
    } else if (type == DT_BAD || type == DT_ENTROPY || is_dlt) {
        encode_int(c, type);
        mode = 5;                          // window + sparse MF insert only, no LZ output
    } else {
        c.error = ERR_BAD_TYPE;
        return;
    }
    lz_encode_normal<PARSER, FORM>(c, src, size, mode);
    if (type == DT_BAD) compress_bad(c, src, size);
    else if (type == DT_ENTROPY) compress_literals(c, src, size);
    else if (is_dlt) {
#if CSCMI_TU != 2
        if (FORM == 2) (void)flt_dp4_nl<2>(uni_gptr(c.S), uni_gptr(c.swapbuf), uni_gptr(src), UNI(size), kDltIndex[type - DT_DLT]);
        else
#endif
        flt_forward_delta(c, src, size, kDltIndex[type - DT_DLT]);
        compress_rle(c, src, size);
    }
}

// LZ::IsDuplicateBlock / MatchFinder::TestFind (csc_lz.cpp:102-112, csc_mf.cpp:526-568) by the stream's own wavefront, against
// the tables as the runs compressed so far leave them: 64 offsets of the block per round, one per lane.  Only offsets with
// HASH2 % 16 == 0 are probed; the bucket index lacks `+i` in the reference (:538), so only slot 0 is; the window side of every
// compare starts at wnd_curpos - distance whatever the offset (the reference passes wnd_curpos_ for every i).
DEV bool dev_is_duplicate(Sc &c, const gu8 *src, uint32_t size)
{
    wave_fence();
    const uint32_t wpos = c.wnd_curpos, vld = c.vld_rge, wsz = c.wnd_size;
    for (uint32_t base = 0; base < size; base += 64) {
        const uint32_t i = base + c.lane;
        bool hit = false;
        if (i < size) {
            const uint64_t v = load8u(src + i);
            const uint32_t lo = (uint32_t)v, hi2 = (uint32_t)(v >> 32) & 0xFFFFu;
            if ((hash2_of(lo) & 15u) == 0) {
                const uint32_t hv = hash6_mul(lo, hi2);
                const uint32_t limit = size - i;
                uint32_t d[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
                if (c.ht_width) d[0] = c.pos - c.ht6[(size_t)(hv >> (32 - c.ht_bits)) * c.ht_width];
                if (c.bt_head) d[1] = c.pos - c.bt_head[hv >> (32 - c.bt_bits)];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const uint32_t dist = d[k];
                    if (dist >= vld) continue;
                    const uint32_t cp = wpos >= dist ? wpos - dist : wpos + wsz - dist;
                    const uint32_t climit = umin(limit, wsz - cp);
                    if (climit <= 18) continue;
                    // more than 18 equal bytes: the first 19
                    const gu8 *q = c.wnd + cp;
                    const bool e0 = load8u(src + i) == load8u(q), e1 = load8u(src + i + 8) == load8u(q + 8);
                    const uint64_t t2 = (load8u(src + i + 16) ^ load8u(q + 16)) & 0xFFFFFFull;
                    hit = hit || (e0 && e1 && t2 == 0);
                }
            }
        }
        if (__ballot(hit)) return true;
    }
    return false;
}

// CSCEncoder::Compress, csc_encoder_main.cpp:85-147, by the stream's kernel itself: block typing from the analyzer's verdicts
// (k_analyze has filled S->binfo), the DT_SKIP / filter-switch / bpb rules, IsDuplicateBlock against the tables as the runs
// compressed SO FAR leave them (the pending run is not compressed yet, exactly as in the reference), equal-type runs of up to
// raw_blocksize.  One launch per chunk, no verdict travels to the host: a batch of streams needs no rounds.  Written as an
// iterator -- seg_next hands out the next run to compress -- so that the kernels keep ONE instance of the block compressor.
struct SegWalk { uint32_t csize, i, blk, last_type, last_begin, last_size, bpb; };
DEV void seg_start(SegWalk &w, uint32_t csize) { w.csize = csize; w.i = 0; w.blk = 0; w.last_type = DT_NORMAL; w.last_begin = 0; w.last_size = 0; w.bpb = 0; }
// -> true: compress [off, off + size) as `type`, then EncodeInt(tail) (tail 1: + coder flush, the chunk is complete)
DEV bool seg_next(Sc &c, SegWalk &w, uint32_t &type, uint32_t &off, uint32_t &size, uint32_t &tail)
{
    EncState *S = c.S;
    const gu8 *src = (const gu8 *)S->inbuf;
    const uint32_t ff = S->filt_flags;
    const BlockInfo *binfo = S->binfo;
    while (w.i < w.csize) {
        const uint32_t cur = umin(kMinBlock, w.csize - w.i);
        uint32_t this_type = DT_NORMAL;
        if (ff) {
            this_type = UNI(binfo[w.blk].type);
            if (this_type != DT_SKIP) w.bpb = UNI(binfo[w.blk].bpb);
        }
        if (this_type == DT_SKIP) this_type = w.last_type;
        if (this_type != DT_NORMAL) {
            if (this_type == DT_EXE && !(ff & 4u)) this_type = DT_NORMAL;
            else if (this_type == DT_ENGTXT && !(ff & 2u)) this_type = DT_NORMAL;
            else if (this_type >= DT_DLT && !(ff & 1u)) this_type = DT_NORMAL;
        }
        if (this_type >= DT_DLT && (double)UNI(binfo[w.blk].dlt_bpb[this_type - DT_DLT]) >= w.bpb * 0.95) this_type = DT_NORMAL;   // :117-121
        if (this_type >= DT_NO_LZ && dev_is_duplicate(c, src + w.i, cur)) this_type = DT_NORMAL;                                    // :123-126
        const bool close = (w.last_type != this_type || w.last_size + cur > S->raw_blocksize) && w.last_size;
        if (w.last_type != this_type || w.last_size + cur > S->raw_blocksize) {
            type = w.last_type; off = w.last_begin; size = w.last_size; tail = 0;
            w.last_begin = w.i;
            w.last_size = 0;
        }
        w.last_type = this_type;
        w.last_size += cur;
        w.i += cur;
        w.blk++;
        if (close) return true;
    }
    if (w.last_size) { type = w.last_type; off = w.last_begin; size = w.last_size; tail = 1; w.last_size = 0; return true; }
    return false;
}

// ------------------------------------------------------------------------------------------
// the register part of a stream context: configuration and the state carried between launches, read from EncState (HBM)
DEV void sc_load_regs(Sc &c, EncState *S, EncLds *L)
{
    // (read through a global-address-space pointer: a load through a generic one counts as divergent -- it could be scratch -- and
    // would put every field below into a vector register)
    const GLOBAL_AS EncState *G = (const GLOBAL_AS EncState *)S;
    c.S = S; c.L = L; c.X = nullptr; c.Q = nullptr; c.q_head = 0; c.q_room = 0;
    c.lane = threadIdx.x & 63;
    c.wnd = (gu8 *)G->wnd; c.wnd_size = G->wnd_size; c.vld_rge = G->vld_rge;
    c.ht2 = (gu32 *)G->ht2; c.ht3 = (gu32 *)G->ht3; c.ht6 = (gu32 *)G->ht6; c.bt_head = (gu32 *)G->bt_head; c.bt_nodes = (gu32 *)G->bt_nodes;
    c.p_lit = (gu32 *)G->p_lit; c.p_delta = (gu32 *)G->p_delta; c.swapbuf = (gu8 *)G->swapbuf;
    c.mfbuf = (gu32 *)G->mfbuf;
    c.ht6_off = kHT2Size + kHT3Size;
    c.bth_off = c.ht6_off + (G->ht_width << G->ht_bits);
    {   // lane roles of the per-position entry gather: lanes < width read the HT6 bucket, 32/33/34 read HT2/HT3/BT head
        uint32_t wd = G->ht_width < G->lz_ht_cyc ? G->ht_width : G->lz_ht_cyc;
        c.gm6 = c.lane < wd ? 0xFFFFFFFFu : 0u;
        c.gm2 = c.lane == 32 ? 0xFFFFFFFFu : 0u;
        c.gm3 = c.lane == 33 ? 0xFFFFFFFFu : 0u;
        c.gmb = (c.lane == 34 && G->bt_head) ? 0xFFFFFFFFu : 0u;
        c.gslot = c.lane < 24 ? 7 + c.lane : (c.lane >= 32 && c.lane <= 34) ? c.lane - 28 : 31;
        // lane i < 12 prices bit `pol` under p_state[state*3 + off] (lanes 0-4, 11) or p_repdist[state*3 + off] (lanes 5-10):
        //   0:(S0,1) 1:(S1,0) 2:(S1,1) 3:(S2,0) 4:(S2,1) 5:(R0,0) 6:(R0,1) 7:(R1,0) 8:(R1,1) 9:(R2,0) 10:(R2,1) 11:(S0,0)
        uint32_t i = c.lane < 12 ? c.lane : 0;
        c.pr_off = (i == 0 || i == 11) ? 0u : (i <= 4 ? (i + 1) / 2 : (i - 5) / 2);
        c.pr_rmask = (i >= 5 && i <= 10) ? 0xFFFFFFFFu : 0u;
        c.pr_pol = i == 0 ? 1u : i == 11 ? 0u : ((i - 1) & 1u);
    }
    c.ht_bits = G->ht_bits; c.ht_width = G->ht_width; c.bt_bits = G->bt_bits; c.bt_size = G->bt_size;
    c.lz_good_len = G->lz_good_len; c.lz_bt_cyc = G->lz_bt_cyc; c.lz_ht_cyc = G->lz_ht_cyc;
    // MatchFinder::SetArg(bt_cyc_, ht_cyc_, 1, good_len_), csc_lz.cpp:32 -- lz_mode 5 never searches
    c.bt_cyc = c.lz_bt_cyc; c.ht_cyc = c.lz_ht_cyc; c.ht_low = 1; c.good_len = c.lz_good_len;
    c.bt_pos = G->bt_pos; c.pos = G->pos; c.wnd_curpos = G->wnd_curpos;
    c.state = G->state; c.ctx = G->ctx; c.lp_rebuild_int = G->lp_rebuild_int;
    c.rc_low = G->rc_low; c.rc_range = G->rc_range; c.rc_cache = G->rc_cache; c.rc_cachesize = G->rc_cachesize;
    c.rc_size = G->rc_size; c.bc_size = G->bc_size; c.bc_curbits = G->bc_curbits; c.bc_curval = G->bc_curval;
    c.bsize = G->bsize;
    c.rc_buf = (gu8 *)G->rc_buf; c.bc_buf = (gu8 *)G->bc_buf; c.arena = (gu8 *)G->arena;
    c.arena_used = G->arena_used; c.arena_cap = G->arena_cap; c.error = G->error;
    c.st_find = c.st_slide = c.st_bt = c.st_lit = c.st_match = 0;
    c.stage_base = c.stage_end = 0;
#ifdef CSCMI_TIMERS
    for (int k = 0; k < 16; k++) c.tm[k] = 0;
#endif
    c.pipe_ok = 0; c.piped = 0; c.tok_headl = 0; c.tok_tail_seen = 0; c.pipe_seq = 0;
    c.wv = 0; c.dp_seq = 0; c.dp_idle = 0; c.dp_seq_seen = 0;
}

DEV void sc_load(Sc &c, EncState *S, EncLds *L)
{
    const GLOBAL_AS EncState *G = (const GLOBAL_AS EncState *)S;
    sc_load_regs(c, S, L);
    if (threadIdx.x < 64) {            // the LDS image belongs to wavefront 0 (a coder wavefront only ever reads it after a hand-over)
        for (uint32_t i = c.lane; i < P_COUNT; i += 64) L->P[i] = G->probs[i];
        for (uint32_t i = c.lane; i < 512; i += 64) L->p2b[i] = d_p2bits[i];
        if (c.lane < 32) L->len_price[c.lane] = G->len_price[c.lane];
        if (c.lane < 4) L->rep[c.lane] = G->rep_dist[c.lane];
        if (c.lane == 0) { L->pipe_cmd = 0; L->pipe_ack = 0; L->tok_head = 0; L->tok_tail = 0; L->dp.cmd = 0; L->dp.idle = 0; L->dp.abort = 0; L->dp.bstat[0] = 0; L->dp.dec = 0; }      // (dp: see EncLds)
    }
}

DEV void sc_store(Sc &c)
{
    EncState *S = c.S;
    EncLds *L = c.L;
    for (uint32_t i = c.lane; i < P_COUNT; i += 64) S->probs[i] = L->P[i];
    if (c.lane < 32) S->len_price[c.lane] = L->len_price[c.lane];
    if (c.lane < 4) S->rep_dist[c.lane] = L->rep[c.lane];
    if (c.lane == 0) {
        S->bt_pos = c.bt_pos; S->pos = c.pos; S->wnd_curpos = c.wnd_curpos;
        S->state = c.state; S->ctx = c.ctx; S->lp_rebuild_int = c.lp_rebuild_int;
        if (!c.Q) {      // (pipeline form: the coder wavefront stores what it owns, d4_coder)
            S->rc_low = c.rc_low; S->rc_range = c.rc_range; S->rc_cache = c.rc_cache; S->rc_cachesize = c.rc_cachesize;
            S->rc_size = c.rc_size; S->bc_size = c.bc_size; S->bc_curbits = c.bc_curbits; S->bc_curval = c.bc_curval;
            S->arena_used = c.arena_used; S->error = c.error;
        } else if (c.error) S->error = c.error;
        S->stats.find_match_calls += c.st_find; S->stats.slide_positions += c.st_slide;
        S->stats.bt_steps += c.st_bt; S->stats.literals += c.st_lit; S->stats.matches += c.st_match;
#ifdef CSCMI_TIMERS
        for (int k = 0; k < 16; k++) S->stats.tm[k] += c.tm[k];
#endif
    }
}

// ==========================================================================================
// k_encode_runs: the stream's serial protocol for a list of typed runs of one chunk
// (CSCEncoder::Compress after block typing, csc_encoder_main.cpp:128-145; tail 9 = WriteEOF :154)
// one workgroup = one stream (one wavefront, or the two / three / four / twelve of a many-wavefront form, see encode_stream).  FAST is the hash-table-only specialisation (levels
// 1-4): the binary-tree code paths are compiled out and the vector replay path is taken.
// (An earlier version paired the parser with a prefetch wavefront running ahead over the staged
// sub-block; with the whole stream state resident in the 256 MiB Infinity Cache it bought nothing
// measurable single-stream and cost 4 % with 954 streams, so it was removed.)
// A multi-stream launch reads its stream's pointers out of tables (states[b], runs[b]).  The compiler cannot see that such a
// loaded pointer is the same in all lanes, so everything read through it (the whole Sc) ended up in VECTOR registers: 145 spilled
// VGPRs / 766 scratch instructions in k_encode_runs_multi_dp4 (round 4's code objects) against 24 / 117 in the single-stream twin.
// Passing the words through v_readfirstlane makes them scalar again: the multi instances allocate registers like the single ones.
template <class T>
DEV T *uni_ptr(T *p)
{
    const uint64_t v = (uint64_t)p;
    return (T *)(((uint64_t)UNI((uint32_t)(v >> 32)) << 32) | UNI((uint32_t)v));
}

template <int PARSER, bool FAST, int FORM>
DEV void encode_stream(EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena, EncLds *lds, void *xlds = nullptr)
{
    Sc c;
    sc_load(c, S, lds);
    c.X = xlds;
    if (reset_arena) c.arena_used = 0;   // first launch of a chunk: the host consumed the previous arena (every wavefront: the one that owns the coder needs it)
    if (FORM == 2) d4_init(c, reset_arena);
    if (FORM == 3) bt_init(c, reset_arena);
    if (FORM == 4) hp_init(c);
    if (FAST) { c.bt_head = nullptr; c.bt_nodes = nullptr; c.bt_bits = 0; c.bt_size = 0; c.gmb = 0; c.fast_ht = true; }
    else c.fast_ht = false;
    c.pair_ok = 0;
    if (PARSER == 2) {
        // lazy-parser kernels are launched with two wavefronts per stream (see "token pipe" in csc_kernels_lz.inc)
        // (FORM 4: a third wavefront, the inserter that runs ahead of the parser, csc_kernels_hp.inc)
        __syncthreads();
        if (FORM == 4 && threadIdx.x >= 128) { hp_inserter_call(c); return; }
        if (FORM == 4 && threadIdx.x >= 64) { hp_coder_call(c); return; }
        if (threadIdx.x >= 64) { coder_service(c); return; }
        c.pipe_ok = blockDim.x >= 128 ? 1u : 0u;
    } else if (FORM == 3) {
        // binary tree: wavefront 1 is the inserter that runs ahead of the parser (csc_kernels_bt.inc)
        __syncthreads();
        // four wavefronts, one a SIMD: 0 parser, 1 inserter, 2 post, 3 coder.  (Round 5 also had a finder wavefront -- the candidate search one
        // request ahead of the parser, seven wavefronts launched.  It was measured slower in every form; commit 70dda76 left it switched on
        // by accident, which took silesia -m5 from 0.56 to 0.42 MB/s.  The code is gone; DESIGN.md section 4 has the full record.)
        if (threadIdx.x >= 192) { bt_coder_call(c); return; }               // wavefront 3: range / bit coder arithmetic + byte output (round 5)
        if (threadIdx.x >= 128) { c.wv = 2; bt_post_call(c); return; }      // wavefront 2: per-length pricing + relaxation behind the parser
        if (threadIdx.x >= 64) { bt_inserter_call(c); return; }
        c.Q = bt_coderq(c);                // from here on this wavefront's coded bits go to the coder wavefront
    } else if (FAST) {
        // advanced parser over hash tables: the pipeline form's wavefronts (FORM 2, csc_kernels_dp4.inc), or one wavefront a stream
        __syncthreads();
        if (FORM == 2 && threadIdx.x >= 64) {                        // (the pipeline form's worker wavefronts: csc_kernels_dp4.inc, d4_role)
            c.wv = threadIdx.x >> 6;
            d4_worker_call(c);
            return;
        }
        c.pair_ok = FORM == 2 ? 1u : 0u;                             // (every other form of the advanced parser over hash tables is ONE wavefront a stream since round 6)
        if (FORM == 2) c.Q = d4_coderq(c);   // from here on this wavefront's coded bits go to the coder wavefront
    }
    const bool self_seg = (nruns & kSelfSegment) != 0;
    SegWalk sw;
    seg_start(sw, nruns & ~kSelfSegment);
    for (uint32_t r = 0;; r++) {
        uint32_t type, off, size, tail;
        if (self_seg) { if (!seg_next(c, sw, type, off, size, tail)) break; }
        else {
            if (r >= nruns) break;
            type = UNI(runs[r].type); off = UNI(runs[r].offset); size = UNI(runs[r].size); tail = UNI(runs[r].tail);
        }
        enc_compress_block<PARSER, FORM>(c, (gu8 *)S->inbuf + off, size, type);
        if (tail == 0) encode_int(c, 0);
        else if (tail == 1) { encode_int(c, 1); coder_flush(c); }
        else if (tail == 9) { encode_int(c, SIG_EOF); coder_flush(c); }
    }
    if (PARSER == 2 && c.pipe_ok) { lds_release(); lds_vstore(&lds->pipe_cmd, kPipeQuit); }
    if (FORM == 3) bt_quit(c);
    if (FORM == 4) hp_quit(c);
    if (PARSER == 3 && FAST && FORM == 2) d4_quit(c);
    sc_store(c);
}

template <int PARSER, bool FAST>
__global__ __launch_bounds__(PARSER == 2 ? 128 : 64) void k_encode_runs(EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena)
{
    __shared__ EncLds lds;
    encode_stream<PARSER, FAST, (PARSER == 3 && FAST) ? 5 : 0>(S, runs, nruns, reset_arena, &lds);      // (advanced parser over hash tables outside the level-3 geometry: one wavefront)
}

#if CSCMI_TU != 2
// CSCEnc_Encode_Flush (csc_enc.cpp:193-203): EncodeInt(SIG_EOF) + Coder::Flush.  A kernel of its own so
// that profiles of k_encode_runs contain chunk launches only.
__global__ __launch_bounds__(64) void k_encode_eof(EncState *S)
{
    __shared__ EncLds lds;
    Sc c;
    sc_load(c, S, &lds);
    c.arena_used = 0;
    encode_int(c, SIG_EOF);
    coder_flush(c);
    sc_store(c);
}

#endif

// the same for many independent streams (tasks): workgroup b advances stream b by one chunk
template <int PARSER, bool FAST>
__global__ __launch_bounds__(PARSER == 2 ? 128 : 64) void k_encode_runs_multi(EncState *const *states, const RunDesc *const *runs,
                                                          const uint32_t *nruns, const uint32_t *reset)
{
    __shared__ EncLds lds;
    const uint32_t b = blockIdx.x;
    encode_stream<PARSER, FAST, 0>(uni_ptr(states[b]), uni_ptr(runs[b]), UNI(nruns[b]), UNI(reset[b]), &lds);
}
#if CSCMI_TU != 1
// Binary-tree configurations (level 5) under the advanced parser: parser, inserter and post wavefronts (csc_kernels_bt.inc)
__global__ __launch_bounds__(256) void k_encode_runs_bt(EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena)
{
    encode_stream<3, false, 3>(S, runs, nruns, reset_arena, &g_ldsbt.base, &g_ldsbt.x);
}
#ifndef CSCMI_DEV_ONE      // (CSCMI_DEV_ONE: analysis builds of ONE single-stream kernel, tools/enc_uniformity.py -- never linked)
__global__ __launch_bounds__(256)
void k_encode_runs_multi_bt(EncState *const *states, const RunDesc *const *runs, const uint32_t *nruns, const uint32_t *reset)
{
    const uint32_t b = blockIdx.x;
    encode_stream<3, false, 3>(uni_ptr(states[b]), uni_ptr(runs[b]), UNI(nruns[b]), UNI(reset[b]), &g_ldsbt.base, &g_ldsbt.x);
}
#endif
// Lazy levels over a hash bucket of up to eight (levels 1 / 2): parser, coder and inserter wavefronts (csc_kernels_hp.inc)
__global__ __launch_bounds__(192) void k_encode_runs_hp(EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena)
{
    encode_stream<2, true, 4>(S, runs, nruns, reset_arena, &g_ldshp.base, &g_ldshp.x);
}
#ifndef CSCMI_DEV_ONE
__global__ __launch_bounds__(192)
void k_encode_runs_multi_hp(EncState *const *states, const RunDesc *const *runs, const uint32_t *nruns, const uint32_t *reset)
{
    const uint32_t b = blockIdx.x;
    encode_stream<2, true, 4>(uni_ptr(states[b]), uni_ptr(runs[b]), UNI(nruns[b]), UNI(reset[b]), &g_ldshp.base, &g_ldshp.x);
}
#endif
#endif
#if CSCMI_TU != 2
// The advanced parser over hash tables as ONE wavefront a stream, four streams a CU (FORM 5): launches of more streams than the pipeline form holds (more than
// 768: the 954-task split, the 2 048-task tree) and every configuration outside the level-3 geometry (level 4, custom props).  Round 6 retired the chain form
// (eight wavefronts) and the turn-taking forms (four wavefronts, 256-VGPR "dense" instance) that served such configurations at few
// streams: no BASELINE configuration reached them, their code objects were half of this file's build time.
__global__ __launch_bounds__(64)
void k_encode_runs_multi_one(EncState *const *states, const RunDesc *const *runs, const uint32_t *nruns, const uint32_t *reset)
{
    __shared__ EncLds lds;
    const uint32_t b = blockIdx.x;
    encode_stream<3, true, 5>(uni_ptr(states[b]), uni_ptr(runs[b]), UNI(nruns[b]), UNI(reset[b]), &lds);
}

// Level-3 geometry (bucket <= 2, good_len <= 16): the pipeline form of csc_kernels_dp4.inc -- spine, two edge wavefronts, inserter,
// two compare wavefronts, a service and a coder wavefront per stream (twelve launched, eight working: d4_role)
__global__ __launch_bounds__(64 * kD4Waves)
void k_encode_runs_dp4(EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena)
{
    encode_stream<3, true, 2>(S, runs, nruns, reset_arena, &g_lds4.base, &g_lds4.x);
}
#ifndef CSCMI_DEV_ONE
__global__ __launch_bounds__(64 * kD4Waves)
void k_encode_runs_multi_dp4(EncState *const *states, const RunDesc *const *runs, const uint32_t *nruns, const uint32_t *reset)
{
    const uint32_t b = blockIdx.x;
    encode_stream<3, true, 2>(uni_ptr(states[b]), uni_ptr(runs[b]), UNI(nruns[b]), UNI(reset[b]), &g_lds4.base, &g_lds4.x);
}
#endif

// ==========================================================================================
// k_init_state: Model::Reset (csc_model.cpp:88-111), Coder::Init (csc_coder.cpp:6-38)
__global__ void k_init_state(EncState *S)
{
    uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (uint32_t i = tid; i < 256 * 256; i += nth) S->p_lit[i] = 2048;
    for (uint32_t i = tid; i < P_COUNT; i += nth) S->probs[i] = 2048;
    if (tid == 0) {
        S->state = 0; S->ctx = 0; S->lp_rebuild_int = 0; S->p_delta_ready = 0;
        S->rc_low = 0; S->rc_range = 0xFFFFFFFFu; S->rc_cachesize = 1; S->rc_cache = 0;
        S->rc_size = S->bc_size = 0; S->bc_curbits = S->bc_curval = 0;
        S->arena_used = 0; S->error = 0;
        S->pos = S->vld_rge; S->bt_pos = 0; S->wnd_curpos = 0;   // MatchFinder::Init :56-58, LZ::Reset :45
        for (int k = 0; k < 4; k++) S->rep_dist[k] = S->wnd_size;
    }
}

// ==========================================================================================
// k_analyze: one workgroup per 8 KiB block.  Analyzer::Analyze + get_channel_idx + GetDltBpb
// (csc_analyzer.cpp:122-239).  All sums are exact u32 (wrap-around like the reference); the
// three floating-point thresholds are IEEE double products of host-supplied constants.
__device__ uint32_t block_sum(uint32_t v, uint32_t *scratch)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[w] = v;
    __syncthreads();
    uint32_t t = 0;
    for (uint32_t i = 0; i < (blockDim.x >> 6); i++) t += scratch[i];
    return t;
}

__device__ uint32_t dlt_bpb_block(const uint8_t *src, uint32_t size, uint32_t chn, uint32_t *freq, uint32_t *scratch)
{
    // GetDltBpb, csc_analyzer.cpp:166-182
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) freq[i] = 0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < size; j += blockDim.x) {
        uint32_t ch = j % chn, idx = j / chn, prev = 0;
        if (idx > 0) prev = src[j - chn];
        else if (ch > 0) {
            uint32_t nprev = (size - (ch - 1) + chn - 1) / chn;
            prev = src[(ch - 1) + (nprev - 1) * chn];
        }
        atomicAdd(&freq[(uint8_t)(src[j] - prev)], 1u);
    }
    __syncthreads();
    uint32_t term = 0;
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) term += freq[i] * d_logtable[freq[i] >> 4];
    uint32_t tot = block_sum(term, scratch);
    uint32_t bpb = size * d_logtable[size >> 4] - tot;
    return bpb / size;
}

__global__ __launch_bounds__(256) void k_analyze(EncState *S, uint32_t chunk_size, const double *ent_coef)
{
    __shared__ uint32_t freq[256];
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t verdict;
    const uint32_t blk = blockIdx.x;
    const uint8_t *src = S->inbuf + (size_t)blk * kMinBlock;
    uint32_t size = umin(kMinBlock, chunk_size - blk * kMinBlock);
    BlockInfo *out = S->binfo + blk;
    const uint32_t tid = threadIdx.x;

    if (size < 512) {   // DT_SKIP: the host may need GetDltBpb under the inherited type
        for (uint32_t k = 0; k < 5; k++) {
            uint32_t v = dlt_bpb_block(src, size, kDltIndex[k], freq, scratch);
            if (tid == 0) out->dlt_bpb[k] = v;
            __syncthreads();
        }
        if (tid == 0) { out->type = DT_SKIP; out->bpb = 0; }
        return;
    }
    freq[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < size; i += 256) atomicAdd(&freq[src[i]], 1u);
    __syncthreads();
    uint32_t f = freq[tid];
    uint32_t tot = block_sum(f * d_logtable[f >> 4], scratch);
    uint32_t diff_num = block_sum(f > 0 ? 1u : 0u, scratch);
    uint32_t hi = block_sum(tid >= 128 ? f : 0u, scratch);
    uint32_t alpha = block_sum((tid >= 'a' && tid <= 'z') ? f : 0u, scratch);
    uint32_t entropy = size * d_logtable[size >> 4] - tot;
    uint32_t bpb = entropy / size;
    uint32_t avg = size >> 8;
    if (tid == 0) {
        uint32_t t = 0;   // 0 = undecided -> channel test
        if (hi < (size >> 3) && (freq[' '] + freq['\n'] + freq[':'] + freq['.'] + freq['/'] > (size >> 4))
            && (freq['a'] + freq['e'] + freq['t'] > (size >> 4)) && entropy > 300 * size && alpha > (size / 3))
            t = DT_ENGTXT;
        else if (freq[0x8b] > avg && freq[0x00] > avg * 2 && freq[0xE8] > 6)
            t = DT_EXE;
        else if (diff_num < 16 && diff_num >= 6
                 && (double)entropy > ent_coef[diff_num - 6] * 100.0 * (double)size)
            t = DT_ENTROPY;
        else if (entropy < 400 * size && diff_num < 200)
            t = DT_NORMAL;
        verdict = t;
    }
    __syncthreads();
    uint32_t type = verdict;
    if (type == 0) {
        // get_channel_idx, csc_analyzer.cpp:122-164
        const uint32_t dk[5] = {1, 2, 3, 4, 8};
        uint32_t same[5] = {0, 0, 0, 0, 0}, succ[5] = {0, 0, 0, 0, 0};
        for (uint32_t i = tid; i + 16 < size; i += 256) {
            int a = src[i];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                int b = src[i + dk[k]];
                same[k] += (a == b);
                succ[k] += (uint32_t)(a > b ? a - b : b - a);
            }
        }
#pragma unroll
        for (int k = 0; k < 5; k++) { same[k] = block_sum(same[k], scratch); succ[k] = block_sum(succ[k], scratch); }
        uint32_t min_same = same[0], max_succ = succ[0], min_succ = succ[0], best = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (same[k] < min_same) min_same = same[k];
            if (succ[k] > max_succ) max_succ = succ[k];
            if (succ[k] < min_succ) { min_succ = succ[k]; best = k; }
        }
        uint32_t sb = succ[0], mb = same[0];
#pragma unroll
        for (int k = 0; k < 5; k++) if ((uint32_t)k == best) { sb = succ[k]; mb = same[k]; }
        bool dlt = ((max_succ > sb * 4) || (max_succ > sb + 40 * size)) && (mb > min_same * 3)
                   && ((double)same[0] < 0.3 * (double)size);
        if (dlt) type = DT_DLT + best;
        else if (entropy > 795 * size) type = DT_BAD;
        else if (entropy > 780 * size) type = DT_FAST;
        else type = DT_NORMAL;
    }
    if (type >= DT_DLT && type < DT_DLT + 5) {
        uint32_t v = dlt_bpb_block(src, size, kDltIndex[type - DT_DLT], freq, scratch);
        if (tid == 0) out->dlt_bpb[type - DT_DLT] = v;
    }
    if (tid == 0) { out->type = type; out->bpb = bpb; }
}

#ifdef CSCMI_STAGE_TEST
// Test-only (tests/stage/libcsc_stage.so, never in the product library): one forward filter over the chunk buffer, so that the
// filter kernels can be held against the reference's own outputs (tests/golden/stages.json) stage by stage.
__global__ __launch_bounds__(64) void k_stage_filter(EncState *S, uint32_t kind, uint32_t size, uint32_t chn, uint32_t *result)
{
    __shared__ EncLds lds;
    Sc c;
    sc_load(c, S, &lds);
    gu8 *src = (gu8 *)S->inbuf;
    uint32_t r = 0;
    if (kind == 0) flt_forward_e89(c, src, size);
    else if (kind == 1) r = flt_forward_dict(c, src, size);
    else flt_forward_delta(c, src, size, chn);
    wave_fence();
    if (c.lane == 0) *result = r;
}
#endif

#endif   // CSCMI_TU != 2

// ==========================================================================================
// host-callable launchers (csc_host.cpp keeps no HIP kernel syntax)
#if defined(CSCMI_DEV_ONE)
// (CSCMI_DEV_ONE == 3: the analysis build of the one-wavefront level-3 form, k_encode_runs_multi_one)
#else
#if CSCMI_TU != 1
// ---- the lazy levels and the binary-tree / wide-bucket configurations (the second code object where there are two): whatever the
// launchers below do not start themselves ends here, `kind` as they got it ----
void launch_encode_runs_multi_other(int kind, uint32_t nstreams, EncState *const *states, const RunDesc *const *runs,
                                    const uint32_t *nruns, const uint32_t *reset, hipStream_t st)
{
    // kind & 16: binary tree without a bucket under the advanced parser -- the inserter form (csc_kernels_bt.inc) while one workgroup a CU holds every stream
    if ((kind & 16) && nstreams <= kBtMultiMax) {
        hipLaunchKernelGGL(k_encode_runs_multi_bt, dim3(nstreams), dim3(256), 0, st, states, runs, nruns, reset);
        return;
    }
    // kind & 32: lazy parser over a bucket of up to eight -- parser + coder + inserter wavefronts while three workgroups a CU hold every stream
    if ((kind & 32) && nstreams <= kHpMultiMax) {
        hipLaunchKernelGGL(k_encode_runs_multi_hp, dim3(nstreams), dim3(192), 0, st, states, runs, nruns, reset);
        return;
    }
#ifndef CSCMI_DEV_M3ONLY
    switch (kind & 7) {
    case 2 | 4: hipLaunchKernelGGL((k_encode_runs_multi<2, true>), dim3(nstreams), dim3(128), 0, st, states, runs, nruns, reset); break;
    case 3: hipLaunchKernelGGL((k_encode_runs_multi<3, false>), dim3(nstreams), dim3(64), 0, st, states, runs, nruns, reset); break;
    default: hipLaunchKernelGGL((k_encode_runs_multi<2, false>), dim3(nstreams), dim3(128), 0, st, states, runs, nruns, reset); break;
    }
#endif
}
void launch_encode_runs_other(int kind, EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena, hipStream_t st)
{
    if (kind & 16) {
        hipLaunchKernelGGL(k_encode_runs_bt, dim3(1), dim3(256), 0, st, S, runs, nruns, reset_arena);
        return;
    }
    if (kind & 32) {
        hipLaunchKernelGGL(k_encode_runs_hp, dim3(1), dim3(192), 0, st, S, runs, nruns, reset_arena);
        return;
    }
#ifndef CSCMI_DEV_M3ONLY
    switch (kind & 7) {
    case 2 | 4: hipLaunchKernelGGL((k_encode_runs<2, true>), dim3(1), dim3(128), 0, st, S, runs, nruns, reset_arena); break;
    case 3: hipLaunchKernelGGL((k_encode_runs<3, false>), dim3(1), dim3(64), 0, st, S, runs, nruns, reset_arena); break;
    default: hipLaunchKernelGGL((k_encode_runs<2, false>), dim3(1), dim3(128), 0, st, S, runs, nruns, reset_arena); break;
    }
#endif
}
#endif
#if CSCMI_TU == 2
// (each code object has its own copy of the constant tables)
hipError_t upload_tables_other()
{
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(d_p2bits), kP2Bits, sizeof(kP2Bits));
    if (e != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(d_logtable), kLogTable, sizeof(kLogTable));
}
#else
#if CSCMI_TU == 1
hipError_t upload_tables_other();
void launch_encode_runs_multi_other(int kind, uint32_t nstreams, EncState *const *states, const RunDesc *const *runs,
                                    const uint32_t *nruns, const uint32_t *reset, hipStream_t st);
void launch_encode_runs_other(int kind, EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena, hipStream_t st);
#endif
hipError_t upload_tables()
{
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(d_p2bits), kP2Bits, sizeof(kP2Bits));
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(d_logtable), kLogTable, sizeof(kLogTable));
#if CSCMI_TU == 1
    if (e == hipSuccess) e = upload_tables_other();
#endif
    return e;
}
void launch_init_state(EncState *S, hipStream_t st) { hipLaunchKernelGGL(k_init_state, dim3(64), dim3(256), 0, st, S); }
void launch_analyze(EncState *S, uint32_t chunk_size, const double *ent_coef, hipStream_t st)
{
    uint32_t nblk = (chunk_size + kMinBlock - 1) / kMinBlock;
    hipLaunchKernelGGL(k_analyze, dim3(nblk), dim3(256), 0, st, S, chunk_size, ent_coef);
}
void launch_encode_runs_multi(int kind, uint32_t nstreams, EncState *const *states, const RunDesc *const *runs,
                              const uint32_t *nruns, const uint32_t *reset, hipStream_t st)
{
    // kind = parser (2 lazy/greedy, 3 advanced) | 4 if the configuration is hash-table-only | 8 if it has the level-3 geometry
    // (bucket <= 2, good_len <= 16): the pipeline form while one workgroup a CU holds every stream (~110 KiB of LDS each)
    // | 16 / | 32: see launch_encode_runs_multi_other.  csc_host.cpp sets 16 only without | 4 and 32 only with parser 2, so a kind of 3 | 4 never carries
    // either: the switch below may come before those tests
    // (Beyond 1024 streams not every stream is resident at once whatever the form: the hardware starts a waiting workgroup where one
    // ends -- the reference's hand-off of the next task to the worker that finishes, csarc.cpp:361-398.  Measured on the 2 048-task
    // tree: the one-wavefront form, 1 024 streams resident, 7.0 s; the pipeline form, 256 resident and each four times faster, 10.4 s.)
    uint32_t d4_max = kD4MultiMax;
#ifdef CSCMI_TIMERS
    if (const char *ev = getenv("CSCMI_D4_MULTI_MAX")) d4_max = (uint32_t)atoi(ev);      // development builds only: the pipeline form beyond one workgroup a CU (tools/gpu_many_streams.py)
#endif
    if (kind == (3 | 4 | 8) && nstreams <= d4_max) {
        hipLaunchKernelGGL(k_encode_runs_multi_dp4, dim3(nstreams), dim3(64 * kD4Waves), 0, st, states, runs, nruns, reset);
        return;
    }
    switch (kind & 7) {
    // (outside the level-3 geometry, or more streams than the pipeline form holds: one wavefront a stream)
    case 3 | 4: hipLaunchKernelGGL(k_encode_runs_multi_one, dim3(nstreams), dim3(64), 0, st, states, runs, nruns, reset); break;
    default: launch_encode_runs_multi_other(kind, nstreams, states, runs, nruns, reset, st); break;
    }
}
void launch_encode_eof(EncState *S, hipStream_t st) { hipLaunchKernelGGL(k_encode_eof, dim3(1), dim3(64), 0, st, S); }
#ifdef CSCMI_STAGE_TEST
void launch_stage_filter(EncState *S, uint32_t kind, uint32_t size, uint32_t chn, uint32_t *result, hipStream_t st)
{
    hipLaunchKernelGGL(k_stage_filter, dim3(1), dim3(64), 0, st, S, kind, size, chn, result);
}
#endif
void launch_encode_runs(int kind, EncState *S, const RunDesc *runs, uint32_t nruns, uint32_t reset_arena, hipStream_t st)
{
    if (kind == (3 | 4 | 8)) {
        hipLaunchKernelGGL(k_encode_runs_dp4, dim3(1), dim3(64 * kD4Waves), 0, st, S, runs, nruns, reset_arena);
        return;
    }
    switch (kind & 7) {      // (3 | 4 never carries | 16 or | 32: see launch_encode_runs_multi)
    case 3 | 4: hipLaunchKernelGGL((k_encode_runs<3, true>), dim3(1), dim3(64), 0, st, S, runs, nruns, reset_arena); break;
    default: launch_encode_runs_other(kind, S, runs, nruns, reset_arena, st); break;
    }
}
#endif   // CSCMI_TU == 2
#endif   // CSCMI_DEV_ONE
