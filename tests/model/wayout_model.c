/* CPU model of the way out's flag coding (csc_amd/csrc/csc_kernels_dp4.inc): a window's packets coded one after the other
 * (d6_literal / d6_rep0len1 / d6_rep_match / d6_match) against the lane arrangement of d6_chunk_lanes -- 64 packets at a
 * time, packet r in lane r, written the way the kernel is: per-lane arrays, ballots as 64-bit masks, counts below the lane,
 * rank chains resolved step by step through the predecessor's lane.  Both must leave the same P[], the same queue entries at
 * the same positions, the same tree records in the same order and the same state / context / queue head / statistics.
 *
 *   gcc -std=gnu99 -O2 -Wall -Wextra -Werror -o wayout_model wayout_model.c && ./wayout_model [seed [lists]]
 *
 * prints "wayout_model: ..." counter lines and WAYOUT_OK; exits 1 at the first difference. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { P_STATE = 0, P_REPDIST = 192, P_N = 384, RING = 128, MRING = 64, MAXP = 256, QCAP = MAXP * 24 + 64 };
enum { K_LIT = 0, K_MATCH = 1, K_REP0LEN1 = 2, K_REP = 3 };

typedef struct { uint32_t nd, len, last; } Packet;              /* nd: 0 literal, 1..4 rep index + 1, >= 5 distance + 5 (the DP's distance code) */
typedef struct {
    uint32_t P[P_N], state, ctx, q_head, st_lit, st_match;
    uint32_t q[QCAP];                                           /* 0 = a slot kept for a tree, not written here */
    uint32_t lt[MAXP], nlt, mt[MAXP][2], nmt;                   /* records in ring order (the rings' heads start at lt0 / mt0) */
} Model;

static uint32_t p_update(uint32_t bit, uint32_t p) { return bit ? p + ((0xFFFu - p) >> 5) : p - (p >> 5); }
static uint32_t clz32(uint32_t x) { return (uint32_t)__builtin_clz(x); }
static uint32_t dist_slot(uint32_t dist) { return dist < 3 ? dist : 33u - clz32(dist - 1); }
static uint32_t len_slots(uint32_t len) { return len < 8 ? 4u : len < 16 ? 5u : 9u; }

/* counters the test asserts on */
static struct {
    uint64_t lists, packets, chunks, carried_chunks, chain_steps, chains_ge8, mixed_chains, kinds[4], rep_idx[4], len_class[3], ndir[3], extra[32];
    uint32_t longest_chain;
} ST;

/* ---------------------------------------------------------------- one packet after the other ---------------------------------------------------------------- */
static void s_flags(Model *m, uint32_t nf, const uint32_t *idx, const uint32_t *bit)
{
    for (uint32_t k = 0; k < nf; k++) {
        const uint32_t p = m->P[idx[k]];
        m->P[idx[k]] = p_update(bit[k], p);
        m->q[m->q_head + k] = 0x80000000u | (bit[k] << 12) | p;
    }
    m->q_head += nf;
}
static void s_tree_record(Model *m, uint32_t w0, uint32_t w1, uint32_t nslots)
{
    m->mt[m->nmt][0] = w0 | (m->q_head << 16); m->mt[m->nmt][1] = w1; m->nmt++;
    m->q_head += nslots;
}
static void serial(Model *m, const Packet *pk, uint32_t n)
{
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t s3 = m->state * 3, nd = pk[r].nd, len = pk[r].len;
        uint32_t idx[5], bit[5];
        if (nd == 0) {                                                             /* d6_literal */
            idx[0] = P_STATE + s3; bit[0] = 0;
            const uint32_t at = m->q_head;
            s_flags(m, 1, idx, bit);
            m->lt[m->nlt++] = m->ctx | (pk[r].last << 8) | (at << 16);
            m->q_head += 8;
            m->state = (m->state * 4) & 0x3F; m->st_lit++;
        } else if (nd <= 4 && nd == 1 && len == 1) {                               /* d6_rep0len1 */
            for (uint32_t k = 0; k < 3; k++) { idx[k] = P_STATE + s3 + k; bit[k] = k == 0; }
            s_flags(m, 3, idx, bit);
            m->state = (m->state * 4 + 2) & 0x3F; m->st_match++;
        } else if (nd <= 4) {                                                      /* d6_rep_match */
            const uint32_t rep_idx = nd - 1;
            for (uint32_t k = 0; k < 5; k++) {
                idx[k] = k < 3 ? P_STATE + s3 + k : P_REPDIST + s3 - 1u + (k == 3 ? 1u : 2u | (rep_idx >> 1));
                bit[k] = k < 3 ? (0x5u >> k) & 1u : (rep_idx >> ((4u - k) & 1u)) & 1u;
            }
            s_flags(m, 5, idx, bit);
            s_tree_record(m, 1u | ((len - 2) << 1), 0, len_slots(len - 2));
            m->state = (m->state * 4 + 3) & 0x3F; m->st_match++;
        } else {                                                                   /* d6_match */
            const uint32_t dist = nd - 5, l2 = len - 2;
            idx[0] = P_STATE + s3; idx[1] = P_STATE + s3 + 1; bit[0] = bit[1] = 1;
            s_flags(m, 2, idx, bit);
            const uint32_t sbits = l2 == 0 ? 3u : l2 <= 2 ? 4u : 5u;
            const uint32_t slot = dist_slot(dist), extra_bits = slot > 2 ? slot - 2 : 0;
            const uint32_t ndir = extra_bits > 4 ? (extra_bits - 4 > 16 ? 2u : 1u) : 0u;
            s_tree_record(m, l2 << 1, dist, len_slots(l2) + sbits + ndir + (extra_bits ? 4u : 0u));
            m->state = (m->state * 4 + 1) & 0x3F; m->st_match++;
            ST.ndir[ndir]++; ST.extra[extra_bits]++;
        }
        m->ctx = pk[r].last;
    }
}

/* ---------------------------------------------------------------- 64 packets in lanes ---------------------------------------------------------------- */
#define LANES 64
static uint32_t below(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }      /* v_mbcnt */

static uint32_t chunk_shape(uint32_t nd, uint32_t ql, int on)                     /* d6_chunk_shape */
{
    const uint32_t len = ql & 0xFFFFu;
    const uint32_t kind = nd == 0 ? 0u : nd > 4 ? 1u : (nd == 1 && len == 1) ? 2u : 3u;
    const uint32_t l2 = len - 2u, dist = nd - 5u;
    const uint32_t sbits = l2 == 0 ? 3u : l2 <= 2 ? 4u : 5u;
    const uint32_t slot = dist < 3 ? dist : 33u - (dist - 1 ? clz32(dist - 1) : 32u), extra_bits = slot > 2 ? slot - 2 : 0;
    const uint32_t ndir = extra_bits > 4 ? (extra_bits - 4 > 16 ? 2u : 1u) : 0u;
    const uint32_t nf = kind == 0 ? 1u : kind == 1 ? 2u : kind == 2 ? 3u : 5u;
    const uint32_t tree = kind == 0 ? 8u : kind == 2 ? 0u : len_slots(l2) + (kind == 1 ? sbits + ndir + (extra_bits ? 4u : 0u) : 0u);
    return on ? kind | (nf << 2) | ((nf + tree) << 8) : 0u;
}
/* one decision of every lane that has it (d6_chunk_flag) */
static void chunk_flag(Model *m, const int *act, const uint32_t *idx, const uint32_t *bit, const uint32_t *qslot, const uint64_t *same_in)
{
    uint64_t am = 0;
    for (uint32_t l = 0; l < LANES; l++) if (act[l]) am |= 1ull << l;
    if (!am) return;
    uint32_t rank[LANES], prev[LANES], pold[LANES], pnew[LANES];
    uint64_t above[LANES];
    for (uint32_t l = 0; l < LANES; l++) {
        const uint64_t same = same_in[l] & am, bl = same & ((1ull << l) - 1ull);
        above[l] = (same >> l) >> 1;
        rank[l] = (uint32_t)__builtin_popcountll(bl);
        prev[l] = bl ? 63u - (uint32_t)__builtin_clzll(bl) : l;
        pold[l] = act[l] ? m->P[idx[l]] : 0;                                    /* the gather: every lane reads before any lane stores */
        pnew[l] = p_update(bit[l], pold[l]);
        if (act[l] && !above[l]) {                                              /* the chain's last lane: what kind of chain was it? */
            const uint32_t n = rank[l] + 1;
            uint32_t ones = 0;
            for (uint32_t j = 0; j < LANES; j++) if ((same >> j) & 1) ones += bit[j];
            if (n > ST.longest_chain) ST.longest_chain = n;
            if (n >= 8) ST.chains_ge8++;
            if (ones != 0 && ones != n) ST.mixed_chains++;
        }
    }
    for (uint32_t d = 1;; d++) {
        int any = 0;
        for (uint32_t l = 0; l < LANES; l++) any |= act[l] && rank[l] >= d;
        if (!any) break;
        uint32_t v[LANES];
        for (uint32_t l = 0; l < LANES; l++) v[l] = pnew[prev[l]];              /* ds_bpermute: all lanes read, then all lanes write */
        for (uint32_t l = 0; l < LANES; l++) if (act[l] && rank[l] == d) { pold[l] = v[l]; pnew[l] = p_update(bit[l], pold[l]); }
        ST.chain_steps++;
    }
    for (uint32_t l = 0; l < LANES; l++) {
        if (act[l] && !above[l]) m->P[idx[l]] = pnew[l];
        if (act[l]) m->q[qslot[l]] = 0x80000000u | (bit[l] << 12) | pold[l];
    }
}
static void lanes_chunk(Model *m, const Packet *pk, uint32_t n)                   /* the master's chunk set-up + d6_chunk_lanes */
{
    uint32_t nd[LANES], ql[LANES], shape[LANES], qpos[LANES], kind[LANES], nf[LANES], state[LANES], ctx[LANES];
    int on[LANES];
    for (uint32_t l = 0; l < LANES; l++) {
        on[l] = l < n;
        nd[l] = on[l] ? pk[l].nd : 0xDEAD0000u + l * 977u;                      /* lanes past the chunk hold whatever the log holds */
        ql[l] = on[l] ? pk[l].len | (pk[l].last << 16) : 0xBEEF0000u ^ (l * 7919u);
        shape[l] = chunk_shape(nd[l], ql[l], on[l]);
        kind[l] = shape[l] & 3u; nf[l] = (shape[l] >> 2) & 7u;
    }
    /* queue offsets: five bit planes of the slot counts, counted below the lane and in all */
    uint32_t need = 0, qoff[LANES] = {0};
    for (uint32_t b = 0; b < 5; b++) {
        uint64_t pm = 0;
        for (uint32_t l = 0; l < LANES; l++) if ((shape[l] >> (8 + b)) & 1u) pm |= 1ull << l;
        for (uint32_t l = 0; l < LANES; l++) qoff[l] += below(pm, l) << b;
        need += (uint32_t)__builtin_popcountll(pm) << b;
    }
    for (uint32_t l = 0; l < LANES; l++) { if ((shape[l] >> 8) >= 32) abort(); qpos[l] = m->q_head + qoff[l]; }
    /* states: bit planes of the kinds, the incoming state's three kinds in front */
    const uint32_t s0 = m->state;
    uint64_t b0 = 0, b1 = 0, lm = 0, tm = 0;
    for (uint32_t l = 0; l < LANES; l++) {
        if (on[l] && (kind[l] & 1u)) b0 |= 1ull << l;
        if (on[l] && (kind[l] & 2u)) b1 |= 1ull << l;
        if (on[l] && kind[l] == 0) lm |= 1ull << l;
        if (on[l] && (kind[l] & 1u)) tm |= 1ull << l;
    }
    const uint64_t h0 = (b0 << 3) | ((s0 & 1u) << 2) | (((s0 >> 2) & 1u) << 1) | ((s0 >> 4) & 1u);
    const uint64_t h1 = (b1 << 3) | (((s0 >> 1) & 1u) << 2) | (((s0 >> 3) & 1u) << 1) | ((s0 >> 5) & 1u);
    for (uint32_t l = 0; l < LANES; l++) {
        const uint32_t a = (uint32_t)(l >= 3 ? b0 >> (l - 3) : h0 >> l) & 7u, b = (uint32_t)(l >= 3 ? b1 >> (l - 3) : h1 >> l) & 7u;      /* bit 2: packet l - 1, bit 0: l - 3 */
        state[l] = ((a >> 2) & 1u) | (((b >> 2) & 1u) << 1) | (((a >> 1) & 1u) << 2) | (((b >> 1) & 1u) << 3) | ((a & 1u) << 4) | ((b & 1u) << 5);
        ctx[l] = l == 0 ? m->ctx : ql[l - 1] >> 16;
    }
    /* records, each ring's count once */
    for (uint32_t l = 0; l < LANES; l++) {
        if (on[l] && kind[l] == 0) m->lt[m->nlt + below(lm, l)] = ctx[l] | ((ql[l] >> 16) << 8) | (qpos[l] << 16);
        if (on[l] && (kind[l] & 1u)) {
            const uint32_t r = m->nmt + below(tm, l);
            m->mt[r][0] = (kind[l] == 3 ? 1u : 0u) | (((ql[l] & 0xFFFFu) - 2u) << 1) | ((qpos[l] + nf[l]) << 16);
            m->mt[r][1] = kind[l] == 1 ? nd[l] - 5u : 0u;
        }
    }
    m->nlt += (uint32_t)__builtin_popcountll(lm); m->nmt += (uint32_t)__builtin_popcountll(tm);
    /* the lanes that stand in this lane's state: one round per distinct state */
    uint64_t same[LANES] = {0}, rem = 0;
    for (uint32_t l = 0; l < LANES; l++) if (on[l]) rem |= 1ull << l;
    while (rem) {
        const uint32_t sv = state[__builtin_ctzll(rem)];
        uint64_t mm = 0;
        for (uint32_t l = 0; l < LANES; l++) if (on[l] && state[l] == sv) mm |= 1ull << l;
        for (uint32_t l = 0; l < LANES; l++) if (state[l] == sv) same[l] = mm;
        rem &= ~mm;
    }
    /* decisions 0..4 */
    int act[LANES]; uint32_t idx[LANES], bit[LANES], qs[LANES]; uint64_t sm[LANES];
    for (uint32_t k = 0; k < 5; k++) {
        uint64_t hi = 0;
        for (uint32_t l = 0; l < LANES; l++) if (on[l] && kind[l] == 3 && (((nd[l] - 1u) >> 1) & 1u)) hi |= 1ull << l;
        for (uint32_t l = 0; l < LANES; l++) {
            const uint32_t s3 = state[l] * 3u, rep_hi = ((nd[l] - 1u) >> 1) & 1u;
            qs[l] = qpos[l] + k; sm[l] = same[l];
            switch (k) {
            case 0: act[l] = on[l]; idx[l] = P_STATE + s3; bit[l] = kind[l] != 0; break;
            case 1: act[l] = on[l] && kind[l] != 0; idx[l] = P_STATE + s3 + 1; bit[l] = kind[l] == 1; break;
            case 2: act[l] = on[l] && kind[l] >= 2; idx[l] = P_STATE + s3 + 2; bit[l] = kind[l] == 3; break;
            case 3: act[l] = on[l] && kind[l] == 3; idx[l] = P_REPDIST + s3; bit[l] = rep_hi; break;
            default: act[l] = on[l] && kind[l] == 3; idx[l] = P_REPDIST + s3 + 1 + rep_hi; bit[l] = (nd[l] - 1u) & 1u; sm[l] = same[l] & (rep_hi ? hi : ~hi); break;
            }
        }
        chunk_flag(m, act, idx, bit, qs, sm);
    }
    /* behind the chunk */
    ST.chunks++;
    m->state = (state[n - 1] * 4 + kind[n - 1]) & 0x3F; m->ctx = ql[n - 1] >> 16;
    m->q_head += need;
    m->st_lit += (uint32_t)__builtin_popcountll(lm); m->st_match += n - (uint32_t)__builtin_popcountll(lm);
}
static void lanes(Model *m, const Packet *pk, uint32_t n)
{
    for (uint32_t at = 0; at < n; at += LANES) {
        if (at && m->state != 0) ST.carried_chunks++;                            /* a later chunk entered with a state the chunk before left */
        lanes_chunk(m, pk + at, n - at < LANES ? n - at : LANES);
    }
}

/* ---------------------------------------------------------------- driver ---------------------------------------------------------------- */
static uint64_t rng_s;
static uint32_t rnd(void) { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)(rng_s >> 16); }

static void run_list(const Packet *pk, uint32_t n, const char *what)
{
    static Model a, b;
    memset(&a, 0, sizeof a);
    for (uint32_t i = 0; i < P_N; i++) a.P[i] = 31 + rnd() % 4035;               /* any probability the coder can hold */
    a.state = rnd() & 0x3F; a.ctx = rnd() & 0xFF; a.q_head = 0;
    b = a;
    serial(&a, pk, n);
    lanes(&b, pk, n);
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t k = pk[r].nd == 0 ? 0 : pk[r].nd > 4 ? 1 : (pk[r].nd == 1 && pk[r].len == 1) ? 2 : 3;
        ST.kinds[k]++;
        if (k == 3) ST.rep_idx[pk[r].nd - 1]++;
        if (k == 1 || k == 3) { const uint32_t c = len_slots(pk[r].len - 2); ST.len_class[c == 4 ? 0 : c == 5 ? 1 : 2]++; }
    }
    ST.lists++; ST.packets += n;
    const char *bad = NULL;
    if (memcmp(a.P, b.P, sizeof a.P)) bad = "P[]";
    else if (a.q_head != b.q_head) bad = "q_head";
    else if (memcmp(a.q, b.q, sizeof a.q)) bad = "queue entries";
    else if (a.nlt != b.nlt || memcmp(a.lt, b.lt, sizeof a.lt)) bad = "lt_rec";
    else if (a.nmt != b.nmt || memcmp(a.mt, b.mt, sizeof a.mt)) bad = "mt_rec";
    else if (a.state != b.state) bad = "state";
    else if (a.ctx != b.ctx) bad = "ctx";
    else if (a.st_lit != b.st_lit || a.st_match != b.st_match) bad = "statistics";
    if (bad) { printf("wayout_model: %s differ (%s, %u packets)\n", bad, what, n); exit(1); }
}
static Packet lit(void) { Packet p = {0, 1, rnd() & 0xFF}; return p; }
static Packet rep0len1(void) { Packet p = {1, 1, rnd() & 0xFF}; return p; }
static Packet rep(uint32_t idx, uint32_t len) { Packet p = {idx + 1, len, rnd() & 0xFF}; return p; }
static Packet match(uint32_t dist, uint32_t len) { Packet p = {dist + 5, len, rnd() & 0xFF}; return p; }
static Packet any(uint32_t lit_pct)
{
    const uint32_t r = rnd() % 100;
    if (r < lit_pct) return lit();
    const uint32_t k = rnd() % 10, len = 2 + rnd() % (rnd() % 8 ? 16 : 60);
    if (k < 1) return rep0len1();
    if (k < 5) return rep(rnd() & 3, len);
    return match((rnd() & 0x7FFFFFFu) >> (rnd() % 26), len);
}

int main(int argc, char **argv)
{
    rng_s = (argc > 1 ? strtoull(argv[1], NULL, 0) : 20240607ull) * 0x9E3779B97F4A7C15ull + 1;
    const uint32_t lists = argc > 2 ? (uint32_t)atoi(argv[2]) : 4000;
    static Packet pk[MAXP];
    for (uint32_t i = 0; i < lists; i++) {                                         /* seeded random lists of 1..200 packets, literal share 0..100 % */
        const uint32_t n = 1 + rnd() % 200, pct = (i % 11) * 10;
        for (uint32_t r = 0; r < n; r++) pk[r] = any(pct);
        run_list(pk, n, "random");
    }
    const uint32_t sizes[] = {63, 64, 65, 128, 200};
    for (uint32_t s = 0; s < 5; s++) {
        const uint32_t n = sizes[s];
        for (uint32_t r = 0; r < n; r++) pk[r] = lit();
        run_list(pk, n, "all literals");
        for (uint32_t r = 0; r < n; r++) pk[r] = r & 1 ? rep0len1() : lit();
        run_list(pk, n, "literal / rep0len1");
        for (uint32_t r = 0; r < n; r++) pk[r] = rep(r & 3, 2 + r % 16);
        run_list(pk, n, "rep indices 0..3, lengths 2..17");
        for (uint32_t r = 0; r < n; r++) pk[r] = rep((r >> 1) & 3, 2 + r % 40);
        run_list(pk, n, "rep indices in pairs, every length class");
        for (uint32_t r = 0; r < n; r++) pk[r] = match(1 + r * 37, 2 + r % 16);
        run_list(pk, n, "matches, lengths 2..17");
        for (uint32_t r = 0; r < n; r++) pk[r] = any(50);
        run_list(pk, n, "mixed");
    }
    {   /* distances on both sides of extra_bits 0, 4, 5, 20, 21 (direct bits in 0, 1 and 2 pieces) */
        const uint32_t e[] = {0, 1, 3, 4, 5, 6, 19, 20, 21, 22};
        uint32_t n = 0;
        pk[n++] = match(0, 2); pk[n++] = match(1, 3); pk[n++] = match(2, 5);
        for (uint32_t i = 0; i < 10; i++) { pk[n++] = match((1u << e[i]) + 1, 2 + i); pk[n++] = match(1u << e[i], 9 + i); pk[n++] = match((2u << e[i]), 18 + i); pk[n++] = lit(); }
        run_list(pk, n, "distance classes");
    }
    printf("wayout_model: lists %llu packets %llu chunks %llu chunks entered with a carried state %llu\n",
           (unsigned long long)ST.lists, (unsigned long long)ST.packets, (unsigned long long)ST.chunks, (unsigned long long)ST.carried_chunks);
    printf("wayout_model: chains longest %u of length >= 8 %llu with both bits %llu chain steps %llu\n",
           ST.longest_chain, (unsigned long long)ST.chains_ge8, (unsigned long long)ST.mixed_chains, (unsigned long long)ST.chain_steps);
    printf("wayout_model: kinds literal %llu match %llu rep0len1 %llu rep %llu rep indices %llu %llu %llu %llu\n",
           (unsigned long long)ST.kinds[0], (unsigned long long)ST.kinds[1], (unsigned long long)ST.kinds[2], (unsigned long long)ST.kinds[3],
           (unsigned long long)ST.rep_idx[0], (unsigned long long)ST.rep_idx[1], (unsigned long long)ST.rep_idx[2], (unsigned long long)ST.rep_idx[3]);
    printf("wayout_model: length classes %llu %llu %llu direct pieces %llu %llu %llu extra bits",
           (unsigned long long)ST.len_class[0], (unsigned long long)ST.len_class[1], (unsigned long long)ST.len_class[2],
           (unsigned long long)ST.ndir[0], (unsigned long long)ST.ndir[1], (unsigned long long)ST.ndir[2]);
    for (uint32_t i = 0; i < 32; i++) if (ST.extra[i]) printf(" %u", i);
    printf("\nWAYOUT_OK\n");
    return 0;
}
