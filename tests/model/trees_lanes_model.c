/* CPU model of the tree wavefront's match / rep pass (d6_trees, csc_amd/csrc/csc_kernels_dp4.inc): the records of the ring coded one
 * after the other (dec_matchlen_1, the distance slot's tree, the direct bits, the low nibble's tree -- the order of Model::EncodeMatch)
 * against the pass that takes up to four records at a time, written the way the kernel is: per-lane arrays, record i of the pass in
 * lanes 16 i .. 16 i + 15 (32 lanes a record when one of them has more than 14 decisions), the lane of an earlier record on the same
 * cell found by arithmetic on that record (d6_rec_lane), chains resolved round by round through the predecessor's lane, one gather,
 * one scatter, one store into the queue.  Both must leave the same P[] and the same queue entries at the same positions.
 *
 *   gcc -std=gnu99 -O2 -Wall -Wextra -Werror -o trees_lanes_model trees_lanes_model.c && ./trees_lanes_model [seed [lists]]
 *
 * prints "trees_lanes_model: ..." counter lines and TREES_LANES_OK; exits 1 at the first difference. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* csc_device.h's layout of the small tables */
enum { P_STATE = 0, P_REPDIST = 192, P_DIST = 384, P_LEN_SLOT = 552, P_LEN_X1 = 554, P_LEN_X2 = 562, P_LEN_X3 = 570, P_DIST_EXTRA = 698,
       P_COUNT = 698 + 464 + 2, P_DUMP = P_COUNT + 3, P_N = P_COUNT + 4 };
enum { MRING = 64, QCAP = 4096, LANES = 64, MAXR = 512, NONE = 0xFF };

typedef struct { uint32_t w0, dist; } Rec;                      /* mt_rec: kind (0 match, 1 rep) | length - 2 << 1 | first kept queue slot << 16, distance */
typedef struct { uint32_t P[P_N], q[QCAP + 1]; } Model;         /* q[QCAP]: the queue's spare word; 0 = never written */

static uint32_t p_update(uint32_t bit, uint32_t p) { return bit ? p + ((0xFFFu - p) >> 5) : p - (p >> 5); }
static uint32_t clz32(uint32_t x) { return x ? (uint32_t)__builtin_clz(x) : 32u; }
static uint32_t dist_slot(uint32_t dist) { return dist < 3 ? dist : 33u - clz32(dist - 1); }
static uint32_t brev4(uint32_t x) { return ((x & 1u) << 3) | ((x & 2u) << 1) | ((x & 4u) >> 1) | ((x & 8u) >> 3); }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

static struct {
    uint64_t lists, records, passes[5], wide_passes, chain_rounds, chained[4], stores_left_to_later;
    uint64_t four_same, four_same_full_chain, pdist_three_offsets, rep_between_matches, extra_class[4], ndir[3];
    uint64_t nine_first, nine_last, nine_mid, ring_cross, len_class[3];
} ST;

/* ---------------------------------------------------------------- one record after the other ---------------------------------------------------------------- */
static void s_bit(Model *m, uint32_t *at, uint32_t idx, uint32_t bit)
{
    const uint32_t p = m->P[idx];
    m->P[idx] = p_update(bit, p);
    m->q[(*at)++ & (QCAP - 1)] = 0x80000000u | (bit << 12) | p;
}
static void s_tree(Model *m, uint32_t *at, uint32_t base, uint32_t x, uint32_t nb)
{
    uint32_t node = 1;
    for (uint32_t j = 0; j < nb; j++) { const uint32_t b = (x >> (nb - 1 - j)) & 1u; s_bit(m, at, base + node, b); node = node * 2 + b; }
}
static void serial(Model *m, Rec r)
{
    uint32_t at = r.w0 >> 16;
    const uint32_t len = (r.w0 >> 1) & 0xFFu, dist = r.dist;
    if (len < 8) { s_bit(m, &at, P_LEN_SLOT, 0); s_tree(m, &at, P_LEN_X1, len, 3); }
    else if (len < 16) { s_bit(m, &at, P_LEN_SLOT, 1); s_bit(m, &at, P_LEN_SLOT + 1, 0); s_tree(m, &at, P_LEN_X2, len - 8, 3); }
    else { s_bit(m, &at, P_LEN_SLOT, 1); s_bit(m, &at, P_LEN_SLOT + 1, 1); s_tree(m, &at, P_LEN_X3, len - 16, 7); }
    if (r.w0 & 1u) return;
    uint32_t pdist_pos, sbits;
    if (len == 0) { pdist_pos = 0; sbits = 3; }
    else if (len <= 2) { pdist_pos = 16 * (len - 1) + 8; sbits = 4; }
    else if (len <= 5) { pdist_pos = 32 * (len - 3) + 8 + 16 * 2; sbits = 5; }
    else { pdist_pos = 32 * 3 + 8 + 16 * 2; sbits = 5; }
    const uint32_t slot = dist_slot(dist), extra_bits = slot > 2 ? slot - 2 : 0;
    s_tree(m, &at, P_DIST + pdist_pos, slot, sbits);
    if (!extra_bits) return;
    const uint32_t extra_len = dist - (1u << extra_bits) - 1;
    if (extra_bits > 4) {                                                           /* EncodeDirect in pieces of <= 16 bits */
        const uint32_t v = extra_len >> 4, l = extra_bits - 4;
        if (l <= 16) m->q[at++ & (QCAP - 1)] = 0x40000000u | (l << 16) | (v & 0xFFFFu);
        else { m->q[at++ & (QCAP - 1)] = 0x40000000u | ((l - 16) << 16) | ((v >> 16) & 0xFFFFu); m->q[at++ & (QCAP - 1)] = 0x40000000u | (16u << 16) | (v & 0xFFFFu); }
    }
    s_tree(m, &at, P_DIST_EXTRA + (extra_bits - 1) * 16, brev4(extra_len & 0x0Fu), 4);
}

/* ---------------------------------------------------------------- up to four records in lanes ---------------------------------------------------------------- */
typedef struct { uint32_t len, k0[3], nb[3], x[3], base[3], n, n_head, ndir, dir0, dir1; } D6Rec;
static D6Rec d6_rec(uint32_t w0, uint32_t dist)
{
    D6Rec r;
    const uint32_t len = (w0 >> 1) & 0xFFu;
    r.len = len;
    r.k0[0] = len < 8 ? 1u : 2u; r.nb[0] = len < 16 ? 3u : 7u; r.x[0] = len < 8 ? len : len < 16 ? len - 8u : len - 16u;
    r.base[0] = len < 8 ? P_LEN_X1 : len < 16 ? P_LEN_X2 : P_LEN_X3;
    uint32_t n = r.k0[0] + r.nb[0];
    const int match = (w0 & 1u) == 0;
    const uint32_t sbits = len == 0 ? 3u : len <= 2 ? 4u : 5u;
    const uint32_t pdist_pos = len == 0 ? 0u : len <= 2 ? 16u * (len - 1u) + 8u : 32u * (umin(len, 6u) - 3u) + 8u + 16u * 2u;
    const uint32_t slot = dist_slot(dist), extra_bits = match && slot > 2 ? slot - 2u : 0u;
    r.k0[1] = n; r.nb[1] = match ? sbits : 0u; r.x[1] = slot; r.base[1] = P_DIST + pdist_pos;
    n += r.nb[1];
    r.n_head = n;
    const uint32_t extra_len = dist - (1u << (extra_bits & 31u)) - 1u;
    r.k0[2] = n; r.nb[2] = extra_bits ? 4u : 0u; r.x[2] = brev4(extra_len & 0x0Fu); r.base[2] = P_DIST_EXTRA + (extra_bits - 1u) * 16u;
    n += r.nb[2];
    r.n = n;
    const uint32_t v = extra_len >> 4, l = extra_bits - 4u;
    r.ndir = extra_bits > 4 ? (l > 16 ? 2u : 1u) : 0u;
    r.dir0 = l <= 16 ? (l << 16) | (v & 0xFFFFu) : ((l - 16u) << 16) | ((v >> 16) & 0xFFFFu);
    r.dir1 = (16u << 16) | (v & 0xFFFFu);
    return r;
}
static void d6_rec_cell(const D6Rec *r, uint32_t k, uint32_t *idx, uint32_t *bit)
{
    *idx = P_LEN_SLOT; *bit = r->len >= 8;
    if (k == 1 && r->len >= 8) { *idx = P_LEN_SLOT + 1; *bit = r->len >= 16; }
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t l = k - r->k0[s];
        if (l < r->nb[s]) { *idx = r->base[s] + ((1u << l) | (r->x[s] >> ((r->nb[s] - l) & 31u))); *bit = (r->x[s] >> ((r->nb[s] - 1u - l) & 31u)) & 1u; }
    }
}
static uint32_t d6_rec_lane(const D6Rec *r, uint32_t idx)
{
    uint32_t k = NONE;
    if (idx == P_LEN_SLOT) k = 0;
    if (idx == P_LEN_SLOT + 1 && r->len >= 8) k = 1;
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t node = idx - r->base[s];
        const uint32_t l = 31u - clz32(node | 1u);
        if (node >= 1u && node < (1u << r->nb[s]) && node == ((1u << l) | (r->x[s] >> ((r->nb[s] - l) & 31u)))) k = r->k0[s] + l;
    }
    return k;
}
/* one pass over the records ring[mdone ..] of which `avail` are written; -> records taken */
static uint32_t lanes_pass(Model *m, const Rec *ring, uint32_t mdone, uint32_t avail)
{
    uint32_t n = umin(avail, 4u), sh = 4;
    uint32_t w0[LANES], dist[LANES];
    D6Rec R[LANES];
    int wide = 0;
    for (uint32_t l = 0; l < LANES; l++) {
        w0[l] = ring[(mdone + (l >> 4)) & (MRING - 1)].w0; dist[l] = ring[(mdone + (l >> 4)) & (MRING - 1)].dist;
        R[l] = d6_rec(w0[l], dist[l]);
        wide |= (l >> 4) < n && R[l].n > 14u;
    }
    if (wide) {
        sh = 5; n = umin(n, 2u);
        for (uint32_t l = 0; l < LANES; l++) {
            w0[l] = ring[(mdone + (l >> 5)) & (MRING - 1)].w0; dist[l] = ring[(mdone + (l >> 5)) & (MRING - 1)].dist;
            R[l] = d6_rec(w0[l], dist[l]);
        }
        ST.wide_passes++;
    }
    const uint32_t S = 1u << sh;
    uint32_t idx[LANES], bit[LANES], pold[LANES], pnew[LANES], prev[LANES], rank[LANES];
    int on[LANES], later[LANES];
    for (uint32_t l = 0; l < LANES; l++) {
        const uint32_t i = l >> sh, k = l & (S - 1u);
        on[l] = i < n && k < R[l].n;
        d6_rec_cell(&R[l], k, &idx[l], &bit[l]);
        idx[l] = on[l] ? idx[l] : 0xFFFFFFFFu;
    }
    for (uint32_t l = 0; l < LANES; l++) pold[l] = m->P[on[l] ? idx[l] : P_DUMP];       /* the gather: every lane reads before any lane stores */
    for (uint32_t l = 0; l < LANES; l++) { prev[l] = l; rank[l] = 0; later[l] = 0; }
    if (n > 1)
        for (uint32_t j = 0; j < 4 && j < n; j++) {
            const D6Rec Rj = d6_rec(w0[j << sh], dist[j << sh]);                     /* v_readlane: uniform */
            for (uint32_t l = 0; l < LANES; l++) {
                const uint32_t i = l >> sh, kj = d6_rec_lane(&Rj, idx[l]);
                const int hit = kj != NONE;
                if (hit && j < i) { prev[l] = (j << sh) + kj; rank[l]++; }
                later[l] = later[l] || (hit && j > i);
            }
        }
    for (uint32_t l = 0; l < LANES; l++) pnew[l] = p_update(bit[l], pold[l]);
    for (uint32_t d = 1; d < n; d++) {
        int any = 0;
        for (uint32_t l = 0; l < LANES; l++) any |= rank[l] >= d;
        if (!any) break;
        uint32_t v[LANES];
        for (uint32_t l = 0; l < LANES; l++) v[l] = pnew[prev[l]];                  /* ds_bpermute: all lanes read, then all lanes write */
        for (uint32_t l = 0; l < LANES; l++) if (rank[l] == d) { pold[l] = v[l]; pnew[l] = p_update(bit[l], pold[l]); }
        ST.chain_rounds++;
    }
    for (uint32_t l = 0; l < LANES; l++) m->P[on[l] && !later[l] ? idx[l] : P_DUMP] = pnew[l];
    for (uint32_t l = 0; l < LANES; l++)                                            /* a scatter has no order among its lanes: one storing lane a cell */
        for (uint32_t o = 0; o < l; o++)
            if (on[l] && !later[l] && on[o] && !later[o] && idx[l] == idx[o]) { printf("trees_lanes_model: lanes %u and %u store to one cell\n", o, l); exit(1); }
    for (uint32_t l = 0; l < LANES; l++) {
        const uint32_t i = l >> sh, k = l & (S - 1u), qpos = w0[l] >> 16;
        const uint32_t kd = k - (S - 2u);
        const int dir = i < n && kd < R[l].ndir;
        const uint32_t at = dir ? qpos + R[l].n_head + kd : qpos + k + (k >= R[l].n_head ? R[l].ndir : 0u);
        m->q[on[l] || dir ? at & (QCAP - 1) : QCAP] = dir ? 0x40000000u | (kd ? R[l].dir1 : R[l].dir0) : 0x80000000u | (bit[l] << 12) | pold[l];
    }
    /* ---- what this pass was: counters for the test ---- */
    ST.passes[n]++;
    if ((mdone & (MRING - 1)) + n > MRING) ST.ring_cross++;
    {
        const D6Rec *r[4];
        uint32_t kind[4];
        for (uint32_t i = 0; i < n; i++) { r[i] = &R[i << sh]; kind[i] = w0[i << sh] & 1u; }
        for (uint32_t i = 0; i < n; i++) {
            if (r[i]->len >= 16) { if (i == 0) ST.nine_first++; if (i == n - 1) ST.nine_last++; if (i > 0 && i < n - 1) ST.nine_mid++; }
            if (i > 0 && i < n - 1 && kind[i] == 1 && kind[i - 1] == 0 && kind[i + 1] == 0) ST.rep_between_matches++;
        }
        for (uint32_t l = 0; l < LANES; l++) if (on[l]) { ST.chained[rank[l]]++; if (later[l]) ST.stores_left_to_later++; }
        if (n == 4 && !kind[0] && !kind[1] && !kind[2] && !kind[3] && r[0]->nb[2]) {
            int same = 1;
            for (uint32_t i = 1; i < 4; i++) same &= r[i]->len == r[0]->len && r[i]->x[1] == r[0]->x[1] && r[i]->x[2] == r[0]->x[2] && r[i]->base[2] == r[0]->base[2];
            if (same) {
                ST.four_same++;
                int full = 1;
                for (uint32_t k = 0; k < r[3]->n; k++) full &= rank[(3u << sh) + k] == 3 && rank[(2u << sh) + k] == 2 && rank[(1u << sh) + k] == 1;
                if (full) ST.four_same_full_chain++;
            }
        }
        uint32_t offs = 0;                                                           /* the distance tree all lengths >= 6 share: at which lanes does it start in this pass? */
        for (uint32_t i = 0; i < n; i++) if (!kind[i] && r[i]->len >= 6) offs |= 1u << r[i]->k0[1];
        if (offs == ((1u << 4) | (1u << 5) | (1u << 9))) ST.pdist_three_offsets++;
    }
    return n;
}

/* ---------------------------------------------------------------- driver ---------------------------------------------------------------- */
static uint64_t rng_s;
static uint32_t rnd(void) { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)(rng_s >> 16); }

static uint32_t rec_slots(Rec r)
{
    const uint32_t len = (r.w0 >> 1) & 0xFFu, nl = len < 8 ? 4u : len < 16 ? 5u : 9u;
    if (r.w0 & 1u) return nl;
    const uint32_t slot = dist_slot(r.dist), eb = slot > 2 ? slot - 2 : 0;
    return nl + (len == 0 ? 3u : len <= 2 ? 4u : 5u) + (eb > 4 ? (eb - 4 > 16 ? 2u : 1u) : 0u) + (eb ? 4u : 0u);
}
/* the list coded serially and in passes; `take` = records written when a pass starts: 0 random (1..6), else that many; the ring's position starts at m0 */
static void run_list(Rec *rec, uint32_t n, uint32_t take, uint32_t m0, const char *what)
{
    static Model a, b;
    static Rec ring[MRING];
    memset(&a, 0, sizeof a);
    for (uint32_t i = 0; i < P_N; i++) a.P[i] = 31 + rnd() % 4035;                 /* any probability the coder can hold */
    uint32_t qpos = rnd() & 0xFFFFu;                                                /* queue positions: low 16 bits, gaps for the flags between the records */
    for (uint32_t i = 0; i < n; i++) {
        qpos += 2 + rnd() % 4;
        rec[i].w0 = (rec[i].w0 & 0xFFFFu) | (qpos << 16);
        qpos += rec_slots(rec[i]);
        const uint32_t len = (rec[i].w0 >> 1) & 0xFFu;
        ST.len_class[len < 8 ? 0 : len < 16 ? 1 : 2]++;
        if (!(rec[i].w0 & 1u)) {
            const uint32_t slot = dist_slot(rec[i].dist), eb = slot > 2 ? slot - 2 : 0;
            ST.extra_class[eb == 0 ? 0 : eb <= 4 ? 1 : eb <= 20 ? 2 : 3]++; ST.ndir[eb > 4 ? (eb > 20 ? 2 : 1) : 0]++;
        }
    }
    if (n * 24u + 64u > QCAP) abort();                                              /* (the list's slots do not lap the queue) */
    b = a;
    for (uint32_t i = 0; i < n; i++) serial(&a, rec[i]);
    for (uint32_t done = 0, pub = 0; done < n;) {
        const uint32_t more = umin(take ? take : 1 + rnd() % 6, n - done);          /* the spine writes records while the wavefront codes: never more than the ring holds */
        while (pub < done + more) { ring[(m0 + pub) & (MRING - 1)] = rec[pub]; pub++; }
        done += lanes_pass(&b, ring, m0 + done, pub - done);
    }
    ST.lists++; ST.records += n;
    b.P[P_DUMP] = a.P[P_DUMP]; b.q[QCAP] = a.q[QCAP];                               /* where idle lanes store */
    const char *bad = memcmp(a.P, b.P, sizeof a.P) ? "P[]" : memcmp(a.q, b.q, sizeof a.q) ? "queue entries" : NULL;
    if (bad) { printf("trees_lanes_model: %s differ (%s, %u records)\n", bad, what, n); exit(1); }
}
static Rec rep(uint32_t len) { Rec r = {1u | ((len - 2) << 1), 0}; return r; }
/* (a length's distance tree has 3, 4 or 5 levels: the encoder never gives lengths 2 and 3..4 a distance whose slot does not fit) */
static Rec match(uint32_t dist, uint32_t len) { Rec r = {(len - 2) << 1, len == 2 ? dist % 65u : len <= 4 ? dist % 16385u : dist}; return r; }
static Rec any(void)
{
    const uint32_t len = 2 + rnd() % (rnd() % 6 ? 16 : 143);
    if (rnd() % 10 < 4) return rep(len);
    return match((rnd() & 0x7FFFFFFu) >> (rnd() % 27), rnd() % 3 ? len : 2 + rnd() % 8);
}

int main(int argc, char **argv)
{
    rng_s = (argc > 1 ? strtoull(argv[1], NULL, 0) : 20240611ull) * 0x9E3779B97F4A7C15ull + 1;
    const uint32_t lists = argc > 2 ? (uint32_t)atoi(argv[2]) : 4000;
    static Rec rec[MAXR];
    for (uint32_t i = 0; i < lists; i++) {                                          /* seeded random lists; every third from a few lengths and distances: long chains */
        const uint32_t n = 1 + rnd() % 120;
        for (uint32_t r = 0; r < n; r++) rec[r] = i % 3 ? any() : (rnd() & 1 ? rep(2 + rnd() % 3 * 7) : match(1u << (rnd() % 3 * 9), 2 + rnd() % 3 * 7));
        run_list(rec, n, 0, rnd(), "random");
    }
    for (uint32_t take = 1; take <= 4; take++) {                                    /* passes of exactly 1, 2, 3 and 4 records */
        for (uint32_t r = 0; r < 48; r++) rec[r] = r % 3 ? match(5 + r * 11, 2 + r % 14) : rep(2 + r % 14);
        run_list(rec, 48, take, 0, "passes of a given size");
    }
    for (uint32_t v = 0; v < 8; v++) {                                              /* four records with the same length, slot and low nibble: a chain of four at every level */
        const uint32_t len = 2 + v * 2, dist = (1u << (3 + v)) + 7;                 /* (length classes 4 and 5 slots: 16 lanes a record) */
        for (uint32_t r = 0; r < 16; r++) rec[r] = match(dist + (v >= 4 ? (r & 3) << 4 : 0), len);       /* (from 7 extra bits on: other direct bits, same slot and nibble) */
        run_list(rec, 16, 4, v * 9, "four of a kind");
    }
    for (uint32_t v = 0; v < 6; v++) {                                              /* lengths 6-7, 8-15 and >= 16 side by side: the shared distance tree at lanes 4, 5 and 9 */
        static const uint32_t order[6][3] = {{8, 12, 20}, {8, 20, 12}, {12, 8, 20}, {12, 20, 9}, {20, 9, 12}, {30, 15, 8}};
        for (uint32_t r = 0; r < 24; r++) rec[r] = r % 4 == 3 ? rep(2 + r) : match(r % 8 < 4 ? 2 : 1 + (r & 1), order[v][r % 4]);
        run_list(rec, 24, 4, 61, "three length classes");
    }
    {   /* rep records between match records */
        for (uint32_t r = 0; r < 40; r++) rec[r] = r & 1 ? rep(2 + (r >> 1) % 12) : match(40 + r, 2 + (r >> 2) % 12);
        run_list(rec, 40, 4, 3, "match / rep alternating");
        run_list(rec, 40, 3, 62, "match / rep alternating, three a pass");
    }
    {   /* extra bits 0, 1..4, 5..20 and > 20: direct entries 0 / 1 / 2, both sides of every edge, every length class */
        static const uint32_t e[] = {0, 1, 2, 3, 4, 5, 6, 12, 19, 20, 21, 22, 26};
        uint32_t n = 0;
        rec[n++] = match(0, 2); rec[n++] = match(1, 3); rec[n++] = match(2, 9);
        for (uint32_t i = 0; i < 13; i++) { rec[n++] = match((1u << e[i]) + 1 + (rnd() & ((1u << e[i]) - 1u)), 2 + i); rec[n++] = match((2u << e[i]), 10 + i); rec[n++] = match((1u << e[i]) + 2, 18 + i * 9); rec[n++] = rep(3 + i); }
        for (uint32_t take = 1; take <= 4; take++) run_list(rec, n, take, 50 + take, "distance classes");
    }
    {   /* a nine-slot record first, last and in the middle of a pass: in sixteen lanes (rep, or a distance without extra bits) and in thirty-two */
        for (uint32_t at = 0; at < 4; at++)
            for (uint32_t v = 0; v < 3; v++) {
                for (uint32_t r = 0; r < 32; r++) rec[r] = r % 4 != at ? (r & 1 ? rep(2 + r % 13) : match(9 + r, 2 + r % 13)) : v == 0 ? rep(18 + r * 3) : v == 1 ? match(r % 3, 18 + r) : match(100 + r * 1000, 18 + r);
                run_list(rec, 32, 4, 60, "nine-slot records");
                run_list(rec, 32, 3, 63, "nine-slot records, three a pass");
                run_list(rec, 32, 2, 1, "nine-slot records, two a pass");
            }
    }
    for (uint32_t m0 = 60; m0 < 64; m0++) {                                         /* passes that cross ring slot 63 -> 0, at every offset */
        for (uint32_t r = 0; r < 64; r++) rec[r] = r % 5 == 4 ? rep(4 + r % 3) : match(3 + (r % 7 << (r % 11)), 4 + r % 3);
        run_list(rec, 64, 4, m0, "ring's end");
    }
    printf("trees_lanes_model: lists %llu records %llu passes of 1 %llu of 2 %llu of 3 %llu of 4 %llu wide %llu crossing the ring's end %llu\n", (unsigned long long)ST.lists,
           (unsigned long long)ST.records, (unsigned long long)ST.passes[1], (unsigned long long)ST.passes[2], (unsigned long long)ST.passes[3], (unsigned long long)ST.passes[4],
           (unsigned long long)ST.wide_passes, (unsigned long long)ST.ring_cross);
    printf("trees_lanes_model: decisions by earlier records on their cell 0 %llu 1 %llu 2 %llu 3 %llu chain rounds %llu stores left to a later record %llu\n", (unsigned long long)ST.chained[0],
           (unsigned long long)ST.chained[1], (unsigned long long)ST.chained[2], (unsigned long long)ST.chained[3], (unsigned long long)ST.chain_rounds, (unsigned long long)ST.stores_left_to_later);
    printf("trees_lanes_model: four of a kind %llu chained at every level %llu shared distance tree at three offsets %llu rep between matches %llu\n", (unsigned long long)ST.four_same,
           (unsigned long long)ST.four_same_full_chain, (unsigned long long)ST.pdist_three_offsets, (unsigned long long)ST.rep_between_matches);
    printf("trees_lanes_model: extra bits none %llu 1..4 %llu 5..20 %llu above 20 %llu direct entries %llu %llu %llu length classes %llu %llu %llu\n", (unsigned long long)ST.extra_class[0],
           (unsigned long long)ST.extra_class[1], (unsigned long long)ST.extra_class[2], (unsigned long long)ST.extra_class[3], (unsigned long long)ST.ndir[0], (unsigned long long)ST.ndir[1],
           (unsigned long long)ST.ndir[2], (unsigned long long)ST.len_class[0], (unsigned long long)ST.len_class[1], (unsigned long long)ST.len_class[2]);
    printf("trees_lanes_model: nine-slot record first %llu last %llu in the middle %llu of a pass\n", (unsigned long long)ST.nine_first, (unsigned long long)ST.nine_last, (unsigned long long)ST.nine_mid);
    printf("TREES_LANES_OK\n");
    return 0;
}
