/*
 * tests/model/trees_model.c -- what an input makes the level-3 parser hand to the tree wavefront (csc_amd/csrc/csc_kernels_dp4.inc:
 * d6_literal / d6_tree_record / d6_chunk_lanes -> d6_trees), counted on the CPU.  TEST INFRASTRUCTURE: it includes the oracle's encoder
 * and runs compress_advanced (csc_lz.cpp:207-333) through the oracle's test hook in the oracle's own arrangement, so the bytes are the
 * oracle's; next to the coding it keeps, per way out (a window's packets plus its exit packet), the records the kernel would write:
 *
 *   literal record      one per literal (context, symbol): eight tree decisions in p_lit, coded up to sixteen records a pass, two halves of eight
 *   match / rep record  one per match or rep match shorter than 145 (rep0len1 has no tree): the length tree, and for a match the
 *                       distance slot tree, zero to two direct-bit entries and the four-bit low tree
 *
 * and from them the conditions tests/test_gpu_trees.py wants its inputs to reach (tests/test_trees_model.py asserts them):
 * records per way out, records of one way out that meet on the same cells, the distance classes inside a run of eight records, ring
 * wraps (128 literal records, 64 match records) inside a way out, repeated (context, symbol) pairs across the halves of sixteen
 * literal records, exit literals (the last literal record of their way out) that share their context row with a literal of the window
 * or land on a ring boundary, positions that leave without a window, queue entries (the spine asks the
 * coder's queue for room about every 2 000 entries: d6_room's slow path) and GetMatchLenPrice refreshes that fall into the first nodes of
 * a window whose predecessor left match records.
 *
 *   gcc -std=gnu99 -O2 -fPIC -shared -Wall -Wextra -Werror -Wl,-Bsymbolic -o libtreesmodel.so trees_model.c ../../oracle/orc_decoder.c ../../oracle/zalloc.c -lm
 */
#include <stdio.h>
#include "../../oracle/orc_encoder.c"

enum { TR_LRING = 128, TR_MRING = 64, TR_MAXREC = 4096 };

typedef struct {
    uint64_t windows, exit_limit, exit_lit, exit_match, exit_match_long, no_window, exit_lit_end0;
    uint64_t lit_records, match_records, queue_entries;
    uint64_t most_lit, most_match;                       /* records of one way out */
    uint64_t wo_match_gt8, wo_lit_gt8, wo_lit_gt16, wo_gt64_nodes;
    uint64_t same_len_cells, same_slot_cells, same_low_cells;     /* in ways out with more than eight match / rep records: records that repeat an earlier record's length, (length class, distance slot), (extra bits, low nibble) inside the same run of eight */
    uint64_t runs8_all_classes;                          /* runs of eight consecutive match records of one way out with extra bits 0, 1..4, 5..20 and > 20 all present */
    uint64_t dir0, dir1, dir2;                           /* match records with zero, one, two direct-bit entries */
    uint64_t lring_wraps_inside, mring_wraps_inside;     /* ways out whose records cross a multiple of the ring size */
    uint64_t pair_repeats_across_halves;                 /* (context, symbol) of record 8..15 of a group of sixteen equal to one of records 0..7 */
    uint64_t pair_repeats_in_eight;                      /* ... of an earlier record of the same group of eight */
    uint64_t exit_lit_same_row, exit_lit_same_pair;      /* exit literal with a window literal in the same context row / with the same symbol too */
    uint64_t exit_lit_on_ring_edge;                      /* exit literal's record at ring slot 0 or 127 */
    uint64_t exit_lit_after_gt64;                        /* exit literal behind a window of more than 64 nodes (more than one chunk of packets) */
    uint64_t no_window_runs_ge8;                         /* eight or more positions in a row without a window */
    uint64_t refreshes, refreshes_early_after_records;   /* len_price_rebuild calls; those within the first eight nodes of a window whose predecessor left match records */
} TrCounts;

static TrCounts T;
static uint64_t tr_lt_total, tr_mt_total;
static uint32_t tr_prev_match, tr_nowin_run;
/* the way out being collected */
static struct { uint32_t ctx, sym; } tr_l[TR_MAXREC];
static struct { uint32_t len, dist, rep; } tr_m[TR_MAXREC];
static uint32_t tr_nl, tr_nm, tr_entries;

static uint32_t tr_len_slots(uint32_t len) { return len < 8 ? 4u : len < 16 ? 5u : 9u; }
static uint32_t tr_class(uint32_t eb) { return eb == 0 ? 0u : eb <= 4 ? 1u : eb <= 20 ? 2u : 3u; }
static uint32_t tr_extra_bits(uint32_t dist) { const uint32_t s = dist_slot(dist); return s > 2 ? s - 2 : 0; }

static void tr_lit(OrcEnc *e, uint32_t c)
{
    if (tr_nl < TR_MAXREC) { tr_l[tr_nl].ctx = e->ctx; tr_l[tr_nl].sym = c; }
    tr_nl++; tr_entries += 9;
    encode_literal(e, c);
}
static void tr_rep0len1(OrcEnc *e) { tr_entries += 3; encode_rep0len1(e); }
static void tr_rep(OrcEnc *e, uint32_t idx, uint32_t len)
{
    if (len < 143) {
        if (tr_nm < TR_MAXREC) { tr_m[tr_nm].len = len; tr_m[tr_nm].dist = 0; tr_m[tr_nm].rep = 1; }
        tr_nm++; tr_entries += 5 + tr_len_slots(len);
    } else T.exit_match_long++;
    encode_rep_match(e, idx, len);
}
static void tr_match(OrcEnc *e, uint32_t dist, uint32_t len)
{
    if (len < 143) {
        const uint32_t eb = tr_extra_bits(dist), ndir = eb > 4 ? (eb - 4 > 16 ? 2u : 1u) : 0u;
        if (tr_nm < TR_MAXREC) { tr_m[tr_nm].len = len; tr_m[tr_nm].dist = dist; tr_m[tr_nm].rep = 0; }
        tr_nm++; tr_entries += 2 + tr_len_slots(len) + (len == 0 ? 3u : len <= 2 ? 4u : 5u) + ndir + (eb ? 4u : 0u);
        if (ndir == 0) T.dir0++; else if (ndir == 1) T.dir1++; else T.dir2++;
    } else T.exit_match_long++;
    encode_match(e, dist, len);
}
static void tr_nonlit(OrcEnc *e, MFUnit u)                 /* lz_encode_nonlit */
{
    if (u.dist <= 4) {
        if (u.len == 1 && u.dist == 1) tr_rep0len1(e);
        else {
            tr_rep(e, u.dist - 1, u.len - 2);
            uint32_t d = e->rep_dist[u.dist - 1];
            for (uint32_t k = u.dist - 1; k > 0; k--) e->rep_dist[k] = e->rep_dist[k - 1];
            e->rep_dist[0] = d;
        }
    } else {
        tr_match(e, u.dist - 5, u.len - 2);
        e->rep_dist[3] = e->rep_dist[2]; e->rep_dist[2] = e->rep_dist[1];
        e->rep_dist[1] = e->rep_dist[0]; e->rep_dist[0] = u.dist - 4;
    }
}
static void tr_backward(OrcEnc *e, int end)                /* lz_ap_backward */
{
    APUnit *ap = e->ap;
    for (int i = end; i;) { ap[ap[i].back_pos].next_pos = i; i = ap[i].back_pos; }
    for (int i = 0; i != end;) {
        uint32_t next = (uint32_t)ap[i].next_pos;
        if (ap[next].dist == 0) tr_lit(e, ap[i].lit);
        else if (ap[next].dist <= 4) {
            if (next - i == 1 && ap[next].dist == 1) tr_rep0len1(e);
            else tr_rep(e, ap[next].dist - 1, next - i - 2);
            e->ctx = ap[next - 1].lit;
        } else {
            tr_match(e, ap[next].dist - 5, next - i - 2);
            e->ctx = ap[next - 1].lit;
        }
        i = (int)next;
    }
    memcpy(e->rep_dist, ap[end].rep_dist, sizeof(e->rep_dist));
}
/* a way out is complete: `exit_lit` = its last literal record is the exit literal */
static void tr_close(uint32_t nodes, int exit_lit)
{
    const uint32_t nl = tr_nl < TR_MAXREC ? tr_nl : TR_MAXREC, nm = tr_nm < TR_MAXREC ? tr_nm : TR_MAXREC;
    T.windows++;
    if (tr_nl > T.most_lit) T.most_lit = tr_nl;
    if (tr_nm > T.most_match) T.most_match = tr_nm;
    if (tr_nm > 8) T.wo_match_gt8++;
    if (tr_nl > 8) T.wo_lit_gt8++;
    if (tr_nl > 16) T.wo_lit_gt16++;
    if (nodes > 64) T.wo_gt64_nodes++;
    if (tr_nm > 8)
        for (uint32_t r = 0; r < nm; r++)
            for (uint32_t q = r & ~7u; q < r; q++) {
                const uint32_t eb_r = tr_extra_bits(tr_m[r].dist), eb_q = tr_extra_bits(tr_m[q].dist);
                const uint32_t lc_r = tr_m[r].len > 5 ? 6u : tr_m[r].len, lc_q = tr_m[q].len > 5 ? 6u : tr_m[q].len;      /* P_DIST's row: length 0, 1..2 by length, 3..5 by length, the rest */
                if (tr_m[r].len == tr_m[q].len) { T.same_len_cells++; }
                if (!tr_m[r].rep && !tr_m[q].rep && lc_r == lc_q && dist_slot(tr_m[r].dist) == dist_slot(tr_m[q].dist)) T.same_slot_cells++;
                if (!tr_m[r].rep && !tr_m[q].rep && eb_r && eb_r == eb_q
                    && ((tr_m[r].dist - (1u << eb_r) - 1) & 15u) == ((tr_m[q].dist - (1u << eb_q) - 1) & 15u)) T.same_low_cells++;
            }
    for (uint32_t r = 0; r + 8 <= nm; r++) {
        uint32_t seen = 0;
        for (uint32_t q = r; q < r + 8; q++) if (!tr_m[q].rep) seen |= 1u << tr_class(tr_extra_bits(tr_m[q].dist));
        if (seen == 15u) T.runs8_all_classes++;
    }
    if (tr_nl && (tr_lt_total % TR_LRING) + tr_nl > TR_LRING) T.lring_wraps_inside++;
    if (tr_nm && (tr_mt_total % TR_MRING) + tr_nm > TR_MRING) T.mring_wraps_inside++;
    for (uint32_t r = 0; r < nl; r++) {
        for (uint32_t q = r & ~7u; q < r; q++) if (tr_l[q].ctx == tr_l[r].ctx && tr_l[q].sym == tr_l[r].sym) { T.pair_repeats_in_eight++; break; }
        if (r & 8u) for (uint32_t q = r & ~15u; q < (r & ~7u); q++) if (tr_l[q].ctx == tr_l[r].ctx && tr_l[q].sym == tr_l[r].sym) { T.pair_repeats_across_halves++; break; }
    }
    if (exit_lit && nl) {
        int row = 0, pair = 0;
        for (uint32_t q = 0; q + 1 < nl; q++) if (tr_l[q].ctx == tr_l[nl - 1].ctx) { row = 1; if (tr_l[q].sym == tr_l[nl - 1].sym) pair = 1; }
        T.exit_lit_same_row += (uint64_t)row; T.exit_lit_same_pair += (uint64_t)pair;
        const uint64_t slot = (tr_lt_total + tr_nl - 1) % TR_LRING;
        if (slot == 0 || slot == TR_LRING - 1) T.exit_lit_on_ring_edge++;
        if (nodes > 64) T.exit_lit_after_gt64++;
        if (nodes == 0) T.exit_lit_end0++;
    }
    T.lit_records += tr_nl; T.match_records += tr_nm; T.queue_entries += tr_entries;
    tr_lt_total += tr_nl; tr_mt_total += tr_nm;
    tr_prev_match = tr_nm;
    tr_nl = tr_nm = tr_entries = 0;
    tr_nowin_run = 0;
}
static void tr_priced(OrcEnc *e, uint32_t state, MFUnit *ret, const uint32_t *rep_dist, uint32_t wpos, uint32_t limit, uint32_t node)
{
    const uint32_t before = e->lp_rebuild_int;
    mf_find_priced(e, state, ret, rep_dist, wpos, limit);
    if (e->lp_rebuild_int > before) { T.refreshes++; if (node < 8 && tr_prev_match) T.refreshes_early_after_records++; }
}

/* lz_compress_advanced, the oracle's arrangement, with the counting in place of the plain encode calls */
static void tr_adv(OrcEnc *e, uint32_t size)
{
    APUnit *ap = e->ap;
    MFUnit *appt = e->appt;
    uint32_t apend = 0, apcur = 0;
    for (uint32_t i = 0; i < size;) {
        tr_priced(e, e->state, appt, e->rep_dist, e->wnd_curpos, size - i, 0);
        if (appt[0].dist == 0) {
            T.no_window++; T.lit_records++; T.queue_entries += 9; tr_lt_total++;
            if (++tr_nowin_run == 8) T.no_window_runs_ge8++;
            encode_literal(e, e->wnd[e->wnd_curpos]);
            mf_slide_pos(e, e->wnd_curpos, 1, size - i);
            i++; e->wnd_curpos++;
            continue;
        }
        apcur = 0; apend = 1;
        ap[0].price = 0; ap[0].back_pos = 0;
        memcpy(ap[0].rep_dist, e->rep_dist, sizeof(e->rep_dist));
        ap[0].state = e->state;
        uint32_t aplimit = UMIN((uint32_t)AP_LIMIT, size - i);
        for (;;) {
            ap[apcur].lit = e->wnd[e->wnd_curpos];
            if (apcur) {
                int l = ap[apcur].back_pos;
                memcpy(ap[apcur].rep_dist, ap[l].rep_dist, sizeof(ap[l].rep_dist));
                if (ap[apcur].dist == 0) {
                    ap[apcur].state = (ap[l].state * 4) & 0x3F;
                } else if (ap[apcur].dist <= 4) {
                    uint32_t len = apcur - (uint32_t)l;
                    if (len == 1 && ap[apcur].dist == 1)
                        ap[apcur].state = (ap[l].state * 4 + 2) & 0x3F;
                    else {
                        ap[apcur].state = (ap[l].state * 4 + 3) & 0x3F;
                        uint32_t k = ap[apcur].dist - 1, tmp = ap[apcur].rep_dist[k];
                        if (k >= 1) {
                            for (; k > 0; k--) ap[apcur].rep_dist[k] = ap[apcur].rep_dist[k - 1];
                            ap[apcur].rep_dist[0] = tmp;
                        }
                    }
                } else {
                    ap[apcur].state = (ap[l].state * 4 + 1) & 0x3F;
                    ap[apcur].rep_dist[0] = ap[apcur].dist - 4;
                    ap[apcur].rep_dist[1] = ap[l].rep_dist[0];
                    ap[apcur].rep_dist[2] = ap[l].rep_dist[1];
                    ap[apcur].rep_dist[3] = ap[l].rep_dist[2];
                }
                if (apcur < aplimit)
                    tr_priced(e, ap[apcur].state, appt, ap[apcur].rep_dist, e->wnd_curpos, size - i - apcur, apcur);
            }
            if (apcur == aplimit) {
                tr_backward(e, (int)apcur);
                i += apcur;
                T.exit_limit++; tr_close(apcur, 0);
                break;
            }
            if (appt[0].len == 1 && apcur + 1 == apend) {
                tr_backward(e, (int)apcur);
                tr_lit(e, ap[apcur].lit);
                i += apcur;
                mf_slide_pos(e, e->wnd_curpos, 1, size - i);
                e->wnd_curpos++;
                i++;
                T.exit_lit++; tr_close(apcur, 1);
                break;
            }
            if (apcur + 1 >= apend) ap[apend++].price = 0xFFFFFFFFu;
            if (appt[0].len >= e->lz_good_len || (appt[0].len > 1 && appt[0].len + apcur >= aplimit)) {
                tr_backward(e, (int)apcur);
                i += apcur;
                tr_nonlit(e, appt[0]);
                mf_slide_pos(e, e->wnd_curpos, appt[0].len, size - i);
                i += appt[0].len;
                e->wnd_curpos += appt[0].len;
                e->ctx = e->wnd[e->wnd_curpos - 1];
                T.exit_match++; tr_close(apcur, 0);
                break;
            }
            uint32_t lit_ctx = e->wnd_curpos ? e->wnd[e->wnd_curpos - 1] : 0;
            uint32_t cprice = literal_price(e, ap[apcur].state, lit_ctx, e->wnd[e->wnd_curpos]);
            if (cprice + ap[apcur].price < ap[apcur + 1].price) {
                ap[apcur + 1].dist = 0;
                ap[apcur + 1].back_pos = (int)apcur;
                ap[apcur + 1].price = cprice + ap[apcur].price;
            }
            if (appt[1].dist && appt[1].len + ap[apcur].price < ap[apcur + 1].price) {
                ap[apcur + 1].dist = 1;
                ap[apcur + 1].back_pos = (int)apcur;
                ap[apcur + 1].price = appt[1].len + ap[apcur].price;
            }
            uint32_t len = appt[0].len;
            while (apcur + len >= apend) ap[apend++].price = 0xFFFFFFFFu;
            while (len > 1) {
                if (appt[len].dist && appt[len].len + ap[apcur].price < ap[apcur + len].price) {
                    ap[apcur + len].dist = appt[len].dist;
                    ap[apcur + len].back_pos = (int)apcur;
                    ap[apcur + len].price = appt[len].len + ap[apcur].price;
                }
                len--;
            }
            apcur++;
            mf_slide_pos(e, e->wnd_curpos, 1, size - i - apcur);
            e->wnd_curpos++;
        }
    }
}

__attribute__((constructor)) static void tr_install(void) { orc_adv_hook = tr_adv; }

/* the counters since the last reset, as 64-bit words in TrCounts' order; -> how many there are */
int trees_model_counts(uint64_t *out, int cap)
{
    const int n = (int)(sizeof(TrCounts) / sizeof(uint64_t));
    for (int i = 0; i < n && i < cap; i++) out[i] = ((const uint64_t *)&T)[i];
    return n;
}
void trees_model_reset(void)
{
    memset(&T, 0, sizeof T);
    tr_lt_total = tr_mt_total = 0; tr_prev_match = tr_nowin_run = 0; tr_nl = tr_nm = tr_entries = 0;
}
