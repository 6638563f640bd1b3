/*
 * oracle/orc_synth.c -- stream SYNTHESIZER: turns a script of packets into a libcsc stream body.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT.  The decoders (product, oracle, reference) are otherwise only ever fed
 * streams that an encoder's parser chose to write; this writes any stream the format can express, legal or
 * not, so that the decoders can be compared where no parser goes (tests/synth_gen.py draws the scripts and
 * predicts what the reference must answer).
 *
 * There is no match finder, no parser and no window here: the script says what to code, and every bit goes
 * through the oracle encoder's own coder and model (orc_enc_int.h).  The only state kept is what the decoder
 * derives too: state_, the literal context, the delta path's order-1 context.  The literal context after a
 * copy is the last byte copied, which only a window knows, so the script carries it (`last`).
 *
 * A script is a sequence of uint32 words; every op is its code followed by its operands:
 *   BLOCK type [size]      encode_int(type); DT_ENGTXT (2) takes one more word, the size field the decoder skips
 *   LIT byte
 *   MATCH dist len last    distance >= 1, length >= 2 as the decoder applies them (coded as dist - 1, len - 2)
 *   REP idx len last       rep match, index 0..3, length >= 2
 *   REP0LEN1 last          one-byte rep match
 *   END_RUN                the end-of-run marker (a match of coded length 0 at coded distance 64)
 *   RESTART flag           encode_int(flag); flag 1 also flushes the coder: the decoder restarts on new blocks
 *   BAD n bytes.. / ENTROPY n bytes.. / LITS n bytes..     n, then the bytes packed four a word, low byte first
 *   DLT type n             encode_int(type), the RLE size field n; then RLE_LIT byte / RLE_RUN len (len >= 11)
 *   EOF                    encode_int(SIG_EOF) and a flush
 *   RAW_TYPE value         encode_int(value) and nothing else (an unknown block type)
 *   FLUSH                  flush the coder without a flag (the end of a stream that stops short of EOF)
 * The 10 property bytes are the caller's to write, as with CSCEnc_Create.
 */
#include <stdlib.h>
#include <string.h>

#include "orc_enc_int.h"

static void *syn_alloc(void *p, size_t n) { (void)p; return malloc(n); }
static void syn_free(void *p, void *a) { (void)p; free(a); }
static ISzAlloc g_syn_alloc = {syn_alloc, syn_free};

static const uint8_t *packed(const uint32_t *s, size_t words, size_t *i, uint32_t n, uint8_t **tmp)
{
    size_t need = ((size_t)n + 3) / 4;
    if (need > words - *i) return NULL;
    uint8_t *b = (uint8_t *)realloc(*tmp, (size_t)n + 4);
    if (!b) return NULL;
    *tmp = b;
    for (uint32_t k = 0; k < n; k++) b[k] = (uint8_t)(s[*i + k / 4] >> (8 * (k & 3)));
    *i += need;
    return b;
}

/* Returns 0, WRITE_ERROR when the output stream refuses bytes, -1 for a malformed script (nothing is read past `words`). */
int orc_synth(const CSCProps *props, const uint32_t *s, size_t words, ISeqOutStream *out, ISzAlloc *user_alloc)
{
    ISzAlloc *const alloc = user_alloc ? user_alloc : &g_syn_alloc;
    if (props->csc_blocksize < 16) return -1;
    OrcEnc *e = (OrcEnc *)alloc->Alloc(alloc, sizeof(OrcEnc));
    if (!e) return -1;
    memset(e, 0, sizeof(*e));
    e->alloc = alloc; e->os = out; e->props = *props;
    e->bsize = props->csc_blocksize;
    coder_reset_state(e);
    e->rc_buf = (uint8_t *)alloc->Alloc(alloc, e->bsize);
    e->bc_buf = (uint8_t *)alloc->Alloc(alloc, e->bsize);
    e->p_lit = (uint32_t *)alloc->Alloc(alloc, 256 * 256 * sizeof(uint32_t));
    uint8_t *volatile tmp = NULL;   /* (volatile: lives across the setjmp) */
    volatile int ret = -1;
    if (e->rc_buf && e->bc_buf && e->p_lit) {
        memset(e->rc_buf, 0, e->bsize);
        memset(e->bc_buf, 0, e->bsize);
        model_reset(e);
        int code = setjmp(e->on_error);
        if (code != 0) { ret = -code; goto done; }
        uint32_t sctx = 0;
        size_t i = 0;
#define NEED(K) do { if ((size_t)(K) > words - i) goto done; } while (0)
        while (i < words) {
            uint32_t op = s[i++];
            switch (op) {
            case ORC_OP_BLOCK:
                NEED(1);
                encode_int(e, s[i]);
                if (s[i++] == DT_ENGTXT) { NEED(1); encode_int(e, s[i++]); }
                break;
            case ORC_OP_RAW_TYPE:
                NEED(1); encode_int(e, s[i++]);
                break;
            case ORC_OP_LIT:
                NEED(1); if (s[i] > 255) goto done;
                encode_literal(e, s[i++]);
                break;
            case ORC_OP_MATCH:
                NEED(3); if (s[i] < 1 || s[i] > (1u << 30) + 1 || s[i + 1] < 2 || s[i + 2] > 255) goto done;
                /* distances the length's context has no slot for (and length 2 at 65: that is END_RUN) */
                if ((s[i + 1] == 2 && s[i] > 64) || (s[i + 1] <= 4 && s[i] > 16385)) goto done;
                encode_match(e, s[i] - 1, s[i + 1] - 2);
                e->ctx = s[i + 2];
                i += 3;
                break;
            case ORC_OP_REP:
                NEED(3); if (s[i] > 3 || s[i + 1] < 2 || s[i + 2] > 255) goto done;
                encode_rep_match(e, s[i], s[i + 1] - 2);
                e->ctx = s[i + 2];
                i += 3;
                break;
            case ORC_OP_REP0LEN1:
                NEED(1); if (s[i] > 255) goto done;
                encode_rep0len1(e);
                e->ctx = s[i++];
                break;
            case ORC_OP_END_RUN:
                encode_match(e, 64, 0);
                break;
            case ORC_OP_RESTART:
                NEED(1);
                encode_int(e, s[i]);
                if (s[i++] == 1) coder_flush(e);
                break;
            case ORC_OP_BAD: case ORC_OP_ENTROPY: case ORC_OP_LITS: {
                NEED(1);
                uint32_t n = s[i++];
                uint8_t *t = tmp;
                const uint8_t *b = packed(s, words, &i, n, &t);
                tmp = t;
                if (!b) goto done;
                if (op == ORC_OP_BAD) compress_bad(e, b, n);
                else if (op == ORC_OP_ENTROPY) compress_literals(e, b, n);
                else for (uint32_t k = 0; k < n; k++) encode_literal(e, b[k]);
                break;
            }
            case ORC_OP_DLT:
                NEED(2);
                encode_int(e, s[i]);
                rle_begin(e, s[i + 1]);
                sctx = 0;
                i += 2;
                break;
            case ORC_OP_RLE_LIT:
                NEED(1); if (s[i] > 255 || !e->p_delta) goto done;
                rle_lit(e, sctx, s[i]);
                sctx = s[i++];
                break;
            case ORC_OP_RLE_RUN:
                NEED(1); if (s[i] < 11 || !e->p_delta) goto done;
                rle_run(e, s[i++] - 11);
                break;
            case ORC_OP_EOF:
                encode_int(e, SIG_EOF);
                coder_flush(e);
                break;
            case ORC_OP_FLUSH:
                coder_flush(e);
                break;
            default:
                goto done;
            }
        }
#undef NEED
        ret = 0;
    }
done:
    free((void *)tmp);
    ISzAlloc *a = e->alloc;
    a->Free(a, e->rc_buf); a->Free(a, e->bc_buf);
    a->Free(a, e->p_lit); a->Free(a, e->p_delta);
    a->Free(a, e);
    return ret;
}
