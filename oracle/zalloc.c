/*
 * oracle/zalloc.c -- deterministic ISzAlloc implementations for the tests.
 * TEST INFRASTRUCTURE.  The reference leaves one byte per coder flush
 * un-stored (csc_coder.cpp:46-47), so goldens are only reproducible with an
 * allocator that hands out memory of known content.
 */
#include <stdlib.h>
#include <string.h>
#include "orc_api.h"

static void *zero_alloc_fn(void *p, size_t n) { (void)p; return calloc(1, n ? n : 1); }
static void any_free_fn(void *p, void *a) { (void)p; free(a); }
static ISzAlloc g_zero = {zero_alloc_fn, any_free_fn};

static void *aa_alloc_fn(void *p, size_t n)
{
    (void)p;
    void *m = malloc(n ? n : 1);
    if (m) memset(m, 0xAA, n);
    return m;
}
static ISzAlloc g_aa = {aa_alloc_fn, any_free_fn};

/* An ISeqOutStream that collects in C.  A stream of one-byte coder blocks makes three Write calls a block (csc_memio.cpp:83-108),
 * hundreds of thousands a stream: too many for a callback into the interpreter (tests/test_gpu_census.py, the arena case). */
typedef struct { ISeqOutStream s; uint8_t *buf; size_t size, cap; } OrcSink;
static size_t sink_write(void *p, const void *buf, size_t size)
{
    OrcSink *k = (OrcSink *)p;
    if (k->size + size > k->cap) {
        size_t cap = k->cap ? k->cap : 4096;
        while (cap < k->size + size) cap *= 2;
        uint8_t *nb = (uint8_t *)realloc(k->buf, cap);
        if (!nb) return 0;
        k->buf = nb; k->cap = cap;
    }
    memcpy(k->buf + k->size, buf, size);
    k->size += size;
    return size;
}
ISeqOutStream *orc_sink_new(void)
{
    OrcSink *k = (OrcSink *)calloc(1, sizeof(OrcSink));
    if (!k) return NULL;
    k->s.Write = sink_write;
    return &k->s;
}
const uint8_t *orc_sink_data(const ISeqOutStream *s, size_t *size) { *size = ((const OrcSink *)s)->size; return ((const OrcSink *)s)->buf; }
void orc_sink_free(ISeqOutStream *s) { if (s) { free(((OrcSink *)s)->buf); free(s); } }

ISzAlloc *orc_zero_alloc(void) { return &g_zero; }
ISzAlloc *orc_aa_alloc(void) { return &g_aa; }
