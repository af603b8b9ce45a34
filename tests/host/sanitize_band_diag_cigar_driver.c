/*
 * Host-only driver for the sanitizer build of the host side of cigar batches banded around a diagonal
 * (tests/test_sw_band_diag_cigar_sanitizers.py): plan-only batches (agx_sw_batch_create_align_band_diag_cigar with ctx == NULL),
 * the span record (agx_sw_band_span_record) over every start phase, begin column and trimmed first row against its definition,
 * the chunking bound and the band check, under AddressSanitizer + UBSan.  No device is touched: upload, fill and walk need one and run under no sanitizer.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "agx.h"

static int fails = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                    \
        }                                                               \
    } while (0)

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

static int admits(int mode, int64_t la, int64_t lb, int64_t c, int64_t w)
{
    const int64_t dlo = c - w, dhi = c + w;
    const int origin = dlo <= 0 && 0 <= dhi;
    switch (mode) {
    case AGX_SW_MODE_GLOBAL: return origin && dlo <= la - lb && la - lb <= dhi;
    case AGX_SW_MODE_EXTEND: return origin;
    case AGX_SW_MODE_EXTEND_QUERY: return origin && dhi >= la - lb;
    case AGX_SW_MODE_FIT: return dlo <= 0 && dhi >= la - lb;
    default: return 1;
    }
}

static uint8_t bases[2 * 65536];

static void one(int mode, int band, int use_diag, int32_t c, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 65536};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_cigar(NULL, NULL, mode, band, use_diag ? &c : NULL, bases, off, len, 1, &b);
    EXPECT(rc == expect);
    if (rc != expect) fprintf(stderr, "  mode %d band %d diag %d lengths %u x %u: rc %d, expected %d (%s)\n", mode, band, c, la, lb, rc, expect, agx_last_error());
    if (b) {
        agx_sw_info info;
        agx_sw_cigar_info ci;
        agx_sw_hit h;
        agx_sw_stat st;
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
        EXPECT(agx_sw_batch_cigar_info(b, &ci) == AGX_OK && ci.n_chunks == 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
    }
}

static void many(int mode, int band, int64_t n, uint32_t lo, uint32_t hi)
{
    uint64_t *off = (uint64_t *)calloc((size_t)(2 * n + 1), sizeof *off);
    uint32_t *len = (uint32_t *)calloc((size_t)(2 * n + 1), sizeof *len);
    int32_t *diag = (int32_t *)calloc((size_t)(n + 1), sizeof *diag);
    if (!off || !len || !diag) {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    for (int64_t p = 0; p < n; p++) {
        uint32_t la = lo + rnd() % (hi - lo + 1), lb = lo + rnd() % (hi - lo + 1);
        int32_t c = (int32_t)(rnd() % (la + lb + 1)) - (int32_t)lb;
        if (!admits(mode, la, lb, c, band)) c = 0;
        if (!admits(mode, la, lb, c, band)) c = (int32_t)la - (int32_t)lb;
        if (!admits(mode, la, lb, c, band)) { /* GLOBAL with |la - lb| > 2w: no centre serves; make it square */
            lb = la;
            c = 0;
        }
        len[2 * p] = la;
        len[2 * p + 1] = lb;
        off[2 * p] = rnd() % 60000; /* anywhere in the symbols: a plan-only create reads none */
        off[2 * p + 1] = rnd() % 60000;
        diag[p] = c;
    }
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_cigar(NULL, NULL, mode, band, diag, bases, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.n_launches <= 4);
        agx_sw_batch_destroy(b);
    }
    free(off);
    free(len);
    free(diag);
}

/* the span record against its definition, for an image of la x rows from row0 in the band dlo .. dhi counted from row0 */
static void spans(uint32_t la, uint32_t rows, uint32_t row0, uint32_t fpad, int32_t dlo, int32_t dhi, int lanes)
{
    for (int k = 0; k < 400; k++) {
        agx_sw_hit h;
        h.score = 0;
        h.a_begin = (int32_t)(rnd() % la);
        h.a_end = h.a_begin + (int32_t)(rnd() % (la - (uint32_t)h.a_begin));
        h.b_begin = (int32_t)(row0 + rnd() % rows);
        h.b_end = h.b_begin + (int32_t)(rnd() % (row0 + rows - (uint32_t)h.b_begin));
        const int64_t s = (int64_t)h.b_begin - row0, ca = h.a_end - h.a_begin + 1, cb = h.b_end - h.b_begin + 1;
        const int64_t lo = (int64_t)dlo + s - h.a_begin, hi = (int64_t)dhi + s - h.a_begin;
        const int inside = lo <= 0 && 0 <= hi && lo <= ca - cb && ca - cb <= hi;
        agx_sw_band_span sp;
        memset(&sp, 0xee, sizeof sp);
        const int rc = agx_sw_band_span_record(la, rows, row0, fpad, dlo, dhi, lanes, &h, &sp);
        EXPECT(rc == (inside ? AGX_OK : AGX_E_ARG));
        if (rc != AGX_OK) {
            EXPECT(sp.ca == 0xeeeeeeeeu); /* nothing written */
            continue;
        }
        EXPECT(sp.ca == (uint32_t)ca && sp.cb == (uint32_t)cb && sp.x_bytes == fpad + (uint32_t)h.a_begin);
        EXPECT(sp.phase == (uint32_t)(s % 4) && 4 * (int64_t)sp.y_dwords + sp.phase == s);
        EXPECT(sp.dlo == lo && sp.dhi == hi && sp.dhi - sp.dlo == dhi - dlo);
        EXPECT(sp.steps == (uint32_t)cb + (uint32_t)lanes + sp.phase);
    }
}

int main(void)
{
    for (size_t k = 0; k < sizeof bases; k++) bases[k] = (uint8_t)"ACGT"[rnd() & 3];
    for (int mode = 0; mode <= 4; mode++) {
        many(mode, 0, 0, 1, 1);
        for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
            many(mode, band, 2000, 0, 40);
            many(mode, band, 200, 100, 3000);
        }
        many(mode, 16, 20000, 150, 150);
        many(mode, 8, 3, 65535, 65535);
        for (uint32_t la = 0; la <= 5; la++)
            for (uint32_t lb = 0; lb <= 5; lb++)
                for (int w = 0; w <= 2; w++)
                    for (int32_t c = -8; c <= 8; c++) one(mode, w, 1, c, la, lb, admits(mode, la, lb, c, w) ? AGX_OK : AGX_E_ARG);
        one(mode, -1, 1, 0, 10, 10, AGX_E_ARG);
        one(mode, 1024, 1, 0, 10, 10, AGX_E_LIMIT);
        one(mode, 1023, 1, 0, 10, 10, AGX_OK);
        one(mode, 4, 1, 0, 65536, 10, AGX_E_LIMIT);
        one(mode, 4, 1, 0, 10, 65536, AGX_E_LIMIT);
        one(mode, 4, 1, 65535 + 4 + 1, 10, 10, AGX_E_ARG);
        one(mode, 4, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
    }
    one(AGX_SW_MODE_FIT, 128, 1, -63000, 2000, 65535, AGX_OK); /* a read far down a long window */
    one(AGX_SW_MODE_LOCAL, 128, 1, 63000, 65535, 2000, AGX_OK);
    one(7, 4, 1, 0, 10, 10, AGX_E_ARG);
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_cigar(NULL, NULL, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    agx_sw_hit h;
    uint64_t op_off[1];
    EXPECT(agx_sw_align_band_diag_cigar(NULL, NULL, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 0, &h, op_off, NULL, 0) == AGX_E_NODEVICE);

    /* span records: untrimmed and trimmed images, narrow and the widest band, every phase and begin column by chance */
    spans(40, 120, 0, 0, -60, -20, 11);
    spans(40, 90, 17, 3, -43, -3, 6);
    spans(2000, 2257, 28872, 1, -256, 0, 9);
    spans(65535, 65535, 0, 2, -1023, 1023, 64);
    spans(1, 1, 0, 0, 0, 0, 1);
    {
        agx_sw_band_span sp;
        agx_sw_hit ok = {5, 1, 4, 2, 6}, bad;
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, &ok, &sp) == AGX_OK);
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, NULL, &sp) == AGX_E_ARG);
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, &ok, NULL) == AGX_E_ARG);
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 0, &ok, &sp) == AGX_E_ARG);
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 65, &ok, &sp) == AGX_E_ARG);
        EXPECT(agx_sw_band_span_record(10, 10, 3, 0, -3, 3, 2, &ok, &sp) == AGX_E_ARG); /* b_begin < row0 */
        EXPECT(agx_sw_band_span_record(10, 6, 0, 0, -3, 3, 2, &ok, &sp) == AGX_E_ARG);  /* b_end beyond the rows */
        EXPECT(agx_sw_band_span_record(4, 10, 0, 0, -3, 3, 2, &ok, &sp) == AGX_E_ARG);  /* a_end beyond a */
        bad = ok;
        bad.a_begin = -1;
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, &bad, &sp) == AGX_E_ARG);
        bad = ok;
        bad.b_begin = 7; /* b_begin = b_end + 1: an empty side */
        EXPECT(agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, &bad, &sp) == AGX_E_ARG);
    }
    EXPECT(agx_sw_band_cigar_bytes_bound(0, 10, 10) == 0 && agx_sw_band_cigar_bytes_bound(2049, 10, 10) == 0);
    for (int32_t w = 1; w <= 2048; w += 89) EXPECT(agx_sw_band_cigar_bytes_bound(w, 2000, 2100) >= 4u * (2000 + 2100));
    {
        const uint32_t ops[3] = {4u << 4 | AGX_CIGAR_EQ, 2u << 4 | AGX_CIGAR_DEL, 3u << 4 | AGX_CIGAR_INS};
        EXPECT(agx_sw_cigar_in_band(ops, 3, -2, 1) == 1 && agx_sw_cigar_in_band(ops, 3, -1, 1) == 0 && agx_sw_cigar_in_band(ops, 3, -2, 0) == 0);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_DIAG_CIGAR_DRIVER_OK\n");
    return 0;
}
