/*
 * Host-only driver for the sanitizer build of the host side of batches banded around a diagonal under two-piece gap costs
 * (tests/test_sw_band_dual_sanitizers.py): plan-only batches (agx_sw_batch_create_align_band_diag_dual with ctx == NULL) over
 * many shapes under AddressSanitizer + UBSan -- the scoring's limits on all six numbers, the c and w limits, the band conditions
 * of every mode on both sides of their edges, the trimmed rows, lane tiling, the sort, waves, group records and image offsets, and
 * what the batch answers to the calls it does not serve.  No device is touched.
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

static uint8_t bases[65536];
static const agx_sw_scoring_dual mm2 = {2, -4, -4, -2, -24, -1};

/* one pair with every argument given; a plan-only create reads no symbol */
static void one(int mode, int what, int band, int use_diag, int32_t c, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_dual(NULL, &mm2, mode, what, band, use_diag ? &c : NULL, bases, off, len, 1, &b);
    EXPECT(rc == expect);
    if (rc != expect)
        fprintf(stderr, "  mode %d what %d band %d diag %d lengths %u x %u: rc %d, expected %d (%s)\n", mode, what, band, c, la, lb, rc, expect, agx_last_error());
    if (rc == AGX_E_ARG && expect == AGX_E_ARG && mode >= 0 && mode <= 4 && band >= 0 && (what == 1 || what == 2))
        EXPECT(strstr(agx_last_error(), "pair 0") != NULL);
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
        /* the trimmed rows: a group steps over the rows the band touches, at most la + 2w + 1 of them, plus its lanes */
        EXPECT(info.padded_cells <= (int64_t)64 * 32 * ((int64_t)la + 2 * band + 1 + 64));
        agx_sw_batch_destroy(b);
    }
}

/* n random pairs with random centres; those the mode does not admit are moved to a centre it does */
static void many(int mode, int what, int band, int64_t n, uint32_t lo, uint32_t hi)
{
    uint64_t *off = (uint64_t *)calloc((size_t)(2 * n + 1), sizeof *off);
    uint32_t *len = (uint32_t *)calloc((size_t)(2 * n + 1), sizeof *len);
    int32_t *diag = (int32_t *)calloc((size_t)(n + 1), sizeof *diag);
    if (!off || !len || !diag) {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    int64_t cells = 0;
    for (int64_t p = 0; p < n; p++) {
        const uint32_t la = lo + rnd() % (hi - lo + 1), lb = lo + rnd() % (hi - lo + 1);
        int32_t c = (int32_t)(rnd() % (la + lb + 1)) - (int32_t)lb;
        if (!admits(mode, la, lb, c, band)) c = 0;
        if (!admits(mode, la, lb, c, band)) c = (int32_t)la - (int32_t)lb;
        if (!admits(mode, la, lb, c, band)) { /* GLOBAL with |la - lb| > 2w: no centre serves; make it square */
            len[2 * p] = len[2 * p + 1] = la;
            c = 0;
            cells += (int64_t)la * la;
        } else {
            len[2 * p] = la;
            len[2 * p + 1] = lb;
            cells += (int64_t)la * lb;
        }
        diag[p] = c;
    }
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_dual(NULL, &mm2, mode, what, band, diag, bases, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == AGX_E_ARG);
        int32_t stop;
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        EXPECT(agx_sw_batch_bind_scores(b, NULL) == AGX_E_NODEVICE);
        agx_sw_batch_destroy(b);
    }
    free(off);
    free(len);
    free(diag);
}

int main(void)
{
    for (size_t k = 0; k < sizeof bases; k++) bases[k] = (uint8_t)"ACGT"[rnd() & 3];
    for (int mode = 0; mode <= 4; mode++)
        for (int what = AGX_SW_ALIGN_ENDS; what <= AGX_SW_ALIGN_SPANS; what++) {
            many(mode, what, 0, 0, 1, 1);
            for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
                many(mode, what, band, 2000, 0, 40);
                many(mode, what, band, 300, 100, 3000);
            }
            many(mode, what, 16, 30000, 150, 150);
            many(mode, what, 8, 3, 65535, 65535);
            /* every small shape and every centre around it, against the table */
            for (uint32_t la = 0; la <= 6; la++)
                for (uint32_t lb = 0; lb <= 6; lb++)
                    for (int w = 0; w <= 2; w++)
                        for (int32_t c = -10; c <= 10; c++) one(mode, what, w, 1, c, la, lb, admits(mode, la, lb, c, w) ? AGX_OK : AGX_E_ARG);
            /* the limits */
            one(mode, what, -1, 1, 0, 10, 10, AGX_E_ARG);
            one(mode, what, 1024, 1, 0, 10, 10, AGX_E_LIMIT);
            one(mode, what, 1023, 1, 0, 10, 10, AGX_OK);
            one(mode, what, 4, 1, 0, 65536, 10, AGX_E_LIMIT);
            one(mode, what, 4, 1, 0, 10, 65536, AGX_E_LIMIT);
            one(mode, what, 4, 1, 65535 + 4 + 1, 10, 10, AGX_E_ARG);
            one(mode, what, 4, 1, -(65535 + 4 + 1), 10, 10, AGX_E_ARG);
            one(mode, what, 4, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
        }
    one(AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 4, 1, 65535 + 4, 10, 10, AGX_OK);  /* the farthest centre: the band misses the matrix */
    one(AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 4, 1, -(65535 + 4), 10, 10, AGX_OK);
    one(AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 8, 1, -30000, 100, 60000, AGX_OK);   /* a read far down a long window */
    one(AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 128, 1, -63000, 2000, 65535, AGX_OK);
    one(AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 128, 1, 63000, 65535, 2000, AGX_OK);
    one(7, AGX_SW_ALIGN_SPANS, 4, 1, 0, 10, 10, AGX_E_ARG);
    one(-1, AGX_SW_ALIGN_SPANS, 4, 1, 0, 10, 10, AGX_E_ARG);
    one(AGX_SW_MODE_FIT, 0, 4, 1, 0, 10, 10, AGX_E_ARG);
    one(AGX_SW_MODE_FIT, 3, 4, 1, 0, 10, 10, AGX_E_ARG);
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_dual(NULL, &mm2, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    /* the scoring: NULL has no default; each of the six numbers on both sides of its limits */
    const uint64_t off[2] = {0, 100};
    const uint32_t len[2] = {40, 50};
    b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_dual(NULL, NULL, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 16, NULL, bases, off, len, 1, &b) == AGX_E_ARG && !b);
    static const int32_t lo[6] = {1, -116, -1000, -1000, -1000, -1000}, hi[6] = {12, 0, 0, 0, 0, 0};
    for (int k = 0; k < 6; k++)
        for (int side = 0; side < 4; side++) {
            agx_sw_scoring_dual sc = mm2;
            int32_t *const f[6] = {&sc.match, &sc.mismatch, &sc.gap_open, &sc.gap_extend, &sc.gap_open2, &sc.gap_extend2};
            if (k == 1) sc.match = 12; /* mismatch >= match - 128 */
            *f[k] = side == 0 ? lo[k] : side == 1 ? hi[k] : side == 2 ? lo[k] - 1 : hi[k] + 1;
            b = NULL;
            const int rc = agx_sw_batch_create_align_band_diag_dual(NULL, &sc, AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_ENDS, 16, NULL, bases, off, len, 1, &b);
            EXPECT(rc == (side < 2 ? AGX_OK : AGX_E_LIMIT) && (b != NULL) == (side < 2));
            if (b) agx_sw_batch_destroy(b);
        }
    agx_sw_hit h;
    EXPECT(agx_sw_align_band_diag_dual(NULL, &mm2, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 0, &h) == AGX_E_NODEVICE);
    EXPECT(agx_sw_align_band_diag_dual(NULL, NULL, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 0, &h) == AGX_E_ARG);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_DUAL_DRIVER_OK\n");
    return 0;
}
