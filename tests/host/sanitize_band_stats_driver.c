/*
 * Host-only driver for the sanitizer build of the planner and validation of stats batches banded around a diagonal
 * (tests/test_sw_band_stats_sanitizers.py): plan-only batches (agx_sw_batch_create_align_band_diag_stats with ctx == NULL) over
 * many shapes under AddressSanitizer + UBSan -- every mode, the band conditions on both sides of their edges, the limits, lane
 * tiling, the sort, waves, group records and image offsets -- and agx_sw_batch_stats on every kind of plan-only banded batch.
 * No device is touched.
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

static uint8_t bases[65536];

/* the table "what the band must hold" of "Banded alignment around a diagonal" */
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

/* one pair with every argument given; a plan-only create reads no symbol */
static void one(int mode, int band, int use_diag, int32_t c, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_stats(NULL, NULL, mode, band, use_diag ? &c : NULL, bases, off, len, 1, &b);
    EXPECT(rc == expect);
    if (rc != expect)
        fprintf(stderr, "  mode %d band %d diag %d lengths %u x %u: rc %d, expected %d (%s)\n", mode, band, c, la, lb, rc, expect, agx_last_error());
    EXPECT((rc == AGX_OK) == (b != NULL));
    if (b) {
        agx_sw_info info;
        agx_sw_hit h;
        agx_sw_stat st = {7, 7};
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
        EXPECT(info.padded_cells <= (int64_t)64 * 32 * ((int64_t)la + 2 * band + 1 + 64));
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_NODEVICE && st.matches == 7 && st.pairs == 7);
        EXPECT(agx_sw_batch_stats(b, NULL, &st) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_stats(b, &h, NULL) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
    }
}

/* n random pairs with random centres inside +-band, moved to 0 where the mode does not admit them (la == lb then) */
static void many(int mode, int band, int64_t n, uint32_t lo, uint32_t hi)
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
        len[2 * p] = lo + rnd() % (hi - lo + 1);
        len[2 * p + 1] = lo + rnd() % (hi - lo + 1);
        diag[p] = (int32_t)(rnd() % (2u * (uint32_t)band + 1u)) - band;
        if (!admits(mode, len[2 * p], len[2 * p + 1], diag[p], band)) {
            len[2 * p + 1] = len[2 * p];
            diag[p] = 0;
        }
        cells += (int64_t)len[2 * p] * len[2 * p + 1];
    }
    agx_sw_batch *b = NULL, *plain = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_stats(NULL, NULL, mode, band, diag, bases, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    EXPECT(agx_sw_batch_create_align_band_diag(NULL, NULL, mode, AGX_SW_ALIGN_SPANS, band, diag, bases, off, len, n, &plain) == AGX_OK);
    if (b && plain) {
        agx_sw_info info, pinfo;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(agx_sw_batch_info(plain, &pinfo) == AGX_OK && pinfo.n_waves == info.n_waves && pinfo.padded_cells == info.padded_cells &&
               pinfo.n_launches == info.n_launches && pinfo.input_bytes == info.input_bytes);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        agx_sw_stat st;
        int32_t stop;
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_stats(plain, &h, &st) == AGX_E_ARG);
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == AGX_E_ARG);
        EXPECT(agx_sw_batch_bind_scores(b, NULL) == AGX_E_NODEVICE);
    }
    agx_sw_batch_destroy(b);
    agx_sw_batch_destroy(plain);
    free(off);
    free(len);
    free(diag);
}

int main(void)
{
    for (size_t k = 0; k < sizeof bases; k++) bases[k] = (uint8_t)"ACGT"[rnd() & 3];
    for (int mode = AGX_SW_MODE_LOCAL; mode <= AGX_SW_MODE_EXTEND_QUERY; mode++) {
        many(mode, 0, 0, 1, 1);
        for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
            many(mode, band, 1500, 0, 40);
            many(mode, band, 200, 100, 3000);
        }
        many(mode, 16, 30000, 150, 150);
        many(mode, 8, 3, 65535, 65535);
        /* every band condition on both sides of its edge, empty sides included */
        for (uint32_t la = 0; la <= 5; la++)
            for (uint32_t lb = 0; lb <= 5; lb++)
                for (int w = 0; w <= 2; w++)
                    for (int32_t c = -8; c <= 8; c++) one(mode, w, 1, c, la, lb, admits(mode, la, lb, c, w) ? AGX_OK : AGX_E_ARG);
        one(mode, 4, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
        /* the limits of a band-diag batch */
        one(mode, -1, 1, 0, 10, 10, AGX_E_ARG);
        one(mode, 1024, 1, 0, 10, 10, AGX_E_LIMIT);
        one(mode, 1023, 1, 0, 10, 10, AGX_OK);
        one(mode, 4, 1, 0, 65536, 10, AGX_E_LIMIT);
        one(mode, 4, 1, 0, 10, 65536, AGX_E_LIMIT);
        one(mode, 7, 1, 65535 + 7 + 1, 10, 10, AGX_E_ARG);
        one(mode, 7, 1, -(65535 + 7 + 1), 10, 10, AGX_E_ARG);
    }
    one(-1, 4, 1, 0, 10, 10, AGX_E_ARG);
    one(5, 4, 1, 0, 10, 10, AGX_E_ARG);
    /* a read in its window: the trimmed rows */
    one(AGX_SW_MODE_FIT, 8, 1, -30000, 100, 60000, AGX_OK);
    one(AGX_SW_MODE_LOCAL, 8, 1, -30000, 100, 60000, AGX_OK);
    /* agx_sw_batch_stats on the other kinds of banded batch */
    {
        const uint64_t off[2] = {0, 0};
        const uint32_t len[2] = {30, 40};
        agx_sw_hit h;
        agx_sw_stat st;
        agx_sw_batch *b = NULL;
        EXPECT(agx_sw_batch_create_align_band(NULL, NULL, AGX_SW_MODE_EXTEND, 4, bases, off, len, 1, &b) == AGX_OK && agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_create_align_band_diag_cigar(NULL, NULL, AGX_SW_MODE_EXTEND, 4, NULL, bases, off, len, 1, &b) == AGX_OK &&
               agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_create_align_band_zdrop(NULL, NULL, AGX_SW_MODE_EXTEND, AGX_SW_ALIGN_SPANS, 4, NULL, 10, bases, off, len, 1, &b) == AGX_OK &&
               agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_stats(NULL, &h, &st) == AGX_E_ARG);
    }
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_stats(NULL, NULL, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    EXPECT(agx_sw_batch_create_align_band_diag_stats(NULL, NULL, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 0, NULL) == AGX_E_ARG);
    agx_sw_hit h;
    agx_sw_stat st;
    EXPECT(agx_sw_align_band_diag_stats(NULL, NULL, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 0, &h, &st) == AGX_E_NODEVICE);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_STATS_DRIVER_OK\n");
    return 0;
}
