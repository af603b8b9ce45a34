/*
 * Host-only driver for the sanitizer build of the planner and validation of z-drop batches
 * (tests/test_sw_band_zdrop_sanitizers.py): plan-only batches (agx_sw_batch_create_align_band_zdrop and _zdrop_cigar with
 * ctx == NULL) over many shapes under AddressSanitizer + UBSan -- the zdrop limits, the mode, the admission rule on both sides of
 * its edges, lane tiling, the sort, waves, group records and image offsets -- and agx_sw_batch_zdrop_stops on every kind of
 * plan-only batch.  No device is touched.
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

/* one pair with every argument given; a plan-only create reads no symbol */
static void one(int cigar, int mode, int what, int band, int use_diag, int32_t c, int32_t zdrop, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = NULL;
    const int rc = cigar ? agx_sw_batch_create_align_band_zdrop_cigar(NULL, NULL, mode, band, use_diag ? &c : NULL, zdrop, bases, off, len, 1, &b)
                         : agx_sw_batch_create_align_band_zdrop(NULL, NULL, mode, what, band, use_diag ? &c : NULL, zdrop, bases, off, len, 1, &b);
    EXPECT(rc == expect);
    if (rc != expect)
        fprintf(stderr, "  cigar %d mode %d what %d band %d diag %d zdrop %d lengths %u x %u: rc %d, expected %d (%s)\n", cigar, mode, what, band, c,
                zdrop, la, lb, rc, expect, agx_last_error());
    EXPECT((rc == AGX_OK) == (b != NULL));
    if (b) {
        agx_sw_info info;
        int32_t stop = 7;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
        EXPECT(info.padded_cells <= (int64_t)64 * 32 * ((int64_t)la + 2 * band + 1 + 64));
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_NODEVICE && stop == 7);
        EXPECT(agx_sw_batch_zdrop_stops(b, NULL) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
    }
}

/* n random pairs with random centres inside +-band */
static void many(int cigar, int what, int band, int32_t zdrop, int64_t n, uint32_t lo, uint32_t hi)
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
        cells += (int64_t)len[2 * p] * len[2 * p + 1];
        diag[p] = (int32_t)(rnd() % (2u * (uint32_t)band + 1u)) - band;
    }
    agx_sw_batch *b = NULL;
    const int rc = cigar ? agx_sw_batch_create_align_band_zdrop_cigar(NULL, NULL, AGX_SW_MODE_EXTEND, band, diag, zdrop, bases, off, len, n, &b)
                         : agx_sw_batch_create_align_band_zdrop(NULL, NULL, AGX_SW_MODE_EXTEND, what, band, diag, zdrop, bases, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  cigar %d band %d n %lld lengths %u..%u: rc %d (%s)\n", cigar, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        int32_t stop;
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_NODEVICE);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == (cigar ? AGX_E_NODEVICE : AGX_E_ARG));
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
    static const int32_t zs[] = {0, 1, 100, AGX_SW_ZDROP_MAX};
    for (int cigar = 0; cigar <= 1; cigar++)
        for (int what = AGX_SW_ALIGN_ENDS; what <= AGX_SW_ALIGN_SPANS; what++) {
            if (cigar && what == AGX_SW_ALIGN_ENDS) continue;
            many(cigar, what, 0, 5, 0, 1, 1);
            for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
                many(cigar, what, band, zs[band & 3], 2000, 0, 40);
                many(cigar, what, band, 20, 300, 100, 3000);
            }
            many(cigar, what, 16, 100, 30000, 150, 150);
            many(cigar, what, 8, 100, 3, 65535, 65535);
            /* the admission rule dlo <= 0 <= dhi on both sides of its edges, empty sides included */
            for (uint32_t la = 0; la <= 5; la++)
                for (uint32_t lb = 0; lb <= 5; lb++)
                    for (int w = 0; w <= 2; w++)
                        for (int32_t c = -4; c <= 4; c++) one(cigar, AGX_SW_MODE_EXTEND, what, w, 1, c, 3, la, lb, c - w <= 0 && 0 <= c + w ? AGX_OK : AGX_E_ARG);
            /* zdrop */
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, -1, 10, 10, AGX_E_ARG);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, AGX_SW_ZDROP_MAX + 1, 10, 10, AGX_E_ARG);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, INT32_MIN, 10, 10, AGX_E_ARG);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, INT32_MAX, 10, 10, AGX_E_ARG);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, AGX_SW_ZDROP_MAX, 10, 10, AGX_OK);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 0, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
            /* the mode */
            for (int mode = -1; mode <= 5; mode++)
                if (mode != AGX_SW_MODE_EXTEND) one(cigar, mode, what, 4, 1, 0, 10, 10, 10, AGX_E_ARG);
            /* the limits of a band-diag batch */
            one(cigar, AGX_SW_MODE_EXTEND, what, -1, 1, 0, 10, 10, 10, AGX_E_ARG);
            one(cigar, AGX_SW_MODE_EXTEND, what, 1024, 1, 0, 10, 10, 10, AGX_E_LIMIT);
            one(cigar, AGX_SW_MODE_EXTEND, what, 1023, 1, 0, 10, 10, 10, AGX_OK);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, 10, 65536, 10, AGX_E_LIMIT);
            one(cigar, AGX_SW_MODE_EXTEND, what, 4, 1, 0, 10, 10, 65536, AGX_E_LIMIT);
        }
    one(0, AGX_SW_MODE_EXTEND, 0, 4, 1, 0, 10, 10, 10, AGX_E_ARG);
    one(0, AGX_SW_MODE_EXTEND, 3, 4, 1, 0, 10, 10, 10, AGX_E_ARG);
    /* agx_sw_batch_zdrop_stops on the other kinds of batch */
    {
        const uint64_t off[2] = {0, 0};
        const uint32_t len[2] = {30, 40};
        int32_t stop;
        agx_sw_batch *b = NULL;
        EXPECT(agx_sw_batch_create(NULL, bases, off, len, 1, &b) == AGX_OK && agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_create_align_band(NULL, NULL, AGX_SW_MODE_EXTEND, 4, bases, off, len, 1, &b) == AGX_OK && agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_create_align_band_diag(NULL, NULL, AGX_SW_MODE_EXTEND, AGX_SW_ALIGN_SPANS, 4, NULL, bases, off, len, 1, &b) == AGX_OK &&
               agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
        EXPECT(agx_sw_batch_zdrop_stops(NULL, &stop) == AGX_E_ARG);
    }
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_zdrop(NULL, NULL, AGX_SW_MODE_EXTEND, AGX_SW_ALIGN_SPANS, 4, NULL, 5, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    agx_sw_hit h;
    EXPECT(agx_sw_align_band_zdrop(NULL, NULL, AGX_SW_MODE_EXTEND, AGX_SW_ALIGN_SPANS, 4, NULL, 5, NULL, NULL, NULL, 0, &h, NULL) == AGX_E_NODEVICE);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_ZDROP_DRIVER_OK\n");
    return 0;
}
