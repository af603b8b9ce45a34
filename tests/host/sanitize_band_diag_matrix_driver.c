/*
 * Host-only driver for the sanitizer build of batches banded around a diagonal under a substitution matrix
 * (tests/test_sw_band_diag_matrix_sanitizers.py): plan-only batches of both kinds (agx_sw_batch_create_align_band_diag_matrix and
 * its _cigar form with ctx == NULL) over the shapes of sanitize_band_diag_driver.c under AddressSanitizer + UBSan, plus every
 * error path of the matrix validation, which comes before anything else.  No device is touched.
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
static agx_sw_matrix good;

static int create(const agx_sw_matrix *m, int cigar, int mode, int what, int band, const int32_t *diag, const uint64_t *off, const uint32_t *len,
                  int64_t n, agx_sw_batch **b)
{
    return cigar ? agx_sw_batch_create_align_band_diag_matrix_cigar(NULL, m, mode, band, diag, bases, off, len, n, b)
                 : agx_sw_batch_create_align_band_diag_matrix(NULL, m, mode, what, band, diag, bases, off, len, n, b);
}

/* one pair with every argument given; a plan-only create reads no symbol */
static void one(const agx_sw_matrix *m, int cigar, int mode, int what, int band, int use_diag, int32_t c, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = (agx_sw_batch *)1;
    const int rc = create(m, cigar, mode, what, band, use_diag ? &c : NULL, off, len, 1, &b);
    EXPECT(rc == expect);
    EXPECT((rc == AGX_OK) == (b != NULL));
    if (rc != expect)
        fprintf(stderr, "  cigar %d mode %d what %d band %d diag %d lengths %u x %u: rc %d, expected %d (%s)\n", cigar, mode, what, band, c, la, lb, rc,
                expect, agx_last_error());
    if (m == &good && rc == AGX_E_ARG && expect == AGX_E_ARG && mode >= 0 && mode <= 4 && band >= 0 && (cigar || what == 1 || what == 2))
        EXPECT(strstr(agx_last_error(), "pair 0") != NULL);
    if (rc == AGX_OK && b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
        EXPECT(info.padded_cells <= (int64_t)64 * 32 * ((int64_t)la + 2 * band + 1 + 64));
        agx_sw_batch_destroy(b);
    }
}

/* n random pairs with random centres; those the mode does not admit are moved to a centre it does */
static void many(int cigar, int mode, int what, int band, int64_t n, uint32_t lo, uint32_t hi)
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
    const int rc = create(&good, cigar, mode, what, band, diag, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  cigar %d mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", cigar, mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        int32_t stop;
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == (cigar ? AGX_E_NODEVICE : AGX_E_ARG));
        agx_sw_cigar_info ci;
        EXPECT(agx_sw_batch_cigar_info(b, &ci) == (cigar ? AGX_OK : AGX_E_ARG));
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
    memset(&good, 0, sizeof good);
    memset(good.code, 0xff, sizeof good.code);
    good.n_symbols = 4;
    good.gap_open = -3;
    good.gap_extend = -1;
    for (int a = 0; a < 4; a++) {
        good.code[(unsigned char)"ACGT"[a]] = good.code[(unsigned char)"acgt"[a]] = (uint8_t)a;
        for (int c = 0; c < 4; c++) good.score[a][c] = a == c ? 1 : -1;
    }
    for (int cigar = 0; cigar <= 1; cigar++)
        for (int mode = 0; mode <= 4; mode++)
            for (int what = AGX_SW_ALIGN_ENDS; what <= AGX_SW_ALIGN_SPANS; what++) {
                if (cigar && what == AGX_SW_ALIGN_ENDS) continue; /* a cigar batch is a SPANS batch: no `what` */
                many(cigar, mode, what, 0, 0, 1, 1);
                for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
                    many(cigar, mode, what, band, 2000, 0, 40);
                    many(cigar, mode, what, band, 300, 100, 3000);
                }
                many(cigar, mode, what, 16, 30000, 150, 150);
                many(cigar, mode, what, 8, 3, 65535, 65535);
                for (uint32_t la = 0; la <= 6; la++)
                    for (uint32_t lb = 0; lb <= 6; lb++)
                        for (int w = 0; w <= 2; w++)
                            for (int32_t c = -10; c <= 10; c++)
                                one(&good, cigar, mode, what, w, 1, c, la, lb, admits(mode, la, lb, c, w) ? AGX_OK : AGX_E_ARG);
                one(&good, cigar, mode, what, -1, 1, 0, 10, 10, AGX_E_ARG);
                one(&good, cigar, mode, what, 1024, 1, 0, 10, 10, AGX_E_LIMIT);
                one(&good, cigar, mode, what, 1023, 1, 0, 10, 10, AGX_OK);
                one(&good, cigar, mode, what, 4, 1, 0, 65536, 10, AGX_E_LIMIT);
                one(&good, cigar, mode, what, 4, 1, 0, 10, 65536, AGX_E_LIMIT);
                one(&good, cigar, mode, what, 4, 1, 65535 + 4 + 1, 10, 10, AGX_E_ARG);
                one(&good, cigar, mode, what, 4, 1, -(65535 + 4 + 1), 10, 10, AGX_E_ARG);
                one(&good, cigar, mode, what, 4, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
            }
    for (int cigar = 0; cigar <= 1; cigar++) {
        one(&good, cigar, AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 4, 1, 65535 + 4, 10, 10, AGX_OK); /* the band misses the matrix */
        one(&good, cigar, AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 4, 1, -(65535 + 4), 10, 10, AGX_OK);
        one(&good, cigar, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 8, 1, -30000, 100, 60000, AGX_OK); /* a read far down a long window */
        one(&good, cigar, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 128, 1, -63000, 2000, 65535, AGX_OK);
        one(&good, cigar, AGX_SW_MODE_LOCAL, AGX_SW_ALIGN_SPANS, 128, 1, 63000, 65535, 2000, AGX_OK);
        one(&good, cigar, 7, AGX_SW_ALIGN_SPANS, 4, 1, 0, 10, 10, AGX_E_ARG);
        one(&good, cigar, -1, AGX_SW_ALIGN_SPANS, 4, 1, 0, 10, 10, AGX_E_ARG);
        if (!cigar) {
            one(&good, 0, AGX_SW_MODE_FIT, 0, 4, 1, 0, 10, 10, AGX_E_ARG);
            one(&good, 0, AGX_SW_MODE_FIT, 3, 4, 1, 0, 10, 10, AGX_E_ARG);
        }
        /* the matrix is validated first: with good and with bad arguments behind it */
        for (int rest = 0; rest <= 1; rest++) {
            const int mode = rest ? 99 : AGX_SW_MODE_FIT, what = rest ? 7 : AGX_SW_ALIGN_SPANS, band = rest ? -1 : 4;
            agx_sw_matrix m = good;
            one(NULL, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_ARG);
            m.n_symbols = 0;
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_ARG);
            m.n_symbols = 33;
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_ARG);
            m = good;
            m.score[1][2] = 5; /* not symmetric */
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_ARG);
            m = good;
            m.code['N'] = 4; /* a code that is no symbol number */
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_ARG);
            m = good;
            m.gap_open = -1001;
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_LIMIT);
            m = good;
            m.gap_extend = 1;
            one(&m, cigar, mode, what, band, 1, 0, 10, 10, AGX_E_LIMIT);
        }
        agx_sw_matrix edge = good; /* the extremes that are admitted */
        edge.n_symbols = 32;
        edge.gap_open = edge.gap_extend = -1000;
        for (int a = 0; a < 32; a++)
            for (int c = 0; c < 32; c++) edge.score[a][c] = (a + c) % 2 ? -128 : 127;
        one(&edge, cigar, AGX_SW_MODE_GLOBAL, AGX_SW_ALIGN_SPANS, 8, 1, 0, 65535, 65535, AGX_OK);
    }
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_matrix(NULL, &good, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_matrix_cigar(NULL, &good, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    EXPECT(agx_sw_batch_create_align_band_diag_matrix(NULL, &good, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 0, NULL) == AGX_E_ARG);
    agx_sw_hit h;
    uint64_t op_off[1];
    EXPECT(agx_sw_align_band_diag_matrix(NULL, &good, AGX_SW_MODE_FIT, AGX_SW_ALIGN_SPANS, 4, NULL, NULL, NULL, NULL, 0, &h) == AGX_E_NODEVICE);
    EXPECT(agx_sw_align_band_diag_matrix_cigar(NULL, &good, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 0, &h, op_off, NULL, 0) == AGX_E_NODEVICE);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_DIAG_MATRIX_DRIVER_OK\n");
    return 0;
}
