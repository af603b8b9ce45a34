/*
 * Host-only driver for the sanitizer build of banded cigar batches (tests/test_sw_band_cigar_sanitizers.py): plan-only creates
 * (agx_sw_batch_create_align_band_cigar with ctx == NULL) over odd shapes, the chunk bound of the traced pairs, and the band-aware
 * CIGAR check fed good and deliberately malformed operation lists, under AddressSanitizer + UBSan.  No device is touched: upload,
 * traced fill and walk need one and run under no sanitizer.
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

static uint32_t rnd_state = 4711u;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* n pairs: la uniform in lo..hi, lb within max_diff of it (clamped); every sequence starts at offset 0 of one shared block */
static void plan(int mode, int band, int64_t n, uint32_t lo, uint32_t hi, uint32_t max_diff, int expect)
{
    uint8_t *bases = (uint8_t *)malloc((size_t)hi + 1);
    uint64_t *off = (uint64_t *)calloc((size_t)(2 * n + 1), sizeof *off);
    uint32_t *len = (uint32_t *)calloc((size_t)(2 * n + 1), sizeof *len);
    if (!bases || !off || !len) {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    for (uint32_t k = 0; k <= hi; k++) bases[k] = (uint8_t)"ACGT"[rnd() & 3];
    int64_t cells = 0;
    for (int64_t p = 0; p < n; p++) {
        const uint32_t la = lo + rnd() % (hi - lo + 1);
        uint32_t lb = la + rnd() % (2 * max_diff + 1);
        lb = lb > max_diff ? lb - max_diff : 0;
        if (lb > hi) lb = hi;
        if (lb < lo) lb = lo;
        len[2 * p] = la;
        len[2 * p + 1] = lb;
        cells += (int64_t)la * lb;
    }
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_cigar(NULL, NULL, mode, band, bases, off, len, n, &b);
    EXPECT(rc == expect);
    if (rc != expect) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == AGX_E_NODEVICE);
        agx_sw_cigar_info ci;
        EXPECT(agx_sw_batch_cigar_info(b, &ci) == AGX_OK && ci.n_chunks == 0 && ci.n_traced == 0);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
    } else
        EXPECT(rc != AGX_OK);
    free(bases);
    free(off);
    free(len);
}

/* the bound by its definition: the worst of the four tilings' directions, rounded up to four dwords, plus the slot */
static uint64_t bound_by_hand(uint32_t width, uint32_t ca, uint32_t cb)
{
    static const uint32_t classes[4] = {4, 8, 16, 32};
    uint64_t worst = 0;
    for (int c = 0; c < 4; c++) {
        const uint64_t K = classes[c], G = (width + K - 1) / K;
        if (G > 64) continue;
        const uint64_t dwords = (((uint64_t)cb + G) * G * ((K + 7) / 8) + 3) & ~(uint64_t)3;
        if (dwords > worst) worst = dwords;
    }
    return 4 * (worst + ca + cb);
}

#define OP(n, c) ((uint32_t)(n) << 4 | (uint32_t)(c))

int main(void)
{
    static const int modes[2] = {AGX_SW_MODE_GLOBAL, AGX_SW_MODE_EXTEND};
    for (int m = 0; m < 2; m++) {
        const int mode = modes[m];
        plan(mode, 0, 0, 1, 1, 0, AGX_OK);
        plan(mode, 0, 1, 0, 0, 0, AGX_OK);
        plan(mode, 3, 7, 0, 1, 1, AGX_OK);
        for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
            if (band < 1023) plan(mode, band, 1500, 0, 40, 5, AGX_OK);
            plan(mode, band, 300, 100, 3000, 0, AGX_OK);
        }
        plan(mode, 16, 30000, 149, 151, 1, AGX_OK);
        plan(mode, 40, 2048, 31, 2999, 299, AGX_OK);
        plan(mode, 8, 3, 65535, 65535, 0, AGX_OK);
        plan(mode, 8, 3, 65536, 65536, 0, AGX_E_LIMIT);
        plan(mode, 1024, 3, 10, 10, 0, AGX_E_LIMIT);
        plan(mode, -1, 3, 10, 10, 0, AGX_E_ARG);
    }
    plan(AGX_SW_MODE_GLOBAL, 0, 4096, 300, 2347, 2047, AGX_OK); /* every width 1..2048 */
    plan(AGX_SW_MODE_GLOBAL, 1100, 4096, 300, 2347, 2047, AGX_E_LIMIT);
    plan(AGX_SW_MODE_LOCAL, 4, 3, 10, 10, 0, AGX_E_ARG);
    plan(AGX_SW_MODE_FIT, 4, 3, 10, 10, 0, AGX_E_ARG);
    plan(AGX_SW_MODE_EXTEND_QUERY, 4, 3, 10, 10, 0, AGX_E_ARG);
    plan(7, 4, 3, 10, 10, 0, AGX_E_ARG);
    agx_sw_batch *b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_cigar(NULL, NULL, AGX_SW_MODE_GLOBAL, 4, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    agx_sw_hit h;
    uint64_t op_off[1];
    EXPECT(agx_sw_align_band_cigar(NULL, NULL, AGX_SW_MODE_GLOBAL, 4, NULL, NULL, NULL, 0, &h, op_off, NULL, 0) == AGX_E_NODEVICE);

    /* the chunk bound: every width, rows at the edges of the range */
    static const uint32_t rows[] = {0, 1, 2, 3, 63, 64, 65, 150, 9999, 65534, 65535};
    for (int32_t width = 1; width <= AGX_SW_BAND_MAX_WIDTH; width++)
        for (size_t r = 0; r < sizeof rows / sizeof rows[0]; r++) {
            const uint32_t cb = rows[r], ca = rows[(r + (uint32_t)width) % (sizeof rows / sizeof rows[0])];
            EXPECT(agx_sw_band_cigar_bytes_bound(width, ca, cb) == bound_by_hand((uint32_t)width, ca, cb));
        }
    EXPECT(agx_sw_band_cigar_bytes_bound(0, 1, 1) == 0 && agx_sw_band_cigar_bytes_bound(-5, 1, 1) == 0);
    EXPECT(agx_sw_band_cigar_bytes_bound(AGX_SW_BAND_MAX_WIDTH + 1, 1, 1) == 0);
    EXPECT(agx_sw_band_cigar_bytes_bound(2048, 65535, 65535) == 4ull * ((65535ull + 64) * 64 * 4 + 2 * 65535ull));

    /* the band-aware check: good lists ... */
    {
        const uint32_t good[] = {OP(4, AGX_CIGAR_EQ), OP(3, AGX_CIGAR_INS), OP(4, AGX_CIGAR_EQ), OP(1, AGX_CIGAR_DIFF), OP(2, AGX_CIGAR_DEL)};
        EXPECT(agx_sw_cigar_in_band(good, 5, 0, 3) == 1);
        EXPECT(agx_sw_cigar_in_band(good, 5, -7, 3) == 1);
        EXPECT(agx_sw_cigar_in_band(good, 5, 0, 2) == 0); /* the run of I ends on diagonal 3 */
        EXPECT(agx_sw_cigar_in_band(good, 2, 0, 3) == 1); /* a prefix */
        EXPECT(agx_sw_cigar_in_band(good, 0, 0, 0) == 1);
        EXPECT(agx_sw_cigar_in_band(NULL, 0, -1, 1) == 1);
        const uint32_t down[] = {OP(65535, AGX_CIGAR_DEL), OP(65535, AGX_CIGAR_INS)};
        EXPECT(agx_sw_cigar_in_band(down, 2, -65535, 0) == 1 && agx_sw_cigar_in_band(down, 2, -65534, 0) == 0);
        EXPECT(agx_sw_cigar_in_band(down + 1, 1, 0, 65534) == 0);
    }
    /* ... and malformed ones: foreign op codes, the longest length a word holds, an origin outside the band, NULL with a count */
    {
        const uint32_t m_op[] = {OP(3, 0)}, s_op[] = {OP(3, 4)}, wild[] = {0xffffffffu}, zero[] = {0u};
        EXPECT(agx_sw_cigar_in_band(m_op, 1, -5, 5) == 0);
        EXPECT(agx_sw_cigar_in_band(s_op, 1, -5, 5) == 0);
        EXPECT(agx_sw_cigar_in_band(wild, 1, -5, 5) == 0);
        EXPECT(agx_sw_cigar_in_band(zero, 1, -5, 5) == 0);
        const uint32_t huge[] = {OP(0xfffffff, AGX_CIGAR_INS), OP(0xfffffff, AGX_CIGAR_INS), OP(0xfffffff, AGX_CIGAR_DEL)};
        EXPECT(agx_sw_cigar_in_band(huge, 3, INT32_MIN, INT32_MAX) == 1); /* 2^29 fits 64-bit arithmetic: no wrap */
        EXPECT(agx_sw_cigar_in_band(huge, 3, -2048, 2048) == 0);
        const uint32_t eq[] = {OP(1, AGX_CIGAR_EQ)};
        EXPECT(agx_sw_cigar_in_band(eq, 1, 1, 3) == 0);
        EXPECT(agx_sw_cigar_in_band(eq, 1, -3, -1) == 0);
        EXPECT(agx_sw_cigar_in_band(NULL, 4, -5, 5) == 0);
        uint32_t *many = (uint32_t *)malloc(sizeof(uint32_t) * 100000);
        if (many) {
            for (int k = 0; k < 100000; k++) many[k] = OP(1 + rnd() % 9, (k & 1) ? AGX_CIGAR_INS : AGX_CIGAR_DEL);
            (void)agx_sw_cigar_in_band(many, 100000, -50, 50);
            EXPECT(agx_sw_cigar_in_band(many, 100000, -1000000, 1000000) == 1);
            free(many);
        }
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_CIGAR_DRIVER_OK\n");
    return 0;
}
