/*
 * Host-only driver for the sanitizer build of the banded planner (tests/test_sw_band_sanitizers.py): plan-only banded batches
 * (agx_sw_batch_create_align_band with ctx == NULL) over many shapes under AddressSanitizer + UBSan -- limits, band, lane
 * tiling, the sort, waves, group records and image offsets.  No device is touched.
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

static uint32_t rnd_state = 12345u;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* n pairs: la uniform in lo..hi, lb within max_diff of it (clamped to lo..hi); every sequence starts at offset 0 of one shared
 * block -- a plan-only create reads no symbol */
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
    const int rc = agx_sw_batch_create_align_band(NULL, NULL, mode, band, bases, off, len, n, &b);
    EXPECT(rc == expect);
    if (rc != expect) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        EXPECT(agx_sw_batch_bind_scores(b, NULL) == AGX_E_NODEVICE);
        agx_sw_batch_destroy(b);
    } else
        EXPECT(rc != AGX_OK);
    free(bases);
    free(off);
    free(len);
}

int main(void)
{
    static const int modes[2] = {AGX_SW_MODE_GLOBAL, AGX_SW_MODE_EXTEND};
    for (int m = 0; m < 2; m++) {
        const int mode = modes[m];
        plan(mode, 0, 0, 1, 1, 0, AGX_OK);
        plan(mode, 0, 1, 0, 0, 0, AGX_OK);
        for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
            if (band < 1023) plan(mode, band, 3000, 0, 40, 5, AGX_OK); /* (a length difference widens a GLOBAL band) */
            plan(mode, band, 500, 100, 3000, 0, AGX_OK);
        }
        plan(mode, 16, 70000, 150, 150, 0, AGX_OK);
        plan(mode, 40, 4096, 32, 3000, 300, AGX_OK);
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
    EXPECT(agx_sw_batch_create_align_band(NULL, NULL, AGX_SW_MODE_GLOBAL, 4, NULL, NULL, NULL, 5, &b) == AGX_E_ARG && !b);
    agx_sw_hit h;
    EXPECT(agx_sw_align_band(NULL, NULL, AGX_SW_MODE_GLOBAL, 4, NULL, NULL, NULL, 0, &h) == AGX_E_NODEVICE);
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_DRIVER_OK\n");
    return 0;
}
