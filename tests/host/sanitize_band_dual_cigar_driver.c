/*
 * Host-only driver for the sanitizer build of the host side of cigar batches banded around a diagonal under two-piece gap costs
 * (tests/test_sw_band_dual_cigar_sanitizers.py): plan-only creates (agx_sw_batch_create_align_band_diag_dual_cigar with
 * ctx == NULL) over odd shapes, the chunk bound with eight bits a cell (agx_sw_band_dual_cigar_bytes_bound) against its formula,
 * and the literal rescoring of the host's check (agx_sw_cigar_rescore_dual) on good and malformed operation lists, under
 * AddressSanitizer + UBSan.  No device is touched: upload, traced fill and walk run under no sanitizer.
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

static void one(int mode, int band, int use_diag, int32_t c, uint32_t la, uint32_t lb, int expect)
{
    const uint64_t off[2] = {0, 0};
    const uint32_t len[2] = {la, lb};
    agx_sw_batch *b = NULL;
    const int rc = agx_sw_batch_create_align_band_diag_dual_cigar(NULL, &mm2, mode, band, use_diag ? &c : NULL, bases, off, len, 1, &b);
    EXPECT(rc == expect);
    if (rc != expect)
        fprintf(stderr, "  mode %d band %d diag %d lengths %u x %u: rc %d, expected %d (%s)\n", mode, band, c, la, lb, rc, expect, agx_last_error());
    if (rc == AGX_E_ARG && expect == AGX_E_ARG && mode >= 0 && mode <= 4 && band >= 0) EXPECT(strstr(agx_last_error(), "pair 0") != NULL);
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == 1 && info.cells == (int64_t)la * lb);
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
    const int rc = agx_sw_batch_create_align_band_diag_dual_cigar(NULL, &mm2, mode, band, diag, bases, off, len, n, &b);
    EXPECT(rc == AGX_OK);
    if (rc) fprintf(stderr, "  mode %d band %d n %lld lengths %u..%u: rc %d (%s)\n", mode, band, (long long)n, lo, hi, rc, agx_last_error());
    if (b) {
        agx_sw_info info;
        EXPECT(agx_sw_batch_info(b, &info) == AGX_OK && info.n_pairs == n && info.cells == cells);
        EXPECT(info.n_waves >= 0 && info.n_launches >= 0 && info.n_launches <= 4 && info.padded_cells >= 0);
        agx_sw_cigar_info ci;
        EXPECT(agx_sw_batch_cigar_info(b, &ci) == AGX_OK && ci.n_traced == 0 && ci.n_chunks == 0);
        EXPECT(agx_sw_batch_launch(b) == AGX_E_NODEVICE);
        agx_sw_hit h;
        EXPECT(agx_sw_batch_hits(b, &h) == AGX_E_NODEVICE);
        uint64_t op_off[2];
        EXPECT(agx_sw_batch_cigars(b, &h, op_off, NULL, 0) == AGX_E_NODEVICE);
        agx_sw_stat st;
        EXPECT(agx_sw_batch_stats(b, &h, &st) == AGX_E_ARG);
        int32_t stop;
        EXPECT(agx_sw_batch_zdrop_stops(b, &stop) == AGX_E_ARG);
        agx_sw_batch_destroy(b);
    }
    free(off);
    free(len);
    free(diag);
}

/* the bound's formula, class by class: eight bits a cell, K / 4 dwords a lane and step, (cb + G) G steps-times-lanes */
static uint64_t bound_by_formula(uint32_t width, uint32_t ca, uint32_t cb)
{
    static const uint32_t classes[4] = {4, 8, 16, 32};
    uint64_t worst = 0;
    for (int k = 0; k < 4; k++) {
        const uint64_t K = classes[k], G = (width + K - 1) / K;
        if (G > 64) continue;
        const uint64_t dw = (((uint64_t)cb + G) * G * (K / 4) + 3) & ~(uint64_t)3;
        if (dw > worst) worst = dw;
    }
    return 4 * (worst + ca + cb);
}

#define OP(len, op) ((uint32_t)(len) << 4 | (uint32_t)(op))

int main(void)
{
    for (size_t k = 0; k < sizeof bases; k++) bases[k] = (uint8_t)"ACGT"[rnd() & 3];
    for (int mode = 0; mode <= 4; mode++) {
        many(mode, 0, 0, 1, 1);
        for (int band = 0; band <= 1023; band = band * 2 + 1) { /* 0, 1, 3, ... 1023: every class edge */
            many(mode, band, 1500, 0, 40);
            many(mode, band, 200, 97, 3001);
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
        one(mode, 4, 0, 0, 10, 10, AGX_OK); /* diag == NULL */
    }
    one(7, 4, 1, 0, 10, 10, AGX_E_ARG);
    agx_sw_batch *b = (agx_sw_batch *)1;
    const uint64_t off[2] = {0, 100};
    const uint32_t len[2] = {40, 50};
    EXPECT(agx_sw_batch_create_align_band_diag_dual_cigar(NULL, NULL, AGX_SW_MODE_FIT, 16, NULL, bases, off, len, 1, &b) == AGX_E_ARG && !b);
    EXPECT(agx_sw_batch_create_align_band_diag_dual_cigar(NULL, &mm2, AGX_SW_MODE_FIT, 16, NULL, bases, off, len, 1, NULL) == AGX_E_ARG);
    agx_sw_scoring_dual bad = mm2;
    bad.gap_extend2 = 1;
    b = (agx_sw_batch *)1;
    EXPECT(agx_sw_batch_create_align_band_diag_dual_cigar(NULL, &bad, AGX_SW_MODE_FIT, 16, NULL, bases, off, len, 1, &b) == AGX_E_LIMIT && !b);
    agx_sw_hit h;
    uint64_t oo[2];
    EXPECT(agx_sw_align_band_diag_dual_cigar(NULL, &mm2, AGX_SW_MODE_FIT, 4, NULL, NULL, NULL, NULL, 0, &h, oo, NULL, 0) == AGX_E_NODEVICE);

    /* the bound */
    EXPECT(agx_sw_band_dual_cigar_bytes_bound(0, 10, 10) == 0 && agx_sw_band_dual_cigar_bytes_bound(2049, 10, 10) == 0);
    EXPECT(agx_sw_band_dual_cigar_bytes_bound(-1, 10, 10) == 0);
    for (int k = 0; k < 20000; k++) {
        const uint32_t width = 1 + rnd() % 2048, ca = rnd() % 65536, cb = rnd() % 65536;
        EXPECT(agx_sw_band_dual_cigar_bytes_bound((int32_t)width, ca, cb) == bound_by_formula(width, ca, cb));
    }
    EXPECT(agx_sw_band_dual_cigar_bytes_bound(2048, 65535, 65535) == 4 * ((uint64_t)(65535 + 64) * 64 * 8 + 2 * 65535));

    /* the literal rescoring: x = ACGTACGTAC.., a gap of 30 costs piece 2 (-54), of 3 piece 1 (-10), of 20 either (-44) */
    uint8_t x[128], y[128];
    for (int k = 0; k < 128; k++) x[k] = y[k] = (uint8_t)"ACGT"[k & 3];
    {
        const uint32_t ops[3] = {OP(40, 7), OP(30, 1), OP(40, 7)}; /* 40= 30I 40=: a of 110 (period 4: 30 symbols shift by 2) */
        uint8_t a[110];
        for (int k = 0; k < 40; k++) a[k] = y[k];
        for (int k = 0; k < 30; k++) a[40 + k] = 'T';
        for (int k = 0; k < 40; k++) a[70 + k] = y[40 + k];
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, 3, a, 110, y, 80, 160 - 54) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, 3, a, 110, y, 80, 160 - 64) == 0); /* the piece-1 cost of 30 */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, 3, a, 110, y, 79, 160 - 54) == 0); /* does not consume y */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, 2, a, 110, y, 80, 160 - 54) == 0);
        const uint32_t split[4] = {OP(40, 7), OP(10, 1), OP(20, 1), OP(40, 7)}; /* equal neighbours: not maximal runs */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, split, 4, a, 110, y, 80, 160 - 54) == 0);
        const uint32_t wrong[3] = {OP(40, 8), OP(30, 1), OP(40, 7)}; /* X over equal symbols */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, wrong, 3, a, 110, y, 80, 160 - 54) == 0);
        const uint32_t zero[3] = {OP(40, 7), OP(0, 1), OP(40, 7)};
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, zero, 3, a, 110, y, 80, 160) == 0);
        const uint32_t op9[1] = {OP(80, 9)};
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, op9, 1, y, 80, y, 80, 160) == 0);
        const uint32_t over[1] = {OP(200, 7)}; /* runs past both sides: refused before a symbol is read */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, over, 1, y, 80, y, 80, 400) == 0);
    }
    {
        const uint32_t d3[3] = {OP(4, 7), OP(3, 2), OP(5, 7)}, d20[1] = {OP(20, 2)}, i19[1] = {OP(19, 1)}, i21[1] = {OP(21, 1)};
        uint8_t t[12];
        memcpy(t, x, 4);
        memcpy(t + 4, "GGG", 3);
        memcpy(t + 7, x + 4, 5);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, d3, 3, x, 9, t, 12, 18 - 10) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, d20, 1, NULL, 0, y, 20, -44) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, i19, 1, x, 19, NULL, 0, -42) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, i21, 1, x, 21, NULL, 0, -45) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, i21, 1, x, 21, NULL, 0, -46) == 0);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, NULL, 0, NULL, 0, NULL, 0, 0) == 1); /* "*" */
        EXPECT(agx_sw_cigar_rescore_dual(NULL, i21, 1, x, 21, NULL, 0, -45) == 0);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, NULL, 1, x, 21, NULL, 0, -45) == 0);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, i21, 1, NULL, 21, NULL, 0, -45) == 0);
    }
    /* random well-formed lists rescored here, and the same with one operation damaged */
    for (int k = 0; k < 3000; k++) {
        uint32_t ops[16];
        uint8_t a[600], t[600];
        uint32_t ca = 0, cb = 0, prev = 0;
        int64_t score = 0;
        const int n = 1 + (int)(rnd() % 12);
        int m = 0;
        for (int q = 0; q < n; q++) {
            uint32_t op;
            do op = (const uint32_t[]){1, 2, 7, 8}[rnd() & 3];
            while (op == prev);
            prev = op;
            const uint32_t l = 1 + rnd() % 40;
            for (uint32_t s = 0; s < l; s++) {
                const uint8_t cx = (uint8_t)"ACGT"[rnd() & 3];
                if (op != 2) a[ca] = cx;
                if (op == 7) t[cb] = cx;
                if (op == 8) t[cb] = cx == 'A' ? 'C' : 'A';
                if (op == 2) t[cb] = cx;
                if (op != 2) ca++;
                if (op != 1) cb++;
            }
            const int64_t p1 = mm2.gap_open + (int64_t)l * mm2.gap_extend, p2 = mm2.gap_open2 + (int64_t)l * mm2.gap_extend2;
            score += op == 7 ? (int64_t)l * mm2.match : op == 8 ? (int64_t)l * mm2.mismatch : p1 > p2 ? p1 : p2;
            ops[m++] = OP(l, op);
        }
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, (uint64_t)m, a, ca, t, cb, (int32_t)score) == 1);
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, (uint64_t)m, a, ca, t, cb, (int32_t)score + 1) == 0);
        const int q = (int)(rnd() % (uint32_t)m);
        ops[q] += 16; /* one symbol more than there is */
        EXPECT(agx_sw_cigar_rescore_dual(&mm2, ops, (uint64_t)m, a, ca, t, cb, (int32_t)score) == 0);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("SANITIZE_BAND_DUAL_CIGAR_DRIVER_OK\n");
    return 0;
}
