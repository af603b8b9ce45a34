/*
 * Checker for banded alignment around a diagonal UNDER TWO-PIECE GAP COSTS (tests/sw_band_dual_ref.py compiles and loads this).
 * A banded five-state Gotoh that applies the section "Banded alignment around a diagonal under two-piece gap costs" of
 * include/agx.h BY DEFINITION, written from the contract and not from the kernel or the planner: every row of the matrix is
 * visited (no trimmed rows), rolling rows indexed by the column (memory O(la), time O(lb x width)), and every neighbour is asked
 * "are you in the matrix and in the band?" before it is read -- a cell that is not does not exist and counts as minus infinity.
 * i = symbols of b (sequence 2p+1) consumed, j = symbols of a; a cell exists iff 0 <= i <= lb, 0 <= j <= la and
 * dlo = c - w <= j - i <= dhi = c + w.  For an existing cell and each piece p = 1, 2 (go_p, ge_p):
 *   Ep[i][j] = max(D[i-1][j] + go_p + ge_p, Ep[i-1][j] + ge_p)   if (i-1, j) exists, else minus infinity      gap along b
 *   Fp[i][j] = max(D[i][j-1] + go_p + ge_p, Fp[i][j-1] + ge_p)   if (i, j-1) exists, else minus infinity      gap along a
 *   D[i][j] = max(E1, F1, E2, F2, D[i-1][j-1] + (a[j-1] == b[i-1] ? match : mismatch) if i, j >= 1, START)
 *   START   = 0 at (0, 0) in the pinned modes; 0 at every (i, 0) in FIT; 0 in every cell in LOCAL (the zero floor); else nothing
 * so row 0 and column 0 come out of the recurrence over the in-band cells, and a cell that nothing reaches stays minus infinity.
 * Results by mode (0 LOCAL, 1 GLOBAL, 2 FIT, 3 EXTEND, 4 EXTEND_QUERY), over existing cells only, in (i, j) order:
 *   LOCAL, EXTEND  the first strict improvement over 0;   FIT, EXTEND_QUERY  the first strict improvement down column la;
 *   GLOBAL  the corner.  A result of minus infinity is error -2: the conditions of the header exclude it.
 * Begins (what = 2): pinned modes 0; LOCAL and FIT from this checker's OWN second fill over the reversed prefixes around the
 * mirrored centre, as the header says; a reverse score that differs is error -4.
 * Pairs with an empty side: the formulas of "Alignment modes" with the gap's two-piece cost max(go1 + L ge1, go2 + L ge2), whatever
 * the band.  Arithmetic is 64-bit: nothing wraps.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (INT64_MIN / 4)
#define REACHED(v) ((v) > NEG / 2)
static int64_t max2(int64_t x, int64_t y) { return x > y ? x : y; }

typedef struct {
    int match, mismatch, go, ge, go2, ge2;
} sc_t;

/* a and b are read forwards (rev = 0: a[j-1], b[i-1]) or as the reversed strings (rev = 1: a[la-j], b[lb-i]) */
static int fill(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, sc_t s, int mode, int64_t dlo, int64_t dhi, int rev, int64_t *score,
                int64_t *bi, int64_t *bj)
{
    const size_t n = (size_t)la + 1;
    int64_t *D = (int64_t *)malloc(sizeof(int64_t) * 2 * n), *E = (int64_t *)malloc(sizeof(int64_t) * 2 * n);
    int64_t *E2 = (int64_t *)malloc(sizeof(int64_t) * 2 * n);
    if (!D || !E || !E2) {
        free(D);
        free(E);
        free(E2);
        return -1;
    }
    const int cell_mode = mode == 0 || mode == 3, column_mode = mode == 2 || mode == 4;
    int64_t best = cell_mode ? 0 : NEG, ri = -1, rj = -1;
    for (int64_t i = 0; i <= lb; i++) {
        int64_t *row = D + (size_t)(i & 1) * n, *erow = E + (size_t)(i & 1) * n;
        const int64_t *up = D + (size_t)((i + 1) & 1) * n, *eup = E + (size_t)((i + 1) & 1) * n;
        int64_t *e2row = E2 + (size_t)(i & 1) * n;
        const int64_t *e2up = E2 + (size_t)((i + 1) & 1) * n;
        const int64_t jlo = i + dlo > 0 ? i + dlo : 0, jhi = i + dhi < la ? i + dhi : la;
        int64_t F = NEG, F2 = NEG;
        for (int64_t j = jlo; j <= jhi; j++) {
            const int64_t d = j - i;
            const int has_up = i > 0 && d + 1 <= dhi;   /* (i-1, j) lies on diagonal d + 1; j <= la holds */
            const int has_left = j > 0 && d - 1 >= dlo; /* (i, j-1) on diagonal d - 1 */
            const int has_diag = i > 0 && j > 0;        /* (i-1, j-1): the same diagonal */
            int64_t e = has_up ? max2(up[j] + s.go + s.ge, eup[j] + s.ge) : NEG;
            int64_t e2 = has_up ? max2(up[j] + s.go2 + s.ge2, e2up[j] + s.ge2) : NEG;
            F = has_left ? max2(row[j - 1] + s.go + s.ge, F + s.ge) : NEG;
            F2 = has_left ? max2(row[j - 1] + s.go2 + s.ge2, F2 + s.ge2) : NEG;
            int64_t v = max2(max2(e, F), max2(e2, F2));
            if (has_diag) {
                const uint8_t x = rev ? a[la - j] : a[j - 1], y = rev ? b[lb - i] : b[i - 1];
                v = max2(v, up[j - 1] + (x == y ? s.match : s.mismatch));
            }
            if (mode == 0 || (mode == 2 && j == 0) || (i == 0 && j == 0)) v = max2(v, 0);
            if (e < NEG) e = NEG;
            if (F < NEG) F = NEG;
            if (e2 < NEG) e2 = NEG;
            if (F2 < NEG) F2 = NEG;
            if (v < NEG) v = NEG;
            erow[j] = e;
            e2row[j] = e2;
            row[j] = v;
            if ((cell_mode || (column_mode && j == la) || (mode == 1 && i == lb && j == la)) && REACHED(v) && v > best) {
                best = v;
                ri = i;
                rj = j;
            }
        }
    }
    free(D);
    free(E);
    free(E2);
    if (!cell_mode && !REACHED(best)) return -2;
    *score = best;
    *bi = ri;
    *bj = rj;
    return 0;
}

static int one(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, sc_t s, int mode, int what, int64_t w, int64_t c, hit_t *h)
{
    h->score = 0;
    h->a_begin = h->a_end = h->b_begin = h->b_end = -1;
    if (la == 0 || lb == 0) { /* "Alignment modes": the boundary formulas */
        const int64_t gap_a = la ? max2(s.go + la * (int64_t)s.ge, s.go2 + la * (int64_t)s.ge2) : 0;
        const int64_t gap_b = lb ? max2(s.go + lb * (int64_t)s.ge, s.go2 + lb * (int64_t)s.ge2) : 0;
        if (mode == 0 || mode == 3) return 0;
        h->a_end = (int32_t)la - 1;
        if (mode == 1) {
            h->score = (int32_t)(gap_a + gap_b);
            h->b_end = (int32_t)lb - 1;
        } else
            h->score = (int32_t)gap_a;
        if (what == 2) h->a_begin = h->b_begin = 0;
        return 0;
    }
    int64_t score, bi, bj;
    int rc = fill(a, la, b, lb, s, mode, c - w, c + w, 0, &score, &bi, &bj);
    if (rc) return rc;
    h->score = (int32_t)score;
    if ((mode == 0 || mode == 3) && score == 0) return 0; /* nothing consumed */
    h->a_end = (int32_t)bj - 1;
    h->b_end = (int32_t)bi - 1;
    if (what != 2) return 0;
    if (mode == 1 || mode == 3 || mode == 4) {
        h->a_begin = h->b_begin = 0;
        return 0;
    }
    if (mode == 2 && bi == 0) {
        h->a_begin = h->b_begin = 0;
        return 0;
    }
    /* the begin: the end cell, by the same rule, of the reversed prefixes inside the mirrored band */
    int64_t rs, rbi, rbj;
    rc = fill(a, bj, b, bi, s, mode == 2 ? 4 : 0, bj - bi - c - w, bj - bi - c + w, 1, &rs, &rbi, &rbj);
    if (rc) return rc;
    if (rs != score) return -4;
    h->a_begin = mode == 2 ? 0 : (int32_t)(bj - rbj);
    h->b_begin = (int32_t)(bi - rbi);
    return 0;
}

int sw_band_dual_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                     int go2, int ge2, int mode, int what, int band, const int32_t *diag, hit_t *hits)
{
    if (mode < 0 || mode > 4 || (what != 1 && what != 2) || band < 0) return -3;
    const sc_t s = {match, mismatch, go, ge, go2, ge2};
    for (int64_t p = 0; p < n_pairs; p++) {
        const int rc = one(bases + off[2 * p], (int64_t)len[2 * p], bases + off[2 * p + 1], (int64_t)len[2 * p + 1], s, mode, what, band,
                           diag ? diag[p] : 0, &hits[p]);
        if (rc) return rc;
    }
    return 0;
}
