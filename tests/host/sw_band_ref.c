/*
 * Checker for banded alignment (tests/sw_band_ref.py compiles and loads this).  A banded Gotoh that applies the section
 * "Banded alignment" of include/agx.h BY DEFINITION, written from the contract and not from the kernel: row by row, two
 * rolling rows indexed by the column (memory O(la), time O(lb x width)), every neighbour asked "are you in the matrix and in
 * the band?" before it is read -- a cell that is not does not exist and counts as minus infinity.
 * i = symbols of b (sequence 2p+1) consumed, j = symbols of a; a cell exists iff 0 <= i <= lb, 0 <= j <= la, dlo <= j - i <= dhi.
 *   E[i][j] = max(D[i-1][j] + go + ge, E[i-1][j] + ge)      gap along b      (nothing above: minus infinity)
 *   F[i][j] = max(D[i][j-1] + go + ge, F[i][j-1] + ge)      gap along a      (nothing to the left: minus infinity)
 *   D[i][j] = max(E[i][j], F[i][j], D[i-1][j-1] + (a[j-1] == b[i-1] ? match : mismatch))          no zero floor
 *   D[0][0] = 0, D[0][j] = go + j ge, D[i][0] = go + i ge where those cells exist; E = -infinity on row 0, F in column 0.
 * Modes: 1 GLOBAL (dlo = min(0, la - lb) - w, dhi = max(0, la - lb) + w, the corner), 3 EXTEND (dlo = -w, dhi = w, the first
 * maximum in (i, j) order, D[0][0] = 0 included).  Arithmetic is 64-bit, so minus infinity never wraps.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (INT64_MIN / 4)
static int64_t max2(int64_t x, int64_t y) { return x > y ? x : y; }

static int band_one(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, int match, int mismatch, int go, int ge, int mode, int64_t w,
                    hit_t *h)
{
    const int64_t diff = mode == 1 ? la - lb : 0;
    const int64_t dlo = (diff < 0 ? diff : 0) - w, dhi = (diff > 0 ? diff : 0) + w;
    int64_t *D = (int64_t *)malloc(sizeof(int64_t) * 2 * ((size_t)la + 1));
    int64_t *E = (int64_t *)malloc(sizeof(int64_t) * 2 * ((size_t)la + 1));
    if (!D || !E) {
        free(D);
        free(E);
        return -1;
    }
    int64_t best = 0, bi = 0, bj = 0, corner = NEG;
    for (int64_t i = 0; i <= lb; i++) {
        int64_t *row = D + (size_t)(i & 1) * ((size_t)la + 1), *erow = E + (size_t)(i & 1) * ((size_t)la + 1);
        const int64_t *up = D + (size_t)((i + 1) & 1) * ((size_t)la + 1), *eup = E + (size_t)((i + 1) & 1) * ((size_t)la + 1);
        const int64_t jlo = i + dlo > 0 ? i + dlo : 0, jhi = i + dhi < la ? i + dhi : la;
        int64_t F = NEG;
        for (int64_t j = jlo; j <= jhi; j++) {
            const int64_t d = j - i;
            const int has_up = i > 0 && d + 1 <= dhi;   /* (i-1, j) lies on diagonal d + 1 */
            const int has_left = j > 0 && d - 1 >= dlo; /* (i, j-1) on diagonal d - 1 */
            int64_t v;
            if (i == 0 && j == 0) {
                v = 0;
                erow[j] = NEG;
                F = NEG;
            } else if (i == 0) {
                v = go + j * (int64_t)ge;
                erow[j] = NEG;
                F = v;
            } else if (j == 0) {
                v = go + i * (int64_t)ge;
                erow[j] = v;
                F = NEG;
            } else {
                erow[j] = has_up ? max2(up[j] + go + ge, eup[j] + ge) : NEG;
                F = has_left ? max2(row[j - 1] + go + ge, F + ge) : NEG;
                v = max2(up[j - 1] + (a[j - 1] == b[i - 1] ? match : mismatch), max2(erow[j], F)); /* (i-1, j-1): same diagonal */
            }
            if (erow[j] < NEG) erow[j] = NEG;
            if (F < NEG) F = NEG;
            row[j] = v;
            if (mode == 3 && v > best) {
                best = v;
                bi = i;
                bj = j;
            }
            if (i == lb && j == la) corner = v;
        }
    }
    free(D);
    free(E);
    h->a_begin = h->a_end = h->b_begin = h->b_end = -1;
    if (mode == 1) {
        if (corner == NEG) return -2; /* the widened band always holds the corner */
        h->score = (int32_t)corner;
        h->a_begin = h->b_begin = 0;
        h->a_end = (int32_t)la - 1;
        h->b_end = (int32_t)lb - 1;
    } else {
        h->score = (int32_t)best;
        if (best > 0) {
            h->a_begin = h->b_begin = 0;
            h->a_end = (int32_t)bj - 1;
            h->b_end = (int32_t)bi - 1;
        }
    }
    return 0;
}

int sw_band_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                int mode, int band, hit_t *hits)
{
    if ((mode != 1 && mode != 3) || band < 0) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int rc = band_one(bases + off[2 * p], (int64_t)len[2 * p], bases + off[2 * p + 1], (int64_t)len[2 * p + 1], match, mismatch, go,
                                ge, mode, band, &hits[p]);
        if (rc) return rc;
    }
    return 0;
}
