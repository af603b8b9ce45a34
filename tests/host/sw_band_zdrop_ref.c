/*
 * Checker for z-drop termination of banded extension (tests/sw_band_zdrop_ref.py compiles and loads this).  Written from the
 * section "Z-drop for banded extension" of include/agx.h and not from the kernel: a banded Gotoh in mode EXTEND as
 * tests/host/sw_band_diag_ref.c fills it -- every row in order, two rolling rows indexed by the column, every neighbour asked
 * "are you in the matrix and in the band?" before it is read -- that applies the rule after each row.
 * i = symbols of b (sequence 2p+1) consumed, j = symbols of a; a cell exists iff 0 <= i <= lb, 0 <= j <= la and
 * dlo = c - w <= j - i <= dhi = c + w; D[0][0] = 0 and nothing else starts a path.
 * The rule: last = min(lb, la - dlo); R(i) = max D[i][j] over the existing cells of row i, c(i) the smallest j that attains it;
 * B = 0 at (bi, bj) = (0, 0); for i = 1 .. last in order: R(i) > B makes (i, c(i)) the new best and no test is made; otherwise
 * B - R(i) > zdrop + |ge| * |(i - bi) - (c(i) - bj)| terminates at row i: stop = i - 1, and later rows are not looked at.
 * term = 0 switches the second summand off (the tests use it only to prove that their inputs exercise it).
 * The hit is B with end cell (bi - 1, bj - 1), all positions -1 at score 0, begins 0 under what = 2; stop = -1 when no row
 * terminated, which includes pairs with an empty side.  A row 1 .. last without an existing cell is error -2: the admission rule
 * dlo <= 0 <= dhi excludes it.  Arithmetic is 64-bit: nothing wraps.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (INT64_MIN / 4)
#define REACHED(v) ((v) > NEG / 2)
static int64_t max2(int64_t x, int64_t y) { return x > y ? x : y; }

static int one(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, int match, int mismatch, int go, int ge, int what, int64_t dlo,
               int64_t dhi, int64_t zdrop, int term, hit_t *h, int32_t *stop)
{
    h->score = 0;
    h->a_begin = h->a_end = h->b_begin = h->b_end = -1;
    *stop = -1;
    if (la == 0 || lb == 0) return 0;
    const size_t n = (size_t)la + 1;
    int64_t *D = (int64_t *)malloc(sizeof(int64_t) * 2 * n), *E = (int64_t *)malloc(sizeof(int64_t) * 2 * n);
    if (!D || !E) {
        free(D);
        free(E);
        return -1;
    }
    const int64_t last = lb < la - dlo ? lb : la - dlo;
    int64_t B = 0, bi = 0, bj = 0;
    int rc = 0;
    for (int64_t i = 0; i <= last; i++) {
        int64_t *row = D + (size_t)(i & 1) * n, *erow = E + (size_t)(i & 1) * n;
        const int64_t *up = D + (size_t)((i + 1) & 1) * n, *eup = E + (size_t)((i + 1) & 1) * n;
        const int64_t jlo = i + dlo > 0 ? i + dlo : 0, jhi = i + dhi < la ? i + dhi : la;
        int64_t F = NEG, R = NEG, c = -1;
        for (int64_t j = jlo; j <= jhi; j++) {
            const int64_t d = j - i;
            const int has_up = i > 0 && d + 1 <= dhi;   /* (i-1, j) lies on diagonal d + 1 */
            const int has_left = j > 0 && d - 1 >= dlo; /* (i, j-1) on diagonal d - 1 */
            const int has_diag = i > 0 && j > 0;        /* (i-1, j-1): the same diagonal */
            int64_t e = has_up ? max2(up[j] + go + ge, eup[j] + ge) : NEG;
            F = has_left ? max2(row[j - 1] + go + ge, F + ge) : NEG;
            int64_t v = max2(e, F);
            if (has_diag) v = max2(v, up[j - 1] + (a[j - 1] == b[i - 1] ? match : mismatch));
            if (i == 0 && j == 0) v = max2(v, 0);
            if (e < NEG) e = NEG;
            if (F < NEG) F = NEG;
            if (v < NEG) v = NEG;
            erow[j] = e;
            row[j] = v;
            if (REACHED(v) && v > R) {
                R = v;
                c = j;
            }
        }
        if (i == 0) continue;
        if (c < 0) {
            rc = -2;
            break;
        }
        if (R > B) {
            B = R;
            bi = i;
            bj = c;
            continue;
        }
        int64_t off = (i - bi) - (c - bj);
        if (off < 0) off = -off;
        if (B - R > zdrop + (term ? (int64_t)(ge < 0 ? -ge : ge) * off : 0)) {
            *stop = (int32_t)(i - 1);
            break;
        }
    }
    free(D);
    free(E);
    if (rc) return rc;
    h->score = (int32_t)B;
    if (B == 0) return 0;
    h->a_end = (int32_t)bj - 1;
    h->b_end = (int32_t)bi - 1;
    if (what == 2) h->a_begin = h->b_begin = 0;
    return 0;
}

int sw_band_zdrop_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                      int what, int band, const int32_t *diag, int64_t zdrop, int term, hit_t *hits, int32_t *stops)
{
    if ((what != 1 && what != 2) || band < 0 || zdrop < 0) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t c = diag ? diag[p] : 0;
        if (c - band > 0 || c + band < 0) return -5; /* the band misses the origin */
        const int rc = one(bases + off[2 * p], (int64_t)len[2 * p], bases + off[2 * p + 1], (int64_t)len[2 * p + 1], match, mismatch, go, ge, what,
                           c - band, c + band, zdrop, term, &hits[p], &stops[p]);
        if (rc) return rc;
    }
    return 0;
}
