/*
 * Checker for the alignment modes (tests/sw_modes_ref.py compiles and loads this).  A plain row-major full-matrix Gotoh
 * that applies the table of include/agx.h ("Alignment modes") BY DEFINITION: every cell of D is kept, the reported cell
 * is found by scanning them in the order the table states.  i = symbols of b (sequence 2p+1) consumed, j = symbols of a:
 *   E[i][j] = max(D[i-1][j] + go + ge, E[i-1][j] + ge)      gap along b
 *   F[i][j] = max(D[i][j-1] + go + ge, F[i][j-1] + ge)      gap along a
 *   D[i][j] = max(E[i][j], F[i][j], D[i-1][j-1] + (a[j-1] == b[i-1] ? match : mismatch))          no zero floor
 *   D[0][0] = 0, D[0][j] = go + j ge, D[i][0] = go + i ge (start pinned) or 0 (FIT), E = -infinity on row 0, F in column 0.
 * Modes: 1 GLOBAL, 2 FIT, 3 EXTEND, 4 EXTEND_QUERY (0, LOCAL, is tests/host/sw_align_ref.c).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (-(1 << 29))
static int max2(int x, int y) { return x > y ? x : y; }

/* score and end cell (0-based inclusive, -1 = nothing consumed); returns 0, or -1 when out of memory */
static int ends_of(const uint8_t *a, int la, const uint8_t *b, int lb, int match, int mismatch, int go, int ge, int mode, int *score,
                   int *a_end, int *b_end)
{
    const size_t W = (size_t)la + 1;
    int *D = (int *)malloc(sizeof(int) * W * ((size_t)lb + 1));
    int *E = (int *)malloc(sizeof(int) * W);
    if (!D || !E) {
        free(D);
        free(E);
        return -1;
    }
    D[0] = 0;
    E[0] = NEG;
    for (int j = 1; j <= la; j++) {
        D[j] = go + j * ge;
        E[j] = NEG;
    }
    for (int i = 1; i <= lb; i++) {
        int *row = D + (size_t)i * W;
        const int *up = row - W;
        row[0] = mode == 2 ? 0 : go + i * ge;
        int F = NEG;
        for (int j = 1; j <= la; j++) {
            E[j] = max2(up[j] + go + ge, E[j] + ge);
            F = max2(row[j - 1] + go + ge, F + ge);
            const int d = up[j - 1] + (a[j - 1] == b[i - 1] ? match : mismatch);
            row[j] = max2(d, max2(E[j], F));
        }
    }
    int bi = 0, bj = 0;
    if (mode == 1) { /* GLOBAL: the corner */
        bi = lb;
        bj = la;
    } else if (mode == 3) { /* EXTEND: the maximum anywhere, D[0][0] included; smallest i, then smallest j */
        for (int i = 0; i <= lb; i++)
            for (int j = 0; j <= la; j++)
                if (D[(size_t)i * W + j] > D[(size_t)bi * W + bj]) {
                    bi = i;
                    bj = j;
                }
    } else { /* FIT, EXTEND_QUERY: the maximum of column la; smallest i */
        bj = la;
        for (int i = 0; i <= lb; i++)
            if (D[(size_t)i * W + la] > D[(size_t)bi * W + la]) bi = i;
    }
    *score = D[(size_t)bi * W + bj];
    *a_end = bj - 1;
    *b_end = bi - 1;
    free(D);
    free(E);
    return 0;
}

/* what: 1 = ends only (begins -1), 2 = spans */
int sw_modes_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go,
                 int ge, int mode, int what, hit_t *hits)
{
    if (mode < 1 || mode > 4) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const uint8_t *a = bases + off[2 * p], *b = bases + off[2 * p + 1];
        const int la = (int)len[2 * p], lb = (int)len[2 * p + 1];
        hit_t h = {0, -1, -1, -1, -1};
        if (ends_of(a, la, b, lb, match, mismatch, go, ge, mode, &h.score, &h.a_end, &h.b_end)) return -1;
        if (what == 2 && !(mode == 3 && h.score == 0)) {
            h.a_begin = h.b_begin = 0;
            if (mode == 2 && h.b_end >= 0) { /* FIT: the latest begin = the smallest end of the reversed problem */
                const int rb = h.b_end + 1;
                uint8_t *buf = (uint8_t *)malloc((size_t)la + rb + 1);
                if (!buf) return -1;
                for (int k = 0; k < la; k++) buf[k] = a[la - 1 - k];
                for (int k = 0; k < rb; k++) buf[la + k] = b[h.b_end - k];
                int s2, ea, eb;
                const int rc = ends_of(buf, la, buf + la, rb, match, mismatch, go, ge, 4, &s2, &ea, &eb);
                free(buf);
                if (rc) return -1;
                if (s2 != h.score || eb < 0) return -2; /* the contract's equivalence would be broken */
                h.b_begin = h.b_end - eb;
            }
        }
        hits[p] = h;
    }
    return 0;
}
