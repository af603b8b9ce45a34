/*
 * Checker for align batches under a substitution matrix (tests/sw_matrix_align_ref.py compiles and loads this).  A plain
 * row-major full-matrix Gotoh that applies the tables of include/agx.h ("Alignment coordinates", "Alignment modes") BY
 * DEFINITION, with the diagonal move adding score[code[a_j]][code[b_i]]: every cell is kept, the reported cells are found
 * by scanning them in the order the header states.  i = symbols of b (sequence 2p+1) consumed, j = symbols of a:
 *   E[i][j] = max(D[i-1][j] + go + ge, E[i-1][j] + ge)      gap along b
 *   F[i][j] = max(D[i][j-1] + go + ge, F[i][j-1] + ge)      gap along a
 *   D[i][j] = max(E[i][j], F[i][j], D[i-1][j-1] + score[code[a[j-1]]][code[b[i-1]]])   and 0 as well where there is a floor
 * Boundaries (kind): LOCAL_K  D[0][j] = D[i][0] = 0 with the zero floor;
 *                    PINNED_K D[0][j] = go + j ge, D[i][0] = go + i ge;   FREE_K the same with D[i][0] = 0 (FIT).
 * E = -infinity on row 0, F in column 0.  Modes: 0 LOCAL, 1 GLOBAL, 2 FIT, 3 EXTEND, 4 EXTEND_QUERY.
 *
 * Begin cells come from the definition too: with the end cell fixed, G[i][j] = the PINNED_K matrix of a[a_end..0] against
 * b[b_end..0] is the best score of an alignment that consumes exactly a[a_end-j+1 .. a_end] and b[b_end-i+1 .. b_end], i.e.
 * of one that begins there and ends in the end cell.  The latest begin is the smallest i, then the smallest j, with
 * G[i][j] == score (no floor, no maximum: equality with the forward score).  The header's other wording -- the end cell of
 * the reversed problem under the mode's own rule -- is evaluated beside it and must agree: -2 otherwise.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (-(1 << 29))
enum { LOCAL_K = 0, PINNED_K = 1, FREE_K = 2 };
static int max2(int x, int y) { return x > y ? x : y; }

/* all of D, (lb + 1) x (la + 1); the caller frees it.  NULL when out of memory. */
static int *fill(const uint8_t *a, int la, const uint8_t *b, int lb, const int8_t *score, const uint8_t *code, int go, int ge, int kind)
{
    const size_t W = (size_t)la + 1;
    int *D = (int *)malloc(sizeof(int) * W * ((size_t)lb + 1));
    int *E = (int *)malloc(sizeof(int) * W);
    if (!D || !E) {
        free(D);
        free(E);
        return NULL;
    }
    D[0] = 0;
    E[0] = NEG;
    for (int j = 1; j <= la; j++) {
        D[j] = kind == LOCAL_K ? 0 : go + j * ge;
        E[j] = NEG;
    }
    for (int i = 1; i <= lb; i++) {
        int *row = D + (size_t)i * W;
        const int *up = row - W;
        row[0] = kind == PINNED_K ? go + i * ge : 0;
        int F = NEG;
        for (int j = 1; j <= la; j++) {
            E[j] = max2(up[j] + go + ge, E[j] + ge);
            F = max2(row[j - 1] + go + ge, F + ge);
            const int d = up[j - 1] + score[32 * code[a[j - 1]] + code[b[i - 1]]];
            row[j] = max2(d, max2(E[j], F));
            if (kind == LOCAL_K) row[j] = max2(row[j], 0);
        }
    }
    free(E);
    return D;
}

/* the mode's score and end cell as (i, j) = symbols consumed; LOCAL with score 0 gives (0, 0) */
static void pick(const int *D, int la, int lb, int mode, int *bi, int *bj)
{
    const size_t W = (size_t)la + 1;
    *bi = *bj = 0;
    if (mode == 1) { /* GLOBAL: the corner */
        *bi = lb;
        *bj = la;
    } else if (mode == 0 || mode == 3) { /* the maximum anywhere (LOCAL: D[0][0] = 0 is its floor); smallest i, then smallest j */
        for (int i = 0; i <= lb; i++)
            for (int j = 0; j <= la; j++)
                if (D[(size_t)i * W + j] > D[(size_t)*bi * W + *bj]) {
                    *bi = i;
                    *bj = j;
                }
    } else { /* FIT, EXTEND_QUERY: the maximum of column la; smallest i */
        *bj = la;
        for (int i = 0; i <= lb; i++)
            if (D[(size_t)i * W + la] > D[(size_t)*bi * W + la]) *bi = i;
    }
}

static void reversed(uint8_t *dst, const uint8_t *src, int n)
{
    for (int k = 0; k < n; k++) dst[k] = src[n - 1 - k];
}

/* what: 1 = ends only (begins -1), 2 = spans.  Returns 0; -1 out of memory; -2 the reversed problem disagrees with the
 * definition; -3 bad mode; -4 a byte outside the alphabet */
int sw_matrix_align_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, const int8_t *score,
                        const uint8_t *code, int go, int ge, int mode, int what, hit_t *hits)
{
    if (mode < 0 || mode > 4) return -3;
    const int kind = mode == 0 ? LOCAL_K : mode == 2 ? FREE_K : PINNED_K;
    for (int64_t p = 0; p < n_pairs; p++) {
        const uint8_t *a = bases + off[2 * p], *b = bases + off[2 * p + 1];
        const int la = (int)len[2 * p], lb = (int)len[2 * p + 1];
        for (int k = 0; k < la; k++)
            if (code[a[k]] >= 32) return -4;
        for (int k = 0; k < lb; k++)
            if (code[b[k]] >= 32) return -4;
        hit_t h = {0, -1, -1, -1, -1};
        int *D = fill(a, la, b, lb, score, code, go, ge, kind);
        if (!D) return -1;
        int bi, bj;
        pick(D, la, lb, mode, &bi, &bj);
        h.score = D[(size_t)bi * ((size_t)la + 1) + bj];
        free(D);
        const int nothing = (mode == 0 || mode == 3) && h.score == 0; /* all four stay -1 */
        if (!nothing) {
            h.a_end = bj - 1;
            h.b_end = bi - 1;
        }
        if (what == 2 && !nothing) {
            h.a_begin = h.b_begin = 0;
            if ((mode == 0 || mode == 2) && h.b_end >= 0) {
                /* LOCAL: latest begin in b, then in a; FIT: all of a, latest begin in b */
                const int ra = bj, rb = bi;
                const size_t W = (size_t)ra + 1;
                uint8_t *buf = (uint8_t *)malloc((size_t)ra + rb + 1);
                if (!buf) return -1;
                reversed(buf, a, ra);
                reversed(buf + ra, b, rb);
                int *G = fill(buf, ra, buf + ra, rb, score, code, go, ge, PINNED_K);
                if (!G) {
                    free(buf);
                    return -1;
                }
                int gi = -1, gj = -1;
                for (int i = 1; i <= rb && gi < 0; i++)
                    for (int j = mode == 2 ? ra : 1; j <= ra; j++)
                        if (G[(size_t)i * W + j] == h.score) {
                            gi = i;
                            gj = j;
                            break;
                        }
                free(G);
                /* the header's other wording: the reversed problem's own end cell (LOCAL by the local rule, FIT in EXTEND_QUERY) */
                int *R = fill(buf, ra, buf + ra, rb, score, code, go, ge, mode == 0 ? LOCAL_K : PINNED_K);
                free(buf);
                if (!R) return -1;
                int ri, rj;
                pick(R, ra, rb, mode == 0 ? 0 : 4, &ri, &rj);
                const int rs = R[(size_t)ri * W + rj];
                free(R);
                if (gi < 0 || rs != h.score || ri != gi || rj != gj) return -2;
                if (mode == 0) h.a_begin = h.a_end - (gj - 1);
                h.b_begin = h.b_end - (gi - 1);
            }
        }
        hits[p] = h;
    }
    return 0;
}
