/*
 * Checker for alignment coordinates (tests/sw_align_ref.py compiles and loads this).  A plain row-major full-matrix
 * Gotoh that applies the contract of include/agx.h ("Alignment coordinates") BY DEFINITION: every cell of H is kept,
 * the end cell is found by scanning all of them in (b, a) order with a strict compare, the begin cell by the same
 * function on the reversed prefixes.  Written from the recurrence stated in include/agx.h (agx_sw_scoring):
 *   E[i][j] = max(H[i-1][j] + go + ge, E[i-1][j] + ge)      gap along b
 *   F[i][j] = max(H[i][j-1] + go + ge, F[i][j-1] + ge)      gap along a
 *   H[i][j] = max(0, E[i][j], F[i][j], H[i-1][j-1] + (a[j] == b[i] ? match : mismatch))
 * with H = 0 and E = F = -infinity outside the matrix; i = position in b (sequence 2p+1), j = position in a (2p).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (-(1 << 29))
static int max2(int x, int y) { return x > y ? x : y; }

/* score and end cell of a (la symbols) against b (lb symbols); returns 0, or -1 when out of memory */
static int ends_of(const uint8_t *a, int la, const uint8_t *b, int lb, int match, int mismatch, int go, int ge, int *score,
                   int *a_end, int *b_end)
{
    *score = 0;
    *a_end = *b_end = -1;
    if (la <= 0 || lb <= 0) return 0;
    const size_t W = (size_t)la + 1;
    int *H = (int *)malloc(sizeof(int) * W * ((size_t)lb + 1));
    int *E = (int *)malloc(sizeof(int) * W);
    if (!H || !E) {
        free(H);
        free(E);
        return -1;
    }
    for (size_t j = 0; j < W; j++) {
        H[j] = 0;
        E[j] = NEG;
    }
    for (int i = 1; i <= lb; i++) {
        int *row = H + (size_t)i * W;
        const int *up = row - W;
        row[0] = 0;
        int F = NEG;
        for (int j = 1; j <= la; j++) {
            E[j] = max2(up[j] + go + ge, E[j] + ge);
            F = max2(row[j - 1] + go + ge, F + ge);
            const int d = up[j - 1] + (a[j - 1] == b[i - 1] ? match : mismatch);
            row[j] = max2(max2(0, d), max2(E[j], F));
        }
    }
    /* the definition: the maximum, then the smallest b among its cells, then the smallest a */
    int best = 0;
    for (int i = 1; i <= lb; i++)
        for (int j = 1; j <= la; j++)
            if (H[(size_t)i * W + j] > best) best = H[(size_t)i * W + j];
    *score = best;
    if (best > 0) {
        int found = 0;
        for (int i = 1; i <= lb && !found; i++)
            for (int j = 1; j <= la; j++)
                if (H[(size_t)i * W + j] == best) {
                    *b_end = i - 1;
                    *a_end = j - 1;
                    found = 1;
                    break;
                }
    }
    free(H);
    free(E);
    return 0;
}

/* what: 1 = ends only (begins -1), 2 = spans */
int sw_align_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch,
                 int go, int ge, int what, hit_t *hits)
{
    for (int64_t p = 0; p < n_pairs; p++) {
        const uint8_t *a = bases + off[2 * p], *b = bases + off[2 * p + 1];
        const int la = (int)len[2 * p], lb = (int)len[2 * p + 1];
        hit_t h = {0, -1, -1, -1, -1};
        if (ends_of(a, la, b, lb, match, mismatch, go, ge, &h.score, &h.a_end, &h.b_end)) return -1;
        if (what == 2 && h.score > 0) {
            const int ra = h.a_end + 1, rb = h.b_end + 1;
            uint8_t *buf = (uint8_t *)malloc((size_t)ra + rb);
            if (!buf) return -1;
            for (int k = 0; k < ra; k++) buf[k] = a[h.a_end - k];
            for (int k = 0; k < rb; k++) buf[ra + k] = b[h.b_end - k];
            int s2, ea, eb;
            const int rc = ends_of(buf, ra, buf + ra, rb, match, mismatch, go, ge, &s2, &ea, &eb);
            free(buf);
            if (rc) return -1;
            if (s2 != h.score) return -2; /* the contract's equivalence would be broken */
            h.a_begin = h.a_end - ea;
            h.b_begin = h.b_end - eb;
        }
        hits[p] = h;
    }
    return 0;
}

/* GLOBAL affine-gap score of a against b (both non-empty), same gap model, no zero floor: an independent statement of
 * what a span is -- the span's two substrings align end to end with exactly the local score */
int sw_global_ref(const uint8_t *a, int la, const uint8_t *b, int lb, int match, int mismatch, int go, int ge, int *out)
{
    const size_t W = (size_t)la + 1;
    int *H = (int *)malloc(sizeof(int) * W * 2), *E = (int *)malloc(sizeof(int) * W);
    if (!H || !E) {
        free(H);
        free(E);
        return -1;
    }
    int *prev = H, *cur = H + W;
    prev[0] = 0;
    for (int j = 1; j <= la; j++) {
        prev[j] = go + j * ge;
        E[j] = NEG;
    }
    for (int i = 1; i <= lb; i++) {
        cur[0] = go + i * ge;
        int F = NEG;
        for (int j = 1; j <= la; j++) {
            E[j] = max2(prev[j] + go + ge, E[j] + ge);
            F = max2(cur[j - 1] + go + ge, F + ge);
            const int d = prev[j - 1] + (a[j - 1] == b[i - 1] ? match : mismatch);
            cur[j] = max2(d, max2(E[j], F));
        }
        int *t = prev;
        prev = cur;
        cur = t;
    }
    *out = prev[la];
    free(H);
    free(E);
    return 0;
}
