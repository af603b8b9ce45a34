/*
 * Checker for alignment statistics (tests/sw_stats_ref.py compiles and loads this).  It applies the contract of
 * include/agx.h ("Alignment statistics") BY DEFINITION and knows nothing of how the device gets there: score and span of
 * every pair come from the existing checkers (the caller passes their hits in); this file runs a plain row-major Gotoh with
 * BOTH ENDS PINNED, forward, over a[a_begin..a_end] x b[b_begin..b_end] on the tuple (score, matches, pairs) and reports
 *   smax = the lexicographic maximum of (matches, pairs) over the alignments of that span that attain the best score
 *   smin = the lexicographic minimum over the same alignments (where it differs from smax the tie rule is exercised)
 * and fails (-2) when the best score of the span is not the hit's score.  i = symbols of b consumed, j = symbols of a:
 *   E[i][j] = max(D[i-1][j] + go + ge, E[i-1][j] + ge)      gap along b
 *   F[i][j] = max(D[i][j-1] + go + ge, F[i][j-1] + ge)      gap along a
 *   D[i][j] = max(E[i][j], F[i][j], D[i-1][j-1] + sub(a[j-1], b[i-1]))       a pair; a match if the symbols are identical
 *   D[0][0] = 0, D[0][j] = go + j ge, D[i][0] = go + i ge, E = -infinity on row 0, F in column 0; the answer is D[cb][ca].
 * A span with an empty side pairs nothing: {0, 0}, its score the one gap (or 0).
 * score != NULL: sub = score[code[x]][code[y]] and "identical" means identical codes; else match / mismatch on the bytes.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;
typedef struct {
    int32_t matches, pairs;
} stat_t;
typedef struct {
    int s;     /* score */
    int64_t l; /* sign * (matches << 20 | pairs): the tie-break, larger is better */
} tup_t;

#define NEG (-(1 << 29))
static tup_t best2(tup_t x, tup_t y) { return (x.s > y.s || (x.s == y.s && x.l >= y.l)) ? x : y; }
static tup_t plus(tup_t x, int s, int64_t l)
{
    tup_t r = {x.s + s, x.l + l};
    return r;
}

/* sign = +1: most matches, then most pairs; -1: fewest matches, then fewest pairs.  Returns 0, -1 out of memory. */
static int pinned(const uint8_t *a, int ca, const uint8_t *b, int cb, int match, int mismatch, int go, int ge, const int8_t *score,
                  const uint8_t *code, int sign, int *out_score, stat_t *out)
{
    const size_t W = (size_t)ca + 1;
    tup_t *D = (tup_t *)malloc(sizeof(tup_t) * W * 2), *E = (tup_t *)malloc(sizeof(tup_t) * W);
    if (!D || !E) {
        free(D);
        free(E);
        return -1;
    }
    tup_t *prev = D, *cur = D + W;
    const tup_t neg = {NEG, 0};
    prev[0].s = 0;
    prev[0].l = 0;
    E[0] = neg;
    for (int j = 1; j <= ca; j++) {
        prev[j].s = go + j * ge;
        prev[j].l = 0;
        E[j] = neg;
    }
    for (int i = 1; i <= cb; i++) {
        cur[0].s = go + i * ge;
        cur[0].l = 0;
        tup_t F = neg;
        for (int j = 1; j <= ca; j++) {
            E[j] = best2(plus(prev[j], go + ge, 0), plus(E[j], ge, 0));
            F = best2(plus(cur[j - 1], go + ge, 0), plus(F, ge, 0));
            const uint8_t x = a[j - 1], y = b[i - 1];
            int same, sub;
            if (score) {
                same = code[x] == code[y];
                sub = score[(size_t)code[x] * 32 + code[y]];
            } else {
                same = x == y;
                sub = same ? match : mismatch;
            }
            const tup_t d = plus(prev[j - 1], sub, sign * ((same ? ((int64_t)1 << 20) : 0) + 1));
            cur[j] = best2(d, best2(E[j], F));
        }
        tup_t *t = prev;
        prev = cur;
        cur = t;
    }
    const tup_t r = prev[ca];
    const int64_t l = sign * r.l;
    *out_score = r.s;
    out->matches = (int32_t)(l >> 20);
    out->pairs = (int32_t)(l & ((1 << 20) - 1));
    free(D);
    free(E);
    return 0;
}

/* -2: the span's best pinned score is not the hit's; -3: a span outside its sequences; -4: a byte outside the alphabet */
int sw_stats_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                 const int8_t *score, const uint8_t *code, const hit_t *hits, stat_t *smax, stat_t *smin)
{
    for (int64_t p = 0; p < n_pairs; p++) {
        const hit_t h = hits[p];
        const int la = (int)len[2 * p], lb = (int)len[2 * p + 1];
        const int ca = h.a_begin >= 0 && h.a_end >= h.a_begin ? h.a_end - h.a_begin + 1 : 0;
        const int cb = h.b_begin >= 0 && h.b_end >= h.b_begin ? h.b_end - h.b_begin + 1 : 0;
        if ((ca && h.a_end >= la) || (cb && h.b_end >= lb)) return -3;
        const uint8_t *a = bases + off[2 * p] + (ca ? h.a_begin : 0), *b = bases + off[2 * p + 1] + (cb ? h.b_begin : 0);
        if (score) {
            for (int k = 0; k < ca; k++)
                if (code[a[k]] >= 32) return -4;
            for (int k = 0; k < cb; k++)
                if (code[b[k]] >= 32) return -4;
        }
        int s1 = 0, s2 = 0;
        if (pinned(a, ca, b, cb, match, mismatch, go, ge, score, code, 1, &s1, &smax[p])) return -1;
        if (pinned(a, ca, b, cb, match, mismatch, go, ge, score, code, -1, &s2, &smin[p])) return -1;
        if (s1 != h.score || s2 != h.score) return -2;
    }
    return 0;
}
