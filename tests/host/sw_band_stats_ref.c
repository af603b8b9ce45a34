/*
 * Checker for the statistics of batches banded around a diagonal (tests/sw_band_stats_ref.py compiles and loads this).  It
 * applies the section "Statistics for batches banded around a diagonal" of include/agx.h BY DEFINITION and knows nothing of how
 * the device gets there: score and span of every pair come from the band-diag checker (the caller passes its hits in); this file
 * runs a row-major Gotoh with BOTH ENDS PINNED over a[a_begin..a_end] x b[b_begin..b_end] on the tuple (score, matches, pairs),
 * through IN-BAND CELLS ONLY, and reports
 *   smax = the lexicographic maximum of (matches, pairs) over the in-band alignments of that span that attain the best score
 *   smin = the lexicographic minimum over the same alignments (where it differs from smax the tie rule is exercised)
 * and fails (-2) when the best in-band score of the span is not the hit's score.
 * Span cell (i, j) -- i symbols of b and j of a consumed, 0 <= i <= cb, 0 <= j <= ca -- is cell (b_begin + i, a_begin + j) of the
 * full matrix and exists iff c - w <= (a_begin + j) - (b_begin + i) <= c + w.  Like sw_band_diag_ref.c every neighbour is asked
 * whether it exists before it is read; one that does not counts as minus infinity:
 *   E[i][j] = max(D[i-1][j] + go + ge, E[i-1][j] + ge)   if (i-1, j) exists                          gap along b
 *   F[i][j] = max(D[i][j-1] + go + ge, F[i][j-1] + ge)   if (i, j-1) exists                          gap along a
 *   D[i][j] = max(E, F, D[i-1][j-1] + (a == b ? match : mismatch) if i, j >= 1; the pair counts, and is a match if a == b)
 *   D[0][0] = (0, 0, 0); the answer is D[cb][ca].
 * A span with an empty side pairs nothing: {0, 0}; its score (one gap, or 0) is not checked here -- the lone run is the band-diag
 * checker's business.  Arithmetic is 64-bit.  Memory is two rows of ca + 1 tuples, time cb x width.
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
    int64_t s; /* score */
    int64_t l; /* sign * (matches << 20 | pairs): the tie-break, larger is better */
} tup_t;

#define NEG (INT64_MIN / 4)
#define REACHED(t) ((t).s > NEG / 2)
static tup_t best2(tup_t x, tup_t y) { return (x.s > y.s || (x.s == y.s && x.l >= y.l)) ? x : y; }
static tup_t plus(tup_t x, int64_t s, int64_t l)
{
    tup_t r = {x.s + s, x.l + l};
    if (!REACHED(x)) {
        r.s = NEG;
        r.l = 0;
    }
    return r;
}

/* sign = +1: most matches, then most pairs; -1: fewest, then fewest.  dlo, dhi: the band in span coordinates (j - i).
 * Returns 0, -1 out of memory, -2 the corner is not reached. */
static int pinned(const uint8_t *a, int64_t ca, const uint8_t *b, int64_t cb, int match, int mismatch, int go, int ge, int64_t dlo, int64_t dhi,
                  int sign, int64_t *out_score, stat_t *out)
{
    const size_t n = (size_t)ca + 1;
    tup_t *D = (tup_t *)malloc(sizeof(tup_t) * 2 * n), *E = (tup_t *)malloc(sizeof(tup_t) * 2 * n);
    if (!D || !E) {
        free(D);
        free(E);
        return -1;
    }
    const tup_t neg = {NEG, 0};
    tup_t corner = neg;
    for (int64_t i = 0; i <= cb; i++) {
        tup_t *row = D + (size_t)(i & 1) * n, *erow = E + (size_t)(i & 1) * n;
        const tup_t *up = D + (size_t)((i + 1) & 1) * n, *eup = E + (size_t)((i + 1) & 1) * n;
        const int64_t jlo = i + dlo > 0 ? i + dlo : 0, jhi = i + dhi < ca ? i + dhi : ca;
        tup_t F = neg;
        for (int64_t j = jlo; j <= jhi; j++) {
            const int64_t d = j - i;
            const int has_up = i > 0 && d + 1 <= dhi, has_left = j > 0 && d - 1 >= dlo, has_diag = i > 0 && j > 0;
            const tup_t e = has_up ? best2(plus(up[j], (int64_t)go + ge, 0), plus(eup[j], ge, 0)) : neg;
            F = has_left ? best2(plus(row[j - 1], (int64_t)go + ge, 0), plus(F, ge, 0)) : neg;
            tup_t v = best2(e, F);
            if (has_diag) {
                const int same = a[j - 1] == b[i - 1];
                v = best2(v, plus(up[j - 1], same ? match : mismatch, sign * ((same ? ((int64_t)1 << 20) : 0) + 1)));
            }
            if (i == 0 && j == 0) {
                v.s = 0;
                v.l = 0;
            }
            if (!REACHED(v)) v = neg;
            erow[j] = e;
            row[j] = v;
            if (i == cb && j == ca) corner = v;
        }
    }
    free(D);
    free(E);
    if (!REACHED(corner)) return -2;
    const int64_t l = sign * corner.l;
    *out_score = corner.s;
    out->matches = (int32_t)(l >> 20);
    out->pairs = (int32_t)(l & ((1 << 20) - 1));
    return 0;
}

/* -2: the span's best pinned in-band score is not the hit's (or its corner is not reached); -3: a span outside its sequences or
 * a begin cell outside the band */
int sw_band_stats_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                      int band, const int32_t *diag, const hit_t *hits, stat_t *smax, stat_t *smin)
{
    if (band < 0) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const hit_t h = hits[p];
        const int64_t la = len[2 * p], lb = len[2 * p + 1], c = diag ? diag[p] : 0;
        const int64_t ca = h.a_begin >= 0 && h.a_end >= h.a_begin ? (int64_t)h.a_end - h.a_begin + 1 : 0;
        const int64_t cb = h.b_begin >= 0 && h.b_end >= h.b_begin ? (int64_t)h.b_end - h.b_begin + 1 : 0;
        smax[p].matches = smax[p].pairs = smin[p].matches = smin[p].pairs = 0;
        if ((ca && h.a_end >= la) || (cb && h.b_end >= lb)) return -3;
        if (!ca || !cb) continue; /* nothing paired */
        const int64_t delta = (int64_t)h.a_begin - h.b_begin; /* span cell (i, j) lies on diagonal j - i + delta of the full matrix */
        const int64_t dlo = c - band - delta, dhi = c + band - delta;
        if (dlo > 0 || dhi < 0) return -3;
        const uint8_t *a = bases + off[2 * p] + h.a_begin, *b = bases + off[2 * p + 1] + h.b_begin;
        int64_t s1 = 0, s2 = 0;
        int rc = pinned(a, ca, b, cb, match, mismatch, go, ge, dlo, dhi, 1, &s1, &smax[p]);
        if (!rc) rc = pinned(a, ca, b, cb, match, mismatch, go, ge, dlo, dhi, -1, &s2, &smin[p]);
        if (rc) return rc;
        if (s1 != h.score || s2 != h.score) return -2;
    }
    return 0;
}
