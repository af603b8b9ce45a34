/*
 * Checker for the CIGARs of batches banded around a diagonal under two-piece gap costs (tests/sw_band_dual_cigar_ref.py compiles
 * and loads this).  BY DEFINITION of include/agx.h ("CIGARs for batches banded around a diagonal under two-piece gap costs"),
 * written from the contract and not from the library: the span comes from the hit (tests/sw_band_dual_ref.py reports it),
 * x = a[a_begin..a_end], y = b[b_begin..b_end]; cell (i, j) of the span is cell (b_begin + i, a_begin + j) of the full matrix, so
 * with delta = a_begin - b_begin it exists iff 0 <= i <= cb, 0 <= j <= ca and dlo' <= j - i <= dhi', dlo' = c - w - delta,
 * dhi' = c + w - delta.  A five-state Gotoh of the span's GLOBAL alignment over those cells -- H, E1, F1, E2, F2 of every cell
 * kept, cells that do not exist are minus infinity and every neighbour is asked "do you exist?" before it is read -- and the
 * walk back as the contract words it: from (cb, ca) in state H; in H prefer the diagonal move, else E if max(E1, E2) >=
 * max(F1, F2), else F, within the direction piece 1 if its value is >= piece 2's; stay in a gap state of piece p only where that
 * piece's extension is strictly better than opening from H of the neighbour under that piece; state H with i == 0 emits j x I,
 * with j == 0 i x D.  A lone run (one side of the span empty) is checked against the band as well.  Arithmetic is 64-bit, so
 * minus infinity never wraps.  The matrices are banded IN STORAGE only (row i keeps the columns i + dlo' .. i + dhi') and kept
 * as 32-bit words: a finite value is at most 131 070 x 1000 in size, and minus infinity has a word of its own.
 * `seen` collects what the walks met: bit 0 a diagonal move, bits 1-4 H sourced from E1, F1, E2, F2, bits 5-8 a stay in E1, F1,
 * E2, F2 (an "extended" decision that came out true).
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (INT64_MIN / 4)
static int64_t max2(int64_t x, int64_t y) { return x > y ? x : y; }

typedef struct {
    int64_t ca, cb, dlo, dhi, width;
    int32_t *v[5]; /* H, E1, F1, E2, F2 */
} mat_t;
#define NEG32 INT32_MIN
static int32_t pack(int64_t v) { return v > NEG ? (int32_t)v : NEG32; }
static int64_t unpack(int32_t v) { return v != NEG32 ? (int64_t)v : NEG; }

static int exists(const mat_t *m, int64_t i, int64_t j)
{
    return i >= 0 && i <= m->cb && j >= 0 && j <= m->ca && j - i >= m->dlo && j - i <= m->dhi;
}
static size_t at(const mat_t *m, int64_t i, int64_t j) { return (size_t)i * (size_t)m->width + (size_t)(j - i - m->dlo); }
static int64_t get(const mat_t *m, int s, int64_t i, int64_t j) { return exists(m, i, j) ? unpack(m->v[s][at(m, i, j)]) : NEG; }
static int64_t plus(int64_t v, int64_t c) { return v > NEG ? v + c : NEG; }

enum { H = 0, E1 = 1, F1 = 2, E2 = 3, F2 = 4 };

/* ops: written forwards from ops[0]; returns their number, -1 out of memory, -2 the corner does not give `score`, -4 the path
 * (or a lone run) meets a cell that does not exist */
static int64_t one(const uint8_t *x, int64_t ca, const uint8_t *y, int64_t cb, int64_t dlo, int64_t dhi, const int *sc, int64_t score, uint32_t *ops,
                   uint32_t *seen)
{
    if (ca == 0 && cb == 0) return 0;
    if (ca == 0 || cb == 0) { /* a lone run from (0, 0): its far end decides, the diagonal moves one way only */
        const int64_t d = ca ? ca : -cb;
        if (0 < dlo || 0 > dhi || d < dlo || d > dhi) return -4;
        ops[0] = (uint32_t)(ca ? ca : cb) << 4 | (ca ? 1u : 2u);
        return 1;
    }
    const int match = sc[0], mismatch = sc[1];
    const int64_t o[3] = {0, (int64_t)sc[2] + sc[3], (int64_t)sc[4] + sc[5]}, e[3] = {0, sc[3], sc[5]}; /* [piece]: first cell, extension */
    mat_t m = {ca, cb, dlo, dhi, dhi - dlo + 1, {NULL, NULL, NULL, NULL, NULL}};
    const size_t cells = (size_t)(cb + 1) * (size_t)m.width;
    int64_t n = -1;
    uint32_t *rev = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)ca + (size_t)cb + 1));
    for (int s = 0; s < 5; s++) m.v[s] = (int32_t *)malloc(sizeof(int32_t) * cells);
    if (!m.v[0] || !m.v[1] || !m.v[2] || !m.v[3] || !m.v[4] || !rev) goto done;
    for (int64_t i = 0; i <= cb; i++)
        for (int64_t j = (i + dlo > 0 ? i + dlo : 0); j <= ca && j <= i + dhi; j++) {
            int64_t v[5] = {NEG, NEG, NEG, NEG, NEG};
            if (i == 0 && j == 0) v[H] = 0;
            else {
                for (int p = 1; p <= 2; p++) {
                    const int es = p == 1 ? E1 : E2, fs = p == 1 ? F1 : F2;
                    v[es] = max2(plus(get(&m, H, i - 1, j), o[p]), plus(get(&m, es, i - 1, j), e[p]));
                    v[fs] = max2(plus(get(&m, H, i, j - 1), o[p]), plus(get(&m, fs, i, j - 1), e[p]));
                }
                const int64_t s = i > 0 && j > 0 ? plus(get(&m, H, i - 1, j - 1), x[j - 1] == y[i - 1] ? match : mismatch) : NEG;
                v[H] = max2(s, max2(max2(v[E1], v[E2]), max2(v[F1], v[F2])));
            }
            for (int s = 0; s < 5; s++) m.v[s][at(&m, i, j)] = pack(v[s]);
        }
    if (!exists(&m, 0, 0) || !exists(&m, cb, ca) || get(&m, H, cb, ca) != score) {
        n = -2;
        goto done;
    }
    {
        int64_t i = cb, j = ca, k = 0;
        int state = H;
        n = -4;
        while (i || j) {
            if (!exists(&m, i, j)) goto done;
            if (state == H && i == 0) {
                for (int64_t t = 0; t < j; t++) rev[k++] = 1;
                break;
            }
            if (state == H && j == 0) {
                for (int64_t t = 0; t < i; t++) rev[k++] = 2;
                break;
            }
            if (i == 0 || j == 0) goto done; /* a gap state on the boundary: the contract's rows and columns 0 are reached in H */
            if (state == H) {
                const int64_t h = get(&m, H, i, j);
                if (h == plus(get(&m, H, i - 1, j - 1), x[j - 1] == y[i - 1] ? match : mismatch)) {
                    rev[k++] = x[j - 1] == y[i - 1] ? 7 : 8;
                    i--;
                    j--;
                    *seen |= 1u;
                } else {
                    const int64_t e1 = get(&m, E1, i, j), e2 = get(&m, E2, i, j), f1 = get(&m, F1, i, j), f2 = get(&m, F2, i, j);
                    if (max2(e1, e2) >= max2(f1, f2)) state = e1 >= e2 ? E1 : E2;
                    else state = f1 >= f2 ? F1 : F2;
                    if (get(&m, state, i, j) != h) goto done; /* (the maximum is attained by the state the rule names) */
                    *seen |= 1u << state;
                }
            } else if (state == E1 || state == E2) {
                const int p = state == E1 ? 1 : 2;
                rev[k++] = 2;
                if (plus(get(&m, state, i - 1, j), e[p]) > plus(get(&m, H, i - 1, j), o[p])) *seen |= 1u << (4 + state);
                else state = H;
                i--;
            } else {
                const int p = state == F1 ? 1 : 2;
                rev[k++] = 1;
                if (plus(get(&m, state, i, j - 1), e[p]) > plus(get(&m, H, i, j - 1), o[p])) *seen |= 1u << (4 + state);
                else state = H;
                j--;
            }
        }
        /* reversed, equal neighbours merged into maximal runs */
        n = 0;
        for (int64_t t = k - 1; t >= 0;) {
            int64_t u = t;
            while (u >= 0 && rev[u] == rev[t]) u--;
            ops[n++] = (uint32_t)(t - u) << 4 | rev[t];
            t = u;
        }
    }
done:
    for (int s = 0; s < 5; s++) free(m.v[s]);
    free(rev);
    return n;
}

/* hits: what the two-piece checker reports for (mode, band, diag) with SPANS; diag: one per pair or NULL = 0; slot[p]: where pair
 * p's operations start in `wide` (room for ca + cb); sc: match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2 */
int sw_band_dual_cigar_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, const int *sc, int band,
                           const int32_t *diag, const hit_t *hits, const uint64_t *slot, uint32_t *wide, uint32_t *count, uint32_t *seen)
{
    if (band < 0) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const hit_t *h = &hits[p];
        const int64_t ca = h->a_begin >= 0 && h->a_end >= h->a_begin ? (int64_t)h->a_end - h->a_begin + 1 : 0;
        const int64_t cb = h->b_begin >= 0 && h->b_end >= h->b_begin ? (int64_t)h->b_end - h->b_begin + 1 : 0;
        if ((ca && h->a_end >= (int64_t)len[2 * p]) || (cb && h->b_end >= (int64_t)len[2 * p + 1])) return -5;
        const int64_t c = diag ? diag[p] : 0;
        const int64_t delta = ca || cb ? (int64_t)h->a_begin - h->b_begin : 0;
        const int64_t n = one(bases + off[2 * p] + (ca ? h->a_begin : 0), ca, bases + off[2 * p + 1] + (cb ? h->b_begin : 0), cb, c - band - delta,
                              c + band - delta, sc, h->score, wide + slot[p], seen);
        if (n < 0) return (int)n;
        count[p] = (uint32_t)n;
    }
    return 0;
}
