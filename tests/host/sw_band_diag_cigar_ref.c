/*
 * Checker for the CIGARs of batches banded around a diagonal (tests/sw_band_diag_cigar_ref.py compiles and loads this).  BY
 * DEFINITION of include/agx.h ("CIGARs for batches banded around a diagonal"), written from the contract and not from the
 * library: the span comes from the hit (tests/sw_band_diag_ref.py reports it), x = a[a_begin..a_end], y = b[b_begin..b_end];
 * cell (i, j) of the span is cell (b_begin + i, a_begin + j) of the full matrix, so with delta = a_begin - b_begin it exists iff
 * 0 <= i <= cb, 0 <= j <= ca and dlo' <= j - i <= dhi', dlo' = c - w - delta, dhi' = c + w - delta.  A full-matrix Gotoh of the
 * span's GLOBAL alignment over those cells -- H, E and F of every cell of the (cb + 1) x (ca + 1) matrix kept, cells that do not
 * exist are minus infinity and every neighbour is asked "do you exist?" before it is read -- and the walk back as the contract
 * words it: from (cb, ca) in state H; in H prefer the diagonal, then E (D), then F (I); stay in a gap only on a strict
 * improvement; state H with i == 0 emits j x I, with j == 0 i x D.  A lone run (one side of the span empty) is checked against
 * the band as well.  Arithmetic is 64-bit, so minus infinity never wraps.  For the long pairs of the tests the matrices are
 * banded IN STORAGE only (row i keeps the columns i + dlo' .. i + dhi') and kept as 32-bit words: a finite value is at most
 * 131 070 x 1000 in size, and minus infinity has a word of its own.
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
    int32_t *H, *E, *F;
} mat_t;
#define NEG32 INT32_MIN
static int32_t pack(int64_t v) { return v > NEG ? (int32_t)v : NEG32; }
static int64_t unpack(int32_t v) { return v != NEG32 ? (int64_t)v : NEG; }

static int exists(const mat_t *m, int64_t i, int64_t j)
{
    return i >= 0 && i <= m->cb && j >= 0 && j <= m->ca && j - i >= m->dlo && j - i <= m->dhi;
}
static size_t at(const mat_t *m, int64_t i, int64_t j) { return (size_t)i * (size_t)m->width + (size_t)(j - i - m->dlo); }
static int64_t getH(const mat_t *m, int64_t i, int64_t j) { return exists(m, i, j) ? unpack(m->H[at(m, i, j)]) : NEG; }
static int64_t getE(const mat_t *m, int64_t i, int64_t j) { return exists(m, i, j) ? unpack(m->E[at(m, i, j)]) : NEG; }
static int64_t getF(const mat_t *m, int64_t i, int64_t j) { return exists(m, i, j) ? unpack(m->F[at(m, i, j)]) : NEG; }
static int64_t plus(int64_t v, int64_t c) { return v > NEG ? v + c : NEG; }

/* ops: written forwards from ops[0]; returns their number, -1 out of memory, -2 the corner does not give `score`, -4 the path
 * (or a lone run) meets a cell that does not exist */
static int64_t one(const uint8_t *x, int64_t ca, const uint8_t *y, int64_t cb, int64_t dlo, int64_t dhi, int match, int mismatch, int go, int ge,
                   int64_t score, uint32_t *ops)
{
    if (ca == 0 && cb == 0) return 0;
    if (ca == 0 || cb == 0) { /* a lone run from (0, 0): its far end decides, the diagonal moves one way only */
        const int64_t d = ca ? ca : -cb;
        if (0 < dlo || 0 > dhi || d < dlo || d > dhi) return -4;
        ops[0] = (uint32_t)(ca ? ca : cb) << 4 | (ca ? 1u : 2u);
        return 1;
    }
    mat_t m = {ca, cb, dlo, dhi, dhi - dlo + 1, NULL, NULL, NULL};
    const int64_t o = (int64_t)go + ge, e = ge;
    const size_t cells = (size_t)(cb + 1) * (size_t)m.width;
    m.H = (int32_t *)malloc(sizeof(int32_t) * cells);
    m.E = (int32_t *)malloc(sizeof(int32_t) * cells);
    m.F = (int32_t *)malloc(sizeof(int32_t) * cells);
    uint32_t *rev = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)ca + (size_t)cb + 1));
    int64_t n = -1;
    if (!m.H || !m.E || !m.F || !rev) goto done;
    for (int64_t i = 0; i <= cb; i++)
        for (int64_t j = (i + dlo > 0 ? i + dlo : 0); j <= ca && j <= i + dhi; j++) {
            int64_t h, ev = NEG, fv = NEG;
            if (i == 0 && j == 0) h = 0;
            else {
                ev = max2(plus(getH(&m, i - 1, j), o), plus(getE(&m, i - 1, j), e));
                fv = max2(plus(getH(&m, i, j - 1), o), plus(getF(&m, i, j - 1), e));
                const int64_t s = i > 0 && j > 0 ? plus(getH(&m, i - 1, j - 1), x[j - 1] == y[i - 1] ? match : mismatch) : NEG;
                h = max2(s, max2(ev, fv));
            }
            m.H[at(&m, i, j)] = pack(h);
            m.E[at(&m, i, j)] = pack(ev);
            m.F[at(&m, i, j)] = pack(fv);
        }
    if (!exists(&m, 0, 0) || !exists(&m, cb, ca) || getH(&m, cb, ca) != score) {
        n = -2;
        goto done;
    }
    {
        int64_t i = cb, j = ca, k = 0;
        int state = 0;
        n = -4;
        while (i || j) {
            if (!exists(&m, i, j)) goto done;
            if (state == 0 && i == 0) {
                for (int64_t t = 0; t < j; t++) rev[k++] = 1;
                break;
            }
            if (state == 0 && j == 0) {
                for (int64_t t = 0; t < i; t++) rev[k++] = 2;
                break;
            }
            if (i == 0 || j == 0) goto done; /* a gap state on the boundary: the contract's rows and columns 0 are reached in H */
            if (state == 0) {
                const int64_t h = getH(&m, i, j);
                if (h == plus(getH(&m, i - 1, j - 1), x[j - 1] == y[i - 1] ? match : mismatch)) {
                    rev[k++] = x[j - 1] == y[i - 1] ? 7 : 8;
                    i--;
                    j--;
                } else if (h == getE(&m, i, j)) state = 1;
                else state = 2;
            } else if (state == 1) {
                rev[k++] = 2;
                state = plus(getE(&m, i - 1, j), e) > plus(getH(&m, i - 1, j), o) ? 1 : 0;
                i--;
            } else {
                rev[k++] = 1;
                state = plus(getF(&m, i, j - 1), e) > plus(getH(&m, i, j - 1), o) ? 2 : 0;
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
    free(m.H);
    free(m.E);
    free(m.F);
    free(rev);
    return n;
}

/* hits: what the band-diag checker reports for (mode, band, diag) with SPANS; diag: one per pair or NULL = 0; slot[p]: where
 * pair p's operations start in `wide` (room for ca + cb) */
int sw_band_diag_cigar_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go,
                           int ge, int band, const int32_t *diag, const hit_t *hits, const uint64_t *slot, uint32_t *wide, uint32_t *count)
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
                              c + band - delta, match, mismatch, go, ge, h->score, wide + slot[p]);
        if (n < 0) return (int)n;
        count[p] = (uint32_t)n;
    }
    return 0;
}
