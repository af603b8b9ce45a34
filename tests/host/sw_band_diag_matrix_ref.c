/* The CHECKER for "Banded alignment around a diagonal under a substitution matrix" (include/agx.h): a banded Gotoh written from
 * the header's words alone -- the band c - w <= j - i <= c + w, the boundaries per mode, the result and tie rules, the begins
 * from its own reversed fill, and for CIGARs a full in-band fill of the span with the walk-back of "Alignment itself".  Plain
 * C99, no library code; time O(lb x width), the hits in rolling rows, the CIGAR fill in (cb + 1) x width cells.  Used by the
 * tests only (tests/sw_band_diag_matrix_ref.py). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { /* the layout of agx_sw_matrix */
    int32_t n_symbols, gap_open, gap_extend;
    uint8_t code[256];
    int8_t score[32][32];
} matrix_t;
typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

enum { LOCAL = 0, GLOBAL = 1, FIT = 2, EXTEND = 3, EXTEND_QUERY = 4 };
enum { ENDS = 1, SPANS = 2 };
enum { OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8 };

#define NEG (-((int64_t)1 << 50)) /* "does not exist"; anything below NEG / 2 is treated as such */
static int64_t lift(int64_t v) { return v < NEG / 2 ? NEG : v; }
static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

static int w_of(const matrix_t *m, uint8_t x, uint8_t y) { return m->score[m->code[x]][m->code[y]]; }

/* One banded fill in `mode` over the cells 0 <= i <= lb, 0 <= j <= la, dlo <= j - i <= dhi.  rev: the sequences are read
 * backwards from a[la - 1], b[lb - 1] (the reversed prefixes of a begin pass).  Returns 0 and the score with its end CELL (i, j)
 * by the mode's rule ((0, 0) with score 0 when LOCAL / EXTEND consume nothing), or -2 when no end cell exists. */
static int fill(const matrix_t *m, int mode, const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb, int64_t dlo, int64_t dhi, int rev,
                int64_t *score, int64_t *ei, int64_t *ej)
{
    const int64_t o = (int64_t)m->gap_open + m->gap_extend, e = m->gap_extend;
    const int64_t width = dhi - dlo + 1;
    /* slot s = j - i - dlo; one spare slot on each side stays NEG */
    int64_t *H = (int64_t *)malloc(sizeof(int64_t) * (size_t)(width + 2)), *E = (int64_t *)malloc(sizeof(int64_t) * (size_t)(width + 2));
    if (!H || !E) {
        free(H);
        free(E);
        return -1;
    }
    for (int64_t s = 0; s < width + 2; s++) H[s] = E[s] = NEG;
    int64_t best = NEG, bi = 0, bj = 0;
    if (mode == EXTEND || mode == LOCAL) best = 0; /* nothing consumed */
    int found = mode == EXTEND || mode == LOCAL;
    for (int64_t i = 0; i <= lb; i++) {
        int64_t jlo = i + dlo, jhi = i + dhi;
        if (jlo < 0) jlo = 0;
        if (jhi > la) jhi = la;
        int64_t F = NEG;
        /* a cell left of the band's first cell of this row does not exist: its H must not be read as "left".  The slot array
         * is indexed from 1; slot s of row i held (i - 1, j) in slot s + 1 and (i - 1, j - 1) in slot s before this row */
        int64_t hleft = NEG;
        for (int64_t j = i + dlo; j <= i + dhi; j++) {
            const int64_t s = j - i - dlo + 1;
            if (j < jlo || j > jhi) { /* outside the matrix: does not exist */
                /* (its slot must read as NEG for the rows below; the diagonal value it held is dropped) */
                H[s] = NEG;
                E[s] = NEG;
                hleft = NEG;
                F = NEG;
                continue;
            }
            const int64_t hdiag = H[s], hup = H[s + 1], eup = E[s + 1];
            int64_t h, ev = NEG;
            if (i > 0) ev = lift(max2(lift(hup) + o, lift(eup) + e));
            F = j > 0 ? lift(max2(lift(hleft) + o, lift(F) + e)) : NEG;
            if (i == 0 && j == 0) {
                h = 0;
            } else if (j == 0) { /* column 0 */
                h = mode == FIT || mode == LOCAL ? 0 : ev;
            } else if (i == 0) { /* row 0: the in-band chain from (0, 0) */
                h = mode == LOCAL ? 0 : F;
            } else {
                const uint8_t x = rev ? a[la - j] : a[j - 1], y = rev ? b[lb - i] : b[i - 1];
                h = lift(hdiag) == NEG ? NEG : hdiag + w_of(m, x, y);
                h = max2(h, max2(ev, F));
                if (mode == LOCAL && h < 0) h = 0;
            }
            h = lift(h);
            H[s] = h;
            E[s] = ev;
            hleft = h;
            if (h == NEG) continue;
            if (mode == LOCAL || mode == EXTEND) {
                if (h > best) { /* rows rising, columns rising: the smallest i, then the smallest j */
                    best = h;
                    bi = i;
                    bj = j;
                }
            } else if (mode == GLOBAL) {
                if (i == lb && j == la) {
                    best = h;
                    bi = i;
                    bj = j;
                    found = 1;
                }
            } else if (j == la) { /* FIT, EXTEND_QUERY: the smallest i among the maxima of column la */
                if (!found || h > best) {
                    best = h;
                    bi = i;
                    bj = j;
                    found = 1;
                }
            }
        }
    }
    free(H);
    free(E);
    if (!found) return -2;
    *score = best;
    *ei = bi;
    *ej = bj;
    return 0;
}

static int admits(int mode, int64_t la, int64_t lb, int64_t dlo, int64_t dhi)
{
    const int origin = dlo <= 0 && 0 <= dhi;
    switch (mode) {
    case GLOBAL: return origin && dlo <= la - lb && la - lb <= dhi;
    case EXTEND: return origin;
    case EXTEND_QUERY: return origin && dhi >= la - lb;
    case FIT: return dlo <= 0 && dhi >= la - lb;
    default: return 1;
    }
}

/* the hit of one pair; 0, or -3 the band does not hold what the mode needs, -2 no end cell, -4 the reverse fill disagrees */
static int one_hit(const matrix_t *m, int mode, int what, int64_t w, int64_t c, const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb,
                   hit_t *out)
{
    const int64_t dlo = c - w, dhi = c + w;
    hit_t h = {0, -1, -1, -1, -1};
    if (!admits(mode, la, lb, dlo, dhi)) return -3;
    int64_t sc = 0, i = 0, j = 0;
    if (mode == LOCAL && (la == 0 || lb == 0)) {
        *out = h;
        return 0;
    }
    if (mode == FIT && la == 0) {
        /* a pair with an empty side is answered by the formulas of "Alignment modes", whatever the band: max_i D[i][0] = 0 at
         * i = 0, also where the band leaves row 0 out (dhi < 0) and a fill would find its first in-band cell of column 0 further
         * down.  (Every other mode's fill gives its formula: the band holds the cells the formula names.) */
        h.a_end = h.b_end = -1;
        if (what == SPANS) h.a_begin = h.b_begin = 0;
        *out = h;
        return 0;
    }
    int rc = fill(m, mode, a, la, b, lb, dlo, dhi, 0, &sc, &i, &j);
    if (rc) return rc;
    h.score = (int32_t)sc;
    if ((mode == LOCAL || mode == EXTEND) && sc == 0) { /* nothing consumed: all four -1 */
        *out = h;
        return 0;
    }
    h.a_end = (int32_t)j - 1;
    h.b_end = (int32_t)i - 1;
    if (what == SPANS) {
        if (mode == LOCAL) {
            int64_t rs, ri, rj;
            rc = fill(m, LOCAL, a, j, b, i, j - i - dhi, j - i - dlo, 1, &rs, &ri, &rj); /* centre (a_end + 1) - (b_end + 1) - c */
            if (rc) return rc;
            if (rs != sc || ri < 1 || rj < 1) return -4;
            h.a_begin = (int32_t)(j - rj);
            h.b_begin = (int32_t)(i - ri);
        } else if (mode == FIT) {
            h.a_begin = 0;
            h.b_begin = 0;
            if (i > 0) {
                int64_t rs, ri, rj;
                rc = fill(m, EXTEND_QUERY, a, la, b, i, la - i - dhi, la - i - dlo, 1, &rs, &ri, &rj); /* centre la - (b_end + 1) - c */
                if (rc) return rc;
                if (rs != sc) return -4;
                h.b_begin = (int32_t)(i - ri); /* ri = 0: all of a in one gap along row b_end + 1 */
            }
        } else
            h.a_begin = h.b_begin = 0;
    }
    *out = h;
    return 0;
}

/* n pairs: bases / off / len as the library takes them (off, len: 2 n entries), diag NULL = 0 for every pair */
int sw_band_diag_matrix_ref(const matrix_t *m, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n, int mode, int what,
                            int band, const int32_t *diag, hit_t *out)
{
    for (int64_t p = 0; p < n; p++) {
        for (int q = 0; q < 2; q++) /* -5: a byte outside the alphabet (the library answers AGX_E_SYMBOL; nothing to check against) */
            for (uint32_t k = 0; k < len[2 * p + q]; k++)
                if (m->code[bases[off[2 * p + q] + k]] >= m->n_symbols) return -5;
        const int rc = one_hit(m, mode, what, band, diag ? diag[p] : 0, bases + off[2 * p], len[2 * p], bases + off[2 * p + 1], len[2 * p + 1],
                               &out[p]);
        if (rc) return rc;
    }
    return 0;
}

/* The CIGAR of one span x (ca), y (cb) inside the band lo .. hi counted from the span's begin cell: the pinned fill of "Alignment
 * itself" over the in-band cells and its walk-back.  ops: room for ca + cb words; returns the number of runs, or < 0. */
static int64_t one_cigar(const matrix_t *m, const uint8_t *x, int64_t ca, const uint8_t *y, int64_t cb, int64_t lo, int64_t hi, int64_t score,
                         uint32_t *ops)
{
    const int64_t o = (int64_t)m->gap_open + m->gap_extend, e = m->gap_extend, go = m->gap_open;
    if (ca == 0 && cb == 0) return 0;
    if (lo > 0 || hi < 0 || ca - cb < lo || ca - cb > hi) return -4;
    if (ca == 0 || cb == 0) {
        ops[0] = (uint32_t)(ca ? ca : cb) << 4 | (uint32_t)(ca ? OP_I : OP_D);
        return 1;
    }
    const int64_t W = hi - lo + 3; /* slot s = j - i - lo + 1, a spare one on each side */
    const size_t cells = (size_t)(cb + 1) * (size_t)W;
    int64_t *H = (int64_t *)malloc(sizeof(int64_t) * cells), *E = (int64_t *)malloc(sizeof(int64_t) * cells),
            *F = (int64_t *)malloc(sizeof(int64_t) * cells);
    if (!H || !E || !F) {
        free(H);
        free(E);
        free(F);
        return -1;
    }
    for (size_t k = 0; k < cells; k++) H[k] = E[k] = F[k] = NEG;
#define AT(M, i, j) M[(size_t)(i) * (size_t)W + (size_t)((j) - (i) - lo + 1)]
#define IN(i, j) ((i) >= 0 && (i) <= cb && (j) >= 0 && (j) <= ca && (j) - (i) >= lo && (j) - (i) <= hi)
    for (int64_t i = 0; i <= cb; i++)
        for (int64_t j = i + lo < 0 ? 0 : i + lo; j <= ca && j <= i + hi; j++) {
            int64_t h;
            if (i == 0 && j == 0) h = 0;
            else if (i == 0) h = go + j * e;
            else if (j == 0) h = go + i * e;
            else {
                const int64_t ev = IN(i - 1, j) ? lift(max2(lift(AT(H, i - 1, j)) + o, lift(AT(E, i - 1, j)) + e)) : NEG;
                const int64_t fv = IN(i, j - 1) ? lift(max2(lift(AT(H, i, j - 1)) + o, lift(AT(F, i, j - 1)) + e)) : NEG;
                AT(E, i, j) = ev;
                AT(F, i, j) = fv;
                h = max2(AT(H, i - 1, j - 1) + w_of(m, x[j - 1], y[i - 1]), max2(ev, fv));
            }
            AT(H, i, j) = h;
        }
    int64_t rc = 0;
    if (AT(H, cb, ca) != score) rc = -2;
    /* walk back from (cb, ca) in state H; operations come out reversed and are merged into runs */
    int64_t i = cb, j = ca, n = 0;
    int state = 0;
    uint32_t *end = ops + ca + cb, *out = end, op = 0, len = 0;
#define EMIT(O, K)                               \
    do {                                         \
        if ((uint32_t)(O) == op) len += (uint32_t)(K); \
        else {                                   \
            if (len) *--out = len << 4 | op;     \
            op = (uint32_t)(O);                  \
            len = (uint32_t)(K);                 \
        }                                        \
    } while (0)
    while (!rc && (i > 0 || j > 0)) {
        if (!IN(i, j)) {
            rc = -4;
            break;
        }
        if (state == 0) {
            if (i == 0) {
                EMIT(OP_I, j);
                break;
            }
            if (j == 0) {
                EMIT(OP_D, i);
                break;
            }
            if (AT(H, i, j) == AT(H, i - 1, j - 1) + w_of(m, x[j - 1], y[i - 1])) {
                EMIT(m->code[x[j - 1]] == m->code[y[i - 1]] ? OP_EQ : OP_X, 1);
                i--;
                j--;
            } else if (AT(H, i, j) == AT(E, i, j))
                state = 1;
            else
                state = 2;
        } else if (state == 1) {
            EMIT(OP_D, 1);
            /* (i - 1, j) exists: E of this cell is true.  Row 0 has no E: the walk goes on in H there */
            state = i - 1 > 0 && j > 0 && lift(AT(E, i - 1, j)) != NEG && AT(E, i - 1, j) + e > AT(H, i - 1, j) + o ? 1 : 0;
            i--;
        } else {
            EMIT(OP_I, 1);
            state = j - 1 > 0 && i > 0 && lift(AT(F, i, j - 1)) != NEG && AT(F, i, j - 1) + e > AT(H, i, j - 1) + o ? 2 : 0;
            j--;
        }
    }
    if (len) *--out = len << 4 | op;
    n = end - out;
    memmove(ops, out, sizeof(uint32_t) * (size_t)n);
#undef EMIT
#undef AT
#undef IN
    free(H);
    free(E);
    free(F);
    return rc ? rc : n;
}

/* n pairs with their SPANS hits: pair p's runs go to ops + slot[p] (room for ca + cb words), their number to count[p].
 * 0, or -2: the fill of a span does not give the hit's score, -4: the path or a cell of it lies outside the band */
int sw_band_diag_matrix_cigar_ref(const matrix_t *m, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n, int band,
                                  const int32_t *diag, const hit_t *hits, const uint64_t *slot, uint32_t *ops, uint32_t *count)
{
    (void)len;
    for (int64_t p = 0; p < n; p++) {
        const hit_t h = hits[p];
        const int64_t ca = h.a_begin >= 0 && h.a_end >= h.a_begin ? (int64_t)h.a_end - h.a_begin + 1 : 0;
        const int64_t cb = h.b_begin >= 0 && h.b_end >= h.b_begin ? (int64_t)h.b_end - h.b_begin + 1 : 0;
        const int64_t a0 = h.a_begin > 0 ? h.a_begin : 0, b0 = h.b_begin > 0 ? h.b_begin : 0;
        const int64_t c = diag ? diag[p] : 0, delta = a0 - b0;
        const int64_t r = one_cigar(m, bases + off[2 * p] + a0, ca, bases + off[2 * p + 1] + b0, cb, c - band - delta, c + band - delta, h.score,
                                    ops + slot[p]);
        if (r < 0) return (int)r;
        count[p] = (uint32_t)r;
    }
    return 0;
}
