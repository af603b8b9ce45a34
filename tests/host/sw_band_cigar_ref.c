/*
 * Checker for the CIGARs of banded batches (tests/sw_band_cigar_ref.py compiles and loads this).  A banded Gotoh over the span
 * a hit reports, BY DEFINITION of include/agx.h ("CIGARs for banded batches"), written from the contract and not from the
 * kernel: row by row over the in-band cells only, every neighbour asked "are you in the matrix and in the band?" before it is
 * read, two rolling rows of H and E indexed by the column, and ONE BYTE per in-band cell of what the walk back will ask:
 *   bits 0-1  in state H at (i, j): 0 if H[i][j] == H[i-1][j-1] + w(i, j), else 1 if H[i][j] == E[i][j], else 2 (F)
 *   bit 2     in state E at (i, j): E[i-1][j] + e > H[i-1][j] + o, strictly (stay in E at (i-1, j))
 *   bit 3     in state F at (i, j): F[i][j-1] + e > H[i][j-1] + o, strictly
 * at dir[i * width + (j - i - dlo)].  The walk is the contract's, literally: from (cb, ca) in state H; state H with i == 0
 * emits j x I, with j == 0 i x D.  i = symbols of b consumed, j = symbols of a; a cell exists iff 0 <= i <= cb, 0 <= j <= ca,
 * dlo <= j - i <= dhi.  The band is the PAIR's, from the full lengths: GLOBAL (mode 1) dlo = min(0, la - lb) - w,
 * dhi = max(0, la - lb) + w; EXTEND (mode 3) dlo = -w, dhi = +w.  Arithmetic is 64-bit, so minus infinity never wraps.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (INT64_MIN / 4)
static int64_t max2(int64_t x, int64_t y) { return x > y ? x : y; }

/* ops: written forwards from ops[0]; returns their number, -1 out of memory, -2 the corner does not give `score`, -4 the walk
 * met a cell that does not exist */
static int64_t one(const uint8_t *x, int64_t ca, const uint8_t *y, int64_t cb, int64_t dlo, int64_t dhi, int match, int mismatch, int go, int ge,
                   int64_t score, uint32_t *ops)
{
    if (ca == 0 && cb == 0) return 0;
    if (ca == 0) {
        ops[0] = (uint32_t)cb << 4 | 2u;
        return 1;
    }
    if (cb == 0) {
        ops[0] = (uint32_t)ca << 4 | 1u;
        return 1;
    }
    const int64_t width = dhi - dlo + 1, o = (int64_t)go + ge, e = ge;
    uint8_t *dir = (uint8_t *)calloc((size_t)(cb + 1) * (size_t)width, 1);
    int64_t *H = (int64_t *)malloc(sizeof(int64_t) * 2 * ((size_t)ca + 1));
    int64_t *E = (int64_t *)malloc(sizeof(int64_t) * 2 * ((size_t)ca + 1));
    uint32_t *rev = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)ca + (size_t)cb + 1));
    int64_t n = -1;
    if (!dir || !H || !E || !rev) goto done;
    int64_t corner = NEG;
    for (int64_t i = 0; i <= cb; i++) {
        int64_t *row = H + (size_t)(i & 1) * ((size_t)ca + 1), *erow = E + (size_t)(i & 1) * ((size_t)ca + 1);
        const int64_t *up = H + (size_t)((i + 1) & 1) * ((size_t)ca + 1), *eup = E + (size_t)((i + 1) & 1) * ((size_t)ca + 1);
        const int64_t jlo = i + dlo > 0 ? i + dlo : 0, jhi = i + dhi < ca ? i + dhi : ca;
        int64_t F = NEG;
        for (int64_t j = jlo; j <= jhi; j++) {
            const int64_t d = j - i;
            const int has_up = i > 0 && d + 1 <= dhi, has_left = j > 0 && d - 1 >= dlo;
            int64_t v;
            uint8_t bits = 0;
            if (i == 0 && j == 0) {
                v = 0;
                erow[j] = NEG;
                F = NEG;
            } else if (i == 0) {
                v = go + j * e;
                erow[j] = NEG;
                F = NEG; /* F[0][j] is not asked: state H with i == 0 ends the walk */
            } else if (j == 0) {
                v = go + i * e;
                erow[j] = NEG;
                F = NEG;
            } else {
                int64_t ev = NEG, fv = NEG;
                if (has_up) {
                    const int64_t open = up[j] + o, ext = eup[j] > NEG ? eup[j] + e : NEG;
                    ev = max2(open, ext);
                    if (ext > open) bits |= 4;
                }
                if (has_left) {
                    const int64_t open = row[j - 1] + o, ext = F > NEG ? F + e : NEG;
                    fv = max2(open, ext);
                    if (ext > open) bits |= 8;
                }
                const int64_t s = up[j - 1] + (x[j - 1] == y[i - 1] ? match : mismatch); /* (i-1, j-1): same diagonal, exists */
                v = max2(s, max2(ev, fv));
                bits |= v == s ? 0 : v == ev ? 1 : 2;
                erow[j] = ev;
                F = fv;
            }
            row[j] = v;
            dir[(size_t)i * (size_t)width + (size_t)(d - dlo)] = bits;
            if (i == cb && j == ca) corner = v;
        }
    }
    if (corner != score) {
        n = -2;
        goto done;
    }
    {
        int64_t i = cb, j = ca, k = 0;
        int state = 0;
        n = -4;
        while (i || j) {
            if (j - i < dlo || j - i > dhi) goto done;
            if (i == 0) {
                for (int64_t t = 0; t < j; t++) rev[k++] = 1;
                break;
            }
            if (j == 0) {
                for (int64_t t = 0; t < i; t++) rev[k++] = 2;
                break;
            }
            const uint8_t bits = dir[(size_t)i * (size_t)width + (size_t)(j - i - dlo)];
            if (state == 0) {
                if ((bits & 3) == 0) {
                    rev[k++] = x[j - 1] == y[i - 1] ? 7 : 8;
                    i--;
                    j--;
                } else
                    state = bits & 3;
            } else if (state == 1) {
                rev[k++] = 2;
                state = bits & 4 ? 1 : 0;
                i--;
            } else {
                rev[k++] = 1;
                state = bits & 8 ? 2 : 0;
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
    free(dir);
    free(H);
    free(E);
    free(rev);
    return n;
}

/* hits: what the banded checker reports for (mode, band); slot[p]: where pair p's operations start in `wide` (room for ca + cb) */
int sw_band_cigar_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                      int mode, int band, const hit_t *hits, const uint64_t *slot, uint32_t *wide, uint32_t *count)
{
    if ((mode != 1 && mode != 3) || band < 0) return -3;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t la = len[2 * p], lb = len[2 * p + 1], diff = mode == 1 ? la - lb : 0;
        const int64_t dlo = (diff < 0 ? diff : 0) - band, dhi = (diff > 0 ? diff : 0) + band;
        const hit_t *h = &hits[p];
        const int64_t ca = h->a_begin >= 0 && h->a_end >= h->a_begin ? (int64_t)h->a_end - h->a_begin + 1 : 0;
        const int64_t cb = h->b_begin >= 0 && h->b_end >= h->b_begin ? (int64_t)h->b_end - h->b_begin + 1 : 0;
        if ((ca && h->a_begin != 0) || (cb && h->b_begin != 0)) return -5; /* begins are 0 */
        const int64_t n = one(bases + off[2 * p], ca, bases + off[2 * p + 1], cb, dlo, dhi, match, mismatch, go, ge, h->score, wide + slot[p]);
        if (n < 0) return (int)n;
        count[p] = (uint32_t)n;
    }
    return 0;
}
