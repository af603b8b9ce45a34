/*
 * Checker for CIGARs (tests/sw_cigar_ref.py compiles and loads this).  It applies the contract of include/agx.h ("Alignment
 * itself") BY DEFINITION and knows nothing of how the device gets there: score and span of every pair come from the existing
 * checkers (the caller passes their hits in); this file fills the three full matrices of the pinned Gotoh recurrence over
 * x = a[a_begin..a_end] (query, ca columns) and y = b[b_begin..b_end] (target, cb rows),
 *   H[0][0] = 0, H[0][j] = go + j ge, H[i][0] = go + i ge, E[0][j] = F[i][0] = -infinity
 *   E[i][j] = max(H[i-1][j] + go + ge, E[i-1][j] + ge)       D
 *   F[i][j] = max(H[i][j-1] + go + ge, F[i][j-1] + ge)       I
 *   H[i][j] = max(H[i-1][j-1] + w(i,j), E[i][j], F[i][j])
 * and walks back from (cb, ca) in state H exactly as the contract words it: diagonal first, then E, then F; a gap state stays
 * only on a strict "extending beats opening"; row 0 and column 0 end the walk with one run.  It fails (-2) when H[cb][ca] is
 * not the hit's score.  Operations are length << 4 | op (I 1, D 2, = 7, X 8), in forward order, runs merged.
 * score != NULL: w = score[code[x]][code[y]] and '=' means identical codes; else match / mismatch on the bytes.
 */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int32_t score, a_begin, a_end, b_begin, b_end;
} hit_t;

#define NEG (-(1 << 29))
enum { OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8 };

/* ops: room for ca + cb words; *n_ops receives the number of runs.  0, -1 out of memory, -2 the corner is not `want`. */
static int one_pair(const uint8_t *x, int ca, const uint8_t *y, int cb, int match, int mismatch, int go, int ge, const int8_t *score,
                    const uint8_t *code, int want, uint32_t *ops, uint32_t *n_ops)
{
    *n_ops = 0;
    if (ca == 0 && cb == 0) return want == 0 ? 0 : -2;
    if (ca == 0 || cb == 0) {
        const int l = ca ? ca : cb;
        if (go + l * ge != want) return -2;
        ops[0] = (uint32_t)l << 4 | (uint32_t)(ca ? OP_I : OP_D);
        *n_ops = 1;
        return 0;
    }
    const size_t W = (size_t)ca + 1, cells = W * ((size_t)cb + 1);
    int32_t *H = (int32_t *)malloc(sizeof(int32_t) * cells), *E = (int32_t *)malloc(sizeof(int32_t) * cells),
            *F = (int32_t *)malloc(sizeof(int32_t) * cells);
    uint8_t *rev = (uint8_t *)malloc((size_t)ca + cb);
    if (!H || !E || !F || !rev) {
        free(H);
        free(E);
        free(F);
        free(rev);
        return -1;
    }
    const int o = go + ge;
#define AT(M, i, j) M[(size_t)(i) * W + (size_t)(j)]
    AT(H, 0, 0) = 0;
    AT(E, 0, 0) = AT(F, 0, 0) = NEG;
    for (int j = 1; j <= ca; j++) {
        AT(H, 0, j) = go + j * ge;
        AT(E, 0, j) = AT(F, 0, j) = NEG;
    }
    for (int i = 1; i <= cb; i++) {
        AT(H, i, 0) = go + i * ge;
        AT(E, i, 0) = AT(F, i, 0) = NEG;
        for (int j = 1; j <= ca; j++) {
            const int e1 = AT(H, i - 1, j) + o, e2 = AT(E, i - 1, j) + ge;
            const int f1 = AT(H, i, j - 1) + o, f2 = AT(F, i, j - 1) + ge;
            const int e = e1 > e2 ? e1 : e2, f = f1 > f2 ? f1 : f2;
            const uint8_t xs = x[j - 1], ys = y[i - 1];
            const int w = score ? score[(size_t)code[xs] * 32 + code[ys]] : (xs == ys ? match : mismatch);
            int h = AT(H, i - 1, j - 1) + w;
            if (e > h) h = e;
            if (f > h) h = f;
            AT(E, i, j) = e;
            AT(F, i, j) = f;
            AT(H, i, j) = h;
        }
    }
    int rc = AT(H, cb, ca) == want ? 0 : -2;
    /* the walk: one op per emitted cell, backwards */
    size_t n = 0;
    int i = cb, j = ca, state = 0; /* 0 H, 1 E, 2 F */
    while (rc == 0) {
        if (state == 0) {
            if (i == 0) {
                for (; j > 0; j--) rev[n++] = OP_I;
                break;
            }
            if (j == 0) {
                for (; i > 0; i--) rev[n++] = OP_D;
                break;
            }
            const uint8_t xs = x[j - 1], ys = y[i - 1];
            const int w = score ? score[(size_t)code[xs] * 32 + code[ys]] : (xs == ys ? match : mismatch);
            const int same = score ? code[xs] == code[ys] : xs == ys;
            if (AT(H, i, j) == AT(H, i - 1, j - 1) + w) {
                rev[n++] = same ? OP_EQ : OP_X;
                i--;
                j--;
            } else if (AT(H, i, j) == AT(E, i, j))
                state = 1;
            else
                state = 2;
        } else if (state == 1) {
            rev[n++] = OP_D;
            state = AT(E, i - 1, j) + ge > AT(H, i - 1, j) + o ? 1 : 0;
            i--;
        } else {
            rev[n++] = OP_I;
            state = AT(F, i, j - 1) + ge > AT(H, i, j - 1) + o ? 2 : 0;
            j--;
        }
    }
    /* reversed, equal neighbours merged into maximal runs */
    uint32_t runs = 0;
    for (size_t k = n; k-- > 0;) {
        if (runs && (ops[runs - 1] & 15u) == rev[k]) ops[runs - 1] += 16u;
        else ops[runs++] = 1u << 4 | rev[k];
    }
    *n_ops = runs;
    free(H);
    free(E);
    free(F);
    free(rev);
    return rc;
}

/* slot[p]: where pair p's operations go in ops (room for ca + cb words each); count[p]: how many there are.
 * -1 out of memory; -2 the span's pinned score is not the hit's; -3 a span outside its sequences; -4 a byte outside the alphabet */
int sw_cigar_ref(const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, int match, int mismatch, int go, int ge,
                 const int8_t *score, const uint8_t *code, const hit_t *hits, const uint64_t *slot, uint32_t *ops, uint32_t *count)
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
        const int rc = one_pair(a, ca, b, cb, match, mismatch, go, ge, score, code, h.score, ops + slot[p], &count[p]);
        if (rc) return rc;
    }
    return 0;
}
