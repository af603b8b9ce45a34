// Smith-Waterman ANCHORED fill for gfx950: the locating fill's int32 cell (agx_sw_loc_kernel.inc: a across the lanes, b
// streams, DPP hand-over, rising offsets) WITHOUT the zero floor and with gap-initialised boundaries.  Behind the modes
// GLOBAL, FIT, EXTEND and EXTEND_QUERY of agx_sw_batch_create_align_mode (agx_sw_anch_kernel.hip, match/mismatch) and of
// agx_sw_batch_create_align_matrix (agx_sw_anch_mat_kernel.hip, MAT); include/agx.h, "Alignment modes"; DESIGN.md 4.1c, 4.1d.
//
// Matrix.  Row r = -1 .. lb-1 (r symbols of b consumed: r + 1), column c = -1 .. la-1.  H[-1][-1] = 0, H[-1][c] = gf + c ge,
// H[r][-1] = gf + r ge (start pinned) or 0 (FIT: free target start), E = -infinity on row -1, F = -infinity in column -1.
//
// Boundaries under the skew.
//   left:  a group's first lane substitutes zb = Z[r][-1] for the left and diagonal inputs, as the locating fill does.  In
//          the rising representation (stored = true + t |ge|) the pinned column gf + r ge is the CONSTANT 2 gf - |ge|; the
//          free one rises by |ge| per step.  One runtime increment (0 or |ge|) serves both.
//   top:   lane gl meets row 0 at step gl.  At that step -- one compare per step, the body taken once per lane -- it loads
//          row -1 of its own columns into z[], minus infinity into e[], H[-1][gl C - 1] into its diagonal input, and resets
//          what it has captured.  Whatever the steps before (its "pre-rows") computed is gone with that: pre-row values reach
//          pre-row cells of the next lane only (lane gl + 1 reads lane gl's step t - 1, a pre-row of both or row 0 of lane gl).
//   minus infinity is kNegInf = -2^30, stored, and nothing is ever added to e[]: e = max(z_up, e).  True values lie within
//          +-(la + lb + 2) * 1000 + 65 599 * 1000 of zero in the rising representation (< 1.4e8): no wrap either way.
//
// Capture.
//   ANY (EXTEND):  the locating fill's rule -- strict improvement of the lane's row maximum over its running maximum, which
//          starts at H[-1][-1] = 0.  Padding (a column beyond a, a row beyond b) never matches, and mismatch, gf, ge <= 0: a
//          padding cell holds at most what its upper, left or upper-left neighbour holds, a cell that precedes it in (row,
//          column) order, so the first cell in that order that holds the maximum is a real one.  Boundary cells are <= 0.
//   COL (FIT, EXTEND_QUERY, GLOBAL):  the query's last column, lane (la-1)/C, column k = (la-1)%C, rows -1 .. lb-1 ONLY (a
//          row beyond b may hold more than the column's maximum: it inherits from columns further left).  k is per group:
//          a tree over the bits of k (C - 1 mask muxes, six loop-invariant masks) extracts z[k]; the running maximum
//          starts at H[-1][la-1] with row -1.  GLOBAL takes the value the same select left at row lb-1.
// ends[] word: (row + 1) << 12 | (column + 1), so row -1 / column -1 ("nothing consumed") are 0.
//
// MAT: the diagonal move adds a substitution-matrix entry as in agx_sw_kernel.inc -- symbol numbers 1..32 in the image,
// padding is symbol 0 in columns and rows alike, `sub` the workgroup's LDS copy of the int16 table of score - gf, one read
// at (the column's hoisted row offset + the step's symbol) in place of compare + select.  Entries that involve symbol 0 are
// <= 0, which is all ANY's argument asks of "never matches"; COL reads real rows of the query's last real column, and no
// real cell has a padding cell above, left or upper-left of it (pre-rows are wiped by the top reset), so it does not
// depend on what padding scores at all.  The diagonal adds at most 128 * 2560 to the range either way: within 1.35e8.
//
// (shared by agx_sw_anch_kernel.hip and agx_sw_anch_mat_kernel.hip; opens an anonymous namespace that the including file
// closes after its launch helper)
#include "agx_sw.h"

namespace {

constexpr uint32_t kAnchRowPad = 0x100u; // never equals a byte
constexpr int kNegInf = -(1 << 30);

__device__ __forceinline__ int anch_shr1(int old, int v)
{
    // DPP wave_shr:1 -- lane i receives lane i-1's v (a group's first lane substitutes the boundary)
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}

template <int C, bool COL, bool MAT>
__device__ __forceinline__ void anch_body(const SwParams &prm, const int flags, const uint32_t *__restrict__ img,
                                          const SwGroup *__restrict__ groups, const SwWave w, int32_t *__restrict__ scores,
                                          uint32_t *__restrict__ ends, const int16_t *sub)
{
    constexpr int XW = (C + 3) / 4; // dwords holding this lane's C symbols
    const int ge = prm.ge, gf = prm.gf, s_match = prm.hd, s_mis = prm.hd - prm.delta;
    const int lane = threadIdx.x & 63;
    const int G = w.G;
    const int grp = lane / G;
    const int gl = lane - grp * G;
    const bool active = grp < (int)w.n_groups;
    const bool start = gl == 0;
    const bool feeder = active && start;

    SwGroup g;
    g.x_dw = g.y_dw = g.lx_ly = g.out = 0;
    if (active) g = groups[w.first_group + grp];
    const int ly = (int)(g.lx_ly >> 16);
    const int la = (int)(g.lx_ly & 0x7fffu);
    const int nyq = (ly + 3) >> 2;

    uint32_t xw[XW];
    {
        const uint32_t o = (uint32_t)gl * C, d0 = o >> 2, sh = o & 3u;
        uint32_t raw[XW + 1];
#pragma unroll
        for (int k = 0; k <= XW; ++k) raw[k] = active ? img[g.x_dw + d0 + k] : 0u;
#pragma unroll
        for (int k = 0; k < XW; ++k) xw[k] = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], sh);
    }

    const uint32_t *yp = img + g.y_dw;
    auto row_quad = [&](int q) -> uint32_t { return (feeder && q < nyq) ? yp[q] : 0u; };

    // state as in the locating fill: z = H + gf at offset r(t) = t |ge|, e = E at offset r(t - 1); no floor
    const int age = -ge;
    const bool free_start = (flags & 1) != 0;
    int zb = free_start ? gf - age : 2 * gf - age; // Z[r][-1] at r(t - 1)
    const int zb_inc = free_start ? age : 0;
    const int ztop = 2 * gf - gl * C * age + (gl - 1) * age; // Z[-1][gl C] at r(gl - 1)
    const int last_lane = la > 0 ? (la - 1) / C : 0;
    const int kcol = (active && gl == last_lane && la > 0) ? la - 1 - last_lane * C : 0;
    const int t_last = ly - 1 + gl; // the step of row lb - 1
    // the bits of kcol as all-ones / all-zeros masks, one register each: the tree below then is a v_and + v_bitop3 pair per node.
    // (Written with selects, the classes 8..30 came out as C - 1 variable-index extractions of C - 1 compares each.)
    uint32_t kmask[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        kmask[n] = (kcol >> n) & 1 ? 0xffffffffu : 0u;
        asm volatile("" : "+v"(kmask[n]));
    }
    int z[C], e[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        z[j] = 0;
        e[j] = kNegInf;
    }
    int z_last = 0, f_last = 0, diag_in = 0, best = 0, zcorner = 0;
    constexpr int kPadRow = MAT ? 0 : (int)kAnchRowPad;
    int yc_prev = kPadRow;
    int hit_t = -1, hit_j = 0;
    // MAT: byte offset of every owned column's matrix row
    int xrow[MAT ? C : 1];
    if constexpr (MAT) {
#pragma unroll
        for (int j = 0; j < C; ++j) xrow[j] = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu) * (kSwMatDim * 2);
    }

    uint32_t q0 = row_quad(0), q1 = row_quad(1), q2 = row_quad(2);
    const int steps = (int)w.steps;
    uint32_t rows = 0;
    int t = 0;

    auto step = [&]() __attribute__((always_inline)) {
        const int fresh = (t < ly) ? (int)(rows & 0xffu) : kPadRow;
        rows >>= 8;
        int zl = anch_shr1(zb, z_last);
        int fl = anch_shr1(zb, f_last);
        int yc = anch_shr1(fresh, yc_prev);
        if (start) {
            zl = zb;
            fl = zb;
            yc = fresh;
        }
        if (t == gl) { // row 0 of this lane: row -1 above it, nothing captured yet
            int v = ztop;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                z[j] = v;
                e[j] = kNegInf;
                v += ge;
            }
            diag_in = start ? gf - 2 * age : ztop;
            if (COL) {
                best = ztop + kcol * ge; // H[-1][la-1], found in row -1
                hit_t = gl - 1;
            } else {
                best = gf + (gl - 1) * age; // H[-1][-1] = 0
                hit_t = -1;
            }
        }
        best += age;
        int zd = diag_in;
        diag_in = zl;
        int zleft = zl, f = fl;
        const int ycol = yc * 2; // MAT: byte offset inside a matrix row
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int xs = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            const int up = z[j];
            const int ev = max(up, e[j]);
            f = max(zleft, f);
            if (j) f += ge;
            const int lag = j ? 0 : age;
            int s;
            if constexpr (MAT)
                s = zd + lag + *reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(sub) + (xrow[j] + ycol));
            else
                s = zd + (xs == yc ? s_match + lag : s_mis + lag);
            const int v = max(max(ev, f), s);
            const int zn = v + (gf + age);
            e[j] = ev;
            z[j] = zn;
            zd = up;
            zleft = zn;
        }
        if (COL) {
            uint32_t sel[C];
#pragma unroll
            for (int j = 0; j < C; ++j) sel[j] = (uint32_t)z[j];
#pragma unroll
            for (int bit = 1, n = 0; bit < C; bit <<= 1, ++n) {
                const uint32_t on = kmask[n];
#pragma unroll
                for (int j = 0; j + bit < C; j += 2 * bit) sel[j] = (on & sel[j + bit]) | (~on & sel[j]);
            }
            const int zk = (int)sel[0];
            const bool in_b = t <= t_last; // rows beyond b do not count
            const bool better = in_b && zk > best;
            best = better ? zk : best;
            hit_t = better ? t : hit_t;
            zcorner = in_b ? zk : zcorner;
        } else {
            int m = z[0];
#pragma unroll
            for (int j = 1; j < C; j += 2) m = j + 1 < C ? max(max(m, z[j]), z[j + 1]) : max(m, z[j]);
            if (m > best) { // a higher score than in any earlier row of this lane's columns
                int col = 0;
#pragma unroll
                for (int j = C - 1; j > 0; --j) col = z[j] == m ? j : col;
                col = z[0] == m ? 0 : col; // leftmost column of the row that holds it
                best = m;
                hit_t = t;
                hit_j = col;
            }
        }
        z_last = zleft;
        f_last = f;
        yc_prev = yc;
        zb += zb_inc;
        ++t;
    };

    const int quads = steps >> 2;
    for (int q = 0; q < quads; ++q) {
        rows = q0;
        q0 = q1;
        q1 = q2;
        q2 = row_quad(q + 3);
#pragma unroll
        for (int b = 0; b < 4; ++b) step();
    }
    rows = q0;
#pragma unroll 1
    while (t < steps) step();

    best -= gf + (steps - 1) * age; // z of the last step stands r(steps - 1) above H + gf
    uint32_t key;
    if (COL) {
        if (flags & 2) { // GLOBAL: the corner, whatever the column's maximum
            best = zcorner - gf - t_last * age;
            hit_t = t_last;
        }
        key = ((uint32_t)(hit_t - gl + 1) << kSwLocColBits) | (uint32_t)la;
        const int src = grp * G + last_lane; // the lane that owns the query's last column
        best = __shfl(best, src);
        key = (uint32_t)__shfl((int)key, src);
    } else {
        key = hit_t < 0 ? 0u : ((uint32_t)(hit_t - gl + 1) << kSwLocColBits) | (uint32_t)(gl * C + hit_j + 1);
        // over the group's lanes by the rule: score, then row, then column (G need not be a power of two)
        for (int o = 1; o < G; o <<= 1) {
            const int ob = __shfl_down(best, o);
            const uint32_t ok = (uint32_t)__shfl_down((int)key, o);
            if (gl + o < G && (ob > best || (ob == best && ok < key))) {
                best = ob;
                key = ok;
            }
        }
    }
    if (feeder) {
        scores[g.out] = best;
        ends[g.out] = key;
    }
}

