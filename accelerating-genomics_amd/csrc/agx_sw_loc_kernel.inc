// Smith-Waterman LOCATING fill for gfx950: the int32 fill of agx_sw_kernel.inc (lanes own columns, rows stream, DPP
// hand-over, rising offsets) that also carries WHERE the running maximum was first reached.  Behind agx_sw_batch_create_align
// (agx_sw_loc_kernel.hip, match/mismatch) and agx_sw_batch_create_align_matrix (agx_sw_loc_mat_kernel.hip, MAT).
//
// Orientation.  An align batch always lays the pair's FIRST sequence a (the query) across the lanes and streams the second,
// b (the target), whichever is shorter: a lane's columns are positions of a, a step's row is a position of b.  The contract
// (include/agx.h) asks for the cell with the smallest b among the maxima, then the smallest a -- in this orientation that is
// "first row, then first column", the order in which a lane meets its cells.
//
// Per step a lane takes the maximum m of this row's C new z values (the score-only fill's v_max3 chain, into a register of
// its own) and compares it with its running maximum, which was bumped by |ge| first and so stands at this step's offset:
// m > best, strictly, means "higher than in any earlier row of my columns".  Only then -- a branch a few steps of a fill
// take -- the lane looks for the first column that holds m (compare + select per column) and notes step and column.  An
// equal value in a later row never replaces the cell, an equal value further right in the same row loses to the scan order.
// Over the lanes of a group the winner is picked by the rule, not by lane order: higher score, then smaller row, then
// smaller column, on the key (row << 12 | column).
//
// Padding cannot win: a padding cell (column beyond a: symbol 0x00; row before or beyond b: 0x100) never matches, so its
// value comes from its upper, left or upper-left neighbour without a gain -- a cell that precedes it in (row, column)
// order and holds at least as much.  By induction the first cell in that order that holds the maximum is a real one, its
// lane finds it, and the key prefers it.  Cells of value 0 are never noted (z of H = 0 equals the bumped start value):
// score 0 leaves the key at -1.
//
// MAT: the diagonal move adds a substitution-matrix entry, exactly as in agx_sw_kernel.inc -- the image holds symbol numbers
// 1..32, padding is symbol 0 in columns and rows alike, `sub` is the workgroup's LDS copy of the kSwMatDim x kSwMatDim int16
// table of score - gf, and a cell reads one entry at (its column's hoisted row offset + the step's symbol) in place of
// compare + select.  Every entry of row 0 and column 0 is <= 0 (the create path fills them with min(0, lowest entry)), so
// the diagonal move into a padding cell is still "without a gain" and the argument above stands word for word.
//
// (shared by agx_sw_loc_kernel.hip and agx_sw_loc_mat_kernel.hip; opens an anonymous namespace that the including file
// closes after its launch helper)
#include "agx_sw.h"

namespace {

constexpr uint32_t kLocRowPad = 0x100u; // never equals a byte

__device__ __forceinline__ int loc_shr1(int old, int v)
{
    // DPP wave_shr:1 -- lane i receives lane i-1's v (a group's first lane substitutes the boundary)
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}

template <int C, bool MAT>
__device__ __forceinline__ void loc_body(const SwParams &prm, const uint32_t *__restrict__ img, const SwGroup *__restrict__ groups,
                                         const SwWave w, int32_t *__restrict__ scores, uint32_t *__restrict__ ends, const int16_t *sub)
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

    // state as in agx_sw_kernel.inc: z = H + gf and e = max(P, 0), both with the rising offset r(t) = t |ge|
    const int age = -ge;
    int floor_t = -age;
    int zb = gf - age;
    int z[C], e[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        z[j] = gf - age;
        e[j] = -2 * age;
    }
    int z_last = gf - age, f_last = gf - age, diag_in = gf - 2 * age, best = gf - age;
    constexpr int kPadRow = MAT ? 0 : (int)kLocRowPad;
    int yc_prev = kPadRow;
    int hit_t = -1, hit_j = 0; // step and own column at which `best` was first reached
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
        int zl = loc_shr1(zb, z_last);
        int fl = loc_shr1(zb, f_last);
        int yc = loc_shr1(fresh, yc_prev);
        if (start) {
            zl = zb;
            fl = zb;
            yc = fresh;
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
            const int ev = max(max(up, e[j]), floor_t);
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
        z_last = zleft;
        f_last = f;
        yc_prev = yc;
        floor_t += age;
        zb += age;
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

    // row of b << 12 | column of a (columns < 4096, rows < 65536); 0xffffffff = nothing above zero was seen
    uint32_t key = hit_t < 0 ? 0xffffffffu : ((uint32_t)(hit_t - gl) << 12) | (uint32_t)(gl * C + hit_j);

    // over the group's lanes by the rule: score, then row, then column (G need not be a power of two)
    for (int o = 1; o < G; o <<= 1) {
        const int ob = __shfl_down(best, o);
        const uint32_t ok = (uint32_t)__shfl_down((int)key, o);
        if (gl + o < G && (ob > best || (ob == best && ok < key))) {
            best = ob;
            key = ok;
        }
    }
    if (feeder) {
        scores[g.out] = best;
        ends[g.out] = key;
    }
}

