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
// STATS (agx_sw_loc_stats_kernel.hip, agx_sw_loc_mat_stats_kernel.hip; DESIGN.md 4.1e): every state is the tuple (score, L),
// L = matches << 12 | pairs of the best path into it, compared lexicographically and held as ONE int64, score << 32 | L.  L is
// non-negative and below 2^24 (pairs <= 2560), so the signed 64-bit order is the tuple order, the high word is the score word
// of the plain build -- rising offset, floor and all -- and a 64-bit add never carries from L into the score.  A diagonal move
// adds 0x1001 for identical symbols and 1 otherwise, but nothing in a row before or beyond b: the pre-rows of the skew must
// stay at the floor tuple (0, 0), which a mismatch of 0 or a padding entry of 0 would otherwise beat.  Capture is by the score
// word alone, exactly as above; L is read at the cell so chosen (the leftmost column of the row that holds the score, whatever
// L the columns further right hold) and leaves by a vector store to lstat[out].  This build runs the BEGIN pass of a stats
// batch: there every alignment of the reported score begins in the first cell (DESIGN.md 4.1b), so the tuple maximum at the
// end cell is over exactly the alignments of the reported span.
//
// (shared by agx_sw_loc_kernel.hip, agx_sw_loc_mat_kernel.hip and their _stats builds; opens an anonymous namespace that the
// including file closes after its launch helper)
#include "agx_sw.h"

#include <type_traits>

namespace {

constexpr uint32_t kLocRowPad = 0x100u; // never equals a byte

__device__ __forceinline__ int loc_shr1(int old, int v)
{
    // DPP wave_shr:1 -- lane i receives lane i-1's v (a group's first lane substitutes the boundary)
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ long long loc_shr1(long long old, long long v) // STATS: both words of the tuple
{
    const uint32_t lo = (uint32_t)loc_shr1((int)old, (int)v);
    const int hi = loc_shr1((int)(old >> 32), (int)(v >> 32));
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | lo);
}
// a score as a state: itself, or the tuple (score, 0)
template <typename S>
__device__ __forceinline__ S loc_lift(int v)
{
    if constexpr (sizeof(S) == 8) return (S)((unsigned long long)(long long)v << 32);
    else return v;
}
__device__ __forceinline__ int loc_score(int v) { return v; }
__device__ __forceinline__ int loc_score(long long v) { return (int)(v >> 32); }

template <int C, bool MAT, bool STATS = false>
__device__ __forceinline__ void loc_body(const SwParams &prm, const uint32_t *__restrict__ img, const SwGroup *__restrict__ groups,
                                         const SwWave w, int32_t *__restrict__ scores, uint32_t *__restrict__ ends, const int16_t *sub,
                                         uint32_t *__restrict__ lstat = nullptr)
{
    using S = typename std::conditional<STATS, long long, int>::type;
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
    S floor_t = loc_lift<S>(-age);
    S zb = loc_lift<S>(gf - age);
    S z[C], e[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        z[j] = loc_lift<S>(gf - age);
        e[j] = loc_lift<S>(-2 * age);
    }
    S z_last = loc_lift<S>(gf - age), f_last = loc_lift<S>(gf - age), diag_in = loc_lift<S>(gf - 2 * age);
    int best = gf - age;
    uint32_t best_l = 0; // STATS: L of the cell `best` was first reached in
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
        S zl = loc_shr1(zb, z_last);
        S fl = loc_shr1(zb, f_last);
        int yc = loc_shr1(fresh, yc_prev);
        if (start) {
            zl = zb;
            fl = zb;
            yc = fresh;
        }
        best += age;
        S zd = diag_in;
        diag_in = zl;
        S zleft = zl, f = fl;
        const int ycol = yc * 2; // MAT: byte offset inside a matrix row
        // STATS: a pair counts in the rows of b only; MAT: identical symbols = this column's row offset equals the step's
        const uint32_t row_inc = yc != kPadRow ? 1u : 0u;
        const int yrow = yc != kPadRow ? yc * (kSwMatDim * 2) : -1;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int xs = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            const S up = z[j];
            const S ev = max(max(up, e[j]), floor_t);
            f = max(zleft, f);
            if (j) f += loc_lift<S>(ge);
            const int lag = j ? 0 : age;
            S s;
            if constexpr (MAT && STATS)
                s = zd + (loc_lift<S>(lag + *reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(sub) + (xrow[j] + ycol))) +
                          (S)(xrow[j] == yrow ? 0x1001u : row_inc));
            else if constexpr (MAT)
                s = zd + lag + *reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(sub) + (xrow[j] + ycol));
            else if constexpr (STATS)
                s = zd + (loc_lift<S>(xs == yc ? s_match + lag : s_mis + lag) + (S)(xs == yc ? 0x1001u : row_inc));
            else
                s = zd + (xs == yc ? s_match + lag : s_mis + lag);
            const S v = max(max(ev, f), s);
            const S zn = v + loc_lift<S>(gf + age);
            e[j] = ev;
            z[j] = zn;
            zd = up;
            zleft = zn;
        }
        int m = loc_score(z[0]);
#pragma unroll
        for (int j = 1; j < C; j += 2) m = j + 1 < C ? max(max(m, loc_score(z[j])), loc_score(z[j + 1])) : max(m, loc_score(z[j]));
        if (m > best) { // a higher score than in any earlier row of this lane's columns
            int col = 0;
#pragma unroll
            for (int j = C - 1; j > 0; --j) col = loc_score(z[j]) == m ? j : col;
            col = loc_score(z[0]) == m ? 0 : col; // leftmost column of the row that holds it
            if constexpr (STATS) { // L of that very cell
#pragma unroll
                for (int j = C - 1; j >= 0; --j) best_l = loc_score(z[j]) == m ? (uint32_t)z[j] : best_l;
            }
            best = m;
            hit_t = t;
            hit_j = col;
        }
        z_last = zleft;
        f_last = f;
        yc_prev = yc;
        floor_t += loc_lift<S>(age);
        zb += loc_lift<S>(age);
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
        uint32_t ol = 0;
        if constexpr (STATS) ol = (uint32_t)__shfl_down((int)best_l, o);
        if (gl + o < G && (ob > best || (ob == best && ok < key))) {
            best = ob;
            key = ok;
            best_l = ol;
        }
    }
    if (feeder) {
        scores[g.out] = best;
        ends[g.out] = key;
        if constexpr (STATS) lstat[g.out] = best_l;
    }
}

