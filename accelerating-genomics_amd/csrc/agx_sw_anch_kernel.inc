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
// STATS (agx_sw_anch_stats_kernel.hip, agx_sw_anch_mat_stats_kernel.hip; DESIGN.md 4.1e): as in agx_sw_loc_kernel.inc every
// state is the tuple (score, L), L = matches << 12 | pairs, one int64 = score << 32 | L; the top reset and both kinds of left
// boundary load L = 0, minus infinity is the tuple (-2^30, 0) and never wins whatever it meets.  The start is pinned in the
// modes that run this build (GLOBAL, EXTEND, EXTEND_QUERY, and EXTEND_QUERY as FIT's begin pass), so every path into the
// captured cell starts at the origin and the tuple maximum there is over exactly the alignments of the reported span.
// Capture reads the score word only: ANY as the locating fill does, COL by strict improvement of the selected column's
// score; L is what the chosen cell holds.
//
// TRACE (agx_sw_trace_kernel.hip, agx_sw_trace_mat_kernel.hip; DESIGN.md 4.1f; COL capture with the GLOBAL flag only): every cell
// also leaves four bits, all from values it computes anyway.  Bits 0..1: where H came from -- 0 the diagonal (v == s), else 1 E
// (v == ev), else 2 F: the order is the tie rule "diagonal, then D, then I".  Bit 2: E extended, e[j] > up before their
// maximum; bit 3: F extended, f > zleft before theirs -- strict, so a tie opens.  up stands for H[r-1] + open + extend and
// e[j] for E[r-1] + extend at one offset (the stored values rise by |ge| per step, which is what adding ge to e would undo),
// zleft and f likewise for column c - 1: a cell's inputs share one offset, so the comparisons are the true ones.  Boundaries
// need nothing of their own: a group's first lane has fl == zl == zb, not greater, so column 0 opens its F from the boundary
// column, and the top reset leaves e = minus infinity, so row 0 opens its E from row -1 -- what "open on ties" and E = F =
// minus infinity on the boundaries ask for.  The nibbles of a lane's C cells of one step fill W = ceil(C / 8) dwords, stored
// at trace + goff[group] + (t G + gl) W dwords: the lanes of a group write consecutive pieces of one step.  Only rows 0 ..
// ly - 1 of a lane are stored (steps gl .. ly - 1 + gl), so (t G + gl) W < (ly + G - 1) G W, the extent the host reserves.
//
// (shared by agx_sw_anch_kernel.hip, agx_sw_anch_mat_kernel.hip, their _stats builds and the two traced builds; opens an
// anonymous namespace that the including file closes after its launch helper)
#include "agx_sw.h"

#include <type_traits>

namespace {

constexpr uint32_t kAnchRowPad = 0x100u; // never equals a byte
constexpr int kNegInf = -(1 << 30);

__device__ __forceinline__ int anch_shr1(int old, int v)
{
    // DPP wave_shr:1 -- lane i receives lane i-1's v (a group's first lane substitutes the boundary)
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ long long anch_shr1(long long old, long long v) // STATS: both words of the tuple
{
    const uint32_t lo = (uint32_t)anch_shr1((int)old, (int)v);
    const int hi = anch_shr1((int)(old >> 32), (int)(v >> 32));
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | lo);
}
// a score as a state: itself, or the tuple (score, 0)
template <typename S>
__device__ __forceinline__ S anch_lift(int v)
{
    if constexpr (sizeof(S) == 8) return (S)((unsigned long long)(long long)v << 32);
    else return v;
}
__device__ __forceinline__ int anch_score(int v) { return v; }
__device__ __forceinline__ int anch_score(long long v) { return (int)(v >> 32); }

// TRACE: W dwords to p (4-byte aligned) as one store where the widths allow, W = 5 as four and one
typedef uint32_t anch_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t anch_u3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t anch_u4 __attribute__((ext_vector_type(4), aligned(4)));
template <int W>
__device__ __forceinline__ void anch_store_words(uint32_t *p, const uint32_t *w)
{
    static_assert(W >= 1 && W <= 5, "classes up to 40 columns");
    if constexpr (W == 1) p[0] = w[0];
    else if constexpr (W == 2) *reinterpret_cast<anch_u2 *>(p) = anch_u2{w[0], w[1]};
    else if constexpr (W == 3) *reinterpret_cast<anch_u3 *>(p) = anch_u3{w[0], w[1], w[2]};
    else {
        *reinterpret_cast<anch_u4 *>(p) = anch_u4{w[0], w[1], w[2], w[3]};
        if constexpr (W == 5) p[4] = w[4];
    }
}

template <int C, bool COL, bool MAT, bool STATS = false, bool TRACE = false>
__device__ __forceinline__ void anch_body(const SwParams &prm, const int flags, const uint32_t *__restrict__ img,
                                          const SwGroup *__restrict__ groups, const SwWave w, int32_t *__restrict__ scores,
                                          uint32_t *__restrict__ ends, const int16_t *sub, uint32_t *__restrict__ lstat = nullptr,
                                          uint32_t *__restrict__ trace = nullptr, const uint64_t *__restrict__ goff = nullptr)
{
    static_assert(!TRACE || (COL && !STATS), "the traced build is the GLOBAL fill of scores");
    using S = typename std::conditional<STATS, long long, int>::type;
    using U = typename std::conditional<STATS, unsigned long long, uint32_t>::type;
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
    S zb = anch_lift<S>(free_start ? gf - age : 2 * gf - age); // Z[r][-1] at r(t - 1)
    const S zb_inc = anch_lift<S>(free_start ? age : 0);
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
    S z[C], e[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        z[j] = 0;
        e[j] = anch_lift<S>(kNegInf);
    }
    S z_last = 0, f_last = 0, diag_in = 0, zcorner = 0;
    int best = 0;
    uint32_t best_l = 0; // STATS: L of the cell `best` was first reached in
    constexpr int kPadRow = MAT ? 0 : (int)kAnchRowPad;
    int yc_prev = kPadRow;
    int hit_t = -1, hit_j = 0;
    // MAT: byte offset of every owned column's matrix row
    int xrow[MAT ? C : 1];
    if constexpr (MAT) {
#pragma unroll
        for (int j = 0; j < C; ++j) xrow[j] = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu) * (kSwMatDim * 2);
    }

    // TRACE: where this lane's dwords of step t go (advanced by one step's G W dwords as t is)
    constexpr int TW = (C + 7) / 8;
    [[maybe_unused]] uint32_t *tp = nullptr;
    if constexpr (TRACE) {
        if (active) tp = trace + goff[w.first_group + grp] + (size_t)gl * TW;
    }

    uint32_t q0 = row_quad(0), q1 = row_quad(1), q2 = row_quad(2);
    const int steps = (int)w.steps;
    uint32_t rows = 0;
    int t = 0;

    auto step = [&]() __attribute__((always_inline)) {
        const int fresh = (t < ly) ? (int)(rows & 0xffu) : kPadRow;
        rows >>= 8;
        S zl = anch_shr1(zb, z_last);
        S fl = anch_shr1(zb, f_last);
        int yc = anch_shr1(fresh, yc_prev);
        if (start) {
            zl = zb;
            fl = zb;
            yc = fresh;
        }
        if (t == gl) { // row 0 of this lane: row -1 above it, nothing captured yet
            S v = anch_lift<S>(ztop);
#pragma unroll
            for (int j = 0; j < C; ++j) {
                z[j] = v;
                e[j] = anch_lift<S>(kNegInf);
                v += anch_lift<S>(ge);
            }
            diag_in = anch_lift<S>(start ? gf - 2 * age : ztop);
            if (COL) {
                best = ztop + kcol * ge; // H[-1][la-1], found in row -1
                hit_t = gl - 1;
            } else {
                best = gf + (gl - 1) * age; // H[-1][-1] = 0
                hit_t = -1;
            }
            best_l = 0;
        }
        best += age;
        S zd = diag_in;
        diag_in = zl;
        S zleft = zl, f = fl;
        const int ycol = yc * 2; // MAT: byte offset inside a matrix row
        // STATS: a pair counts in the rows of b only; MAT: identical symbols = this column's row offset equals the step's
        const uint32_t row_inc = yc != kPadRow ? 1u : 0u;
        const int yrow = yc != kPadRow ? yc * (kSwMatDim * 2) : -1;
        [[maybe_unused]] uint32_t tw[TW];
        if constexpr (TRACE) {
#pragma unroll
            for (int k = 0; k < TW; ++k) tw[k] = 0;
        }
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int xs = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            const S up = z[j];
            [[maybe_unused]] uint32_t nib = 0;
            if constexpr (TRACE) nib = ((uint32_t)(up - e[j]) >> 31) << 2 | ((uint32_t)(zleft - f) >> 31) << 3; // sign bits: no difference wraps
            const S ev = max(up, e[j]);
            f = max(zleft, f);
            if (j) f += anch_lift<S>(ge);
            const int lag = j ? 0 : age;
            S s;
            if constexpr (MAT && STATS)
                s = zd + (anch_lift<S>(lag + *reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(sub) + (xrow[j] + ycol))) +
                          (S)(xrow[j] == yrow ? 0x1001u : row_inc));
            else if constexpr (MAT)
                s = zd + lag + *reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(sub) + (xrow[j] + ycol));
            else if constexpr (STATS)
                s = zd + (anch_lift<S>(xs == yc ? s_match + lag : s_mis + lag) + (S)(xs == yc ? 0x1001u : row_inc));
            else
                s = zd + (xs == yc ? s_match + lag : s_mis + lag);
            const S v = max(max(ev, f), s);
            if constexpr (TRACE) {
                const uint32_t not_s = (uint32_t)(s - v) >> 31, not_e = (uint32_t)(ev - v) >> 31; // v is their maximum
                nib |= not_s + (not_s & not_e);
                tw[j >> 3] |= nib << (4 * (j & 7));
            }
            S zn = v + anch_lift<S>(gf + age);
            // (the bits are off the cell's chain: left to itself the scheduler defers them and keeps seven values per column
            // alive for it -- 229 registers at 16 columns.  Tying them to the value the next column waits for keeps them here.)
            if constexpr (TRACE) {
                if (j + 1 < C) asm volatile("" : "+v"(tw[j >> 3]), "+v"(zn), "+v"(z[j + 1]));
                else asm volatile("" : "+v"(tw[j >> 3]), "+v"(zn));
            }
            e[j] = ev;
            z[j] = zn;
            zd = up;
            zleft = zn;
        }
        if (COL) {
            U sel[C];
#pragma unroll
            for (int j = 0; j < C; ++j) sel[j] = (U)z[j];
#pragma unroll
            for (int bit = 1, n = 0; bit < C; bit <<= 1, ++n) {
                const U on = (U)(S)(int)kmask[n]; // (STATS: the mask over both words)
#pragma unroll
                for (int j = 0; j + bit < C; j += 2 * bit) sel[j] = (on & sel[j + bit]) | (~on & sel[j]);
            }
            const S zk = (S)sel[0];
            const bool in_b = t <= t_last; // rows beyond b do not count
            const bool better = in_b && anch_score(zk) > best;
            best = better ? anch_score(zk) : best;
            if constexpr (STATS) best_l = better ? (uint32_t)zk : best_l;
            hit_t = better ? t : hit_t;
            zcorner = in_b ? zk : zcorner;
        } else {
            int m = anch_score(z[0]);
#pragma unroll
            for (int j = 1; j < C; j += 2) m = j + 1 < C ? max(max(m, anch_score(z[j])), anch_score(z[j + 1])) : max(m, anch_score(z[j]));
            if (m > best) { // a higher score than in any earlier row of this lane's columns
                int col = 0;
#pragma unroll
                for (int j = C - 1; j > 0; --j) col = anch_score(z[j]) == m ? j : col;
                col = anch_score(z[0]) == m ? 0 : col; // leftmost column of the row that holds it
                if constexpr (STATS) { // L of that very cell
#pragma unroll
                    for (int j = C - 1; j >= 0; --j) best_l = anch_score(z[j]) == m ? (uint32_t)z[j] : best_l;
                }
                best = m;
                hit_t = t;
                hit_j = col;
            }
        }
        if constexpr (TRACE) {
            if (active && t >= gl && t <= t_last) anch_store_words<TW>(tp, tw); // rows 0 .. ly - 1 of this lane
            tp += (size_t)G * TW;
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
            best = anch_score(zcorner) - gf - t_last * age;
            if constexpr (STATS) best_l = (uint32_t)zcorner;
            hit_t = t_last;
        }
        key = ((uint32_t)(hit_t - gl + 1) << kSwLocColBits) | (uint32_t)la;
        const int src = grp * G + last_lane; // the lane that owns the query's last column
        best = __shfl(best, src);
        key = (uint32_t)__shfl((int)key, src);
        if constexpr (STATS) best_l = (uint32_t)__shfl((int)best_l, src);
    } else {
        key = hit_t < 0 ? 0u : ((uint32_t)(hit_t - gl + 1) << kSwLocColBits) | (uint32_t)(gl * C + hit_j + 1);
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
    }
    if (feeder) {
        scores[g.out] = best;
        ends[g.out] = key;
        if constexpr (STATS) lstat[g.out] = best_l;
    }
}

