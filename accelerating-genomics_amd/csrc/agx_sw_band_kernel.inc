// Smith-Waterman BANDED fill for gfx950: pinned-start Gotoh (no zero floor, gap-initialised boundaries) over the cells within a
// fixed distance of the main diagonal.  Behind agx_sw_batch_create_align_band, modes GLOBAL and EXTEND (include/agx.h, "Banded
// alignment"; DESIGN.md 4.1g).  The anchored fill (agx_sw_anch_kernel.inc) lays the query's COLUMNS across the lanes; here the
// lanes own DIAGONALS, so neither side has a column limit and the cost is length x band.
//
// Matrix.  Cell (i, j): i symbols of b (target) and j of a (query) consumed, 0 <= i <= lb, 0 <= j <= la, diagonal d = j - i,
// inside the band iff dlo <= d <= dhi.  A group of G lanes owns one pair; lane gl owns the K diagonals d0 + k, d0 = dlo + gl K,
// k = 0 .. K - 1 (G K >= dhi - dlo + 1; the slots beyond dhi are masked).  State per diagonal, in registers: z = H + gf
// (gf = gap_open + gap_extend, what both gap recurrences read) and e = E, int32, TRUE values -- no rising offset.
//
// Step t: lane gl fills row i = t - gl of its diagonals, left to right (k = 0 .. K - 1 is j = i + d0 + k).  A cell reads
//   left  (i, j - 1)      diagonal d - 1: the cell before it in this step; for k = 0 lane gl - 1's last cell of step t - 1
//                         (DPP wave_shr:1 of z and f), a group's first lane substitutes minus infinity
//   diag  (i - 1, j - 1)  diagonal d:     its own z[k] of the step before
//   up    (i - 1, j)      diagonal d + 1: its own z[k + 1], e[k + 1] of the step before (read before cell k + 1 overwrites them);
//                         for k = K - 1 the FIRST cell lane gl + 1 computes in this very step (it is one row behind).
// Hence two phases: every lane computes cell 0, hands its z and e to the left (DPP wave_shl:1; a group's last lane substitutes
// minus infinity), then computes cells 1 .. K - 1.
//
// Symbols.  b[i - 1] of a lane's row enters at the group's first lane and moves one lane per step (wave_shr:1), as in the
// anchored fill; a row outside 1 .. lb carries kBandRowPad, which equals no byte.  The query runs the other way: lane gl holds the
// K bytes a[j0 - 1 .. j0 + K - 2], j0 = i + d0, in K / 4 dwords and shifts them by one byte per step (v_alignbyte); the byte that
// enters on top is byte 1 of lane gl + 1's window of the same step (wave_shl:1), and the group's last lane takes it from the
// image: a[q0 + t], q0 = dlo + G K - G.  The host stores a behind (-q0 mod 4) zero bytes, so that byte sits at a dword boundary
// when t is a multiple of four in every group of the wave, and b behind one byte for the same reason: both loaders read one
// dword per four steps, three quads ahead.  Positions outside a read as 0, the padding symbol (byte 0x00 is refused on input).
//
// Boundaries and masking.  Only H is masked: after a cell is computed its z is replaced by minus infinity unless
// 0 <= i <= lb, 0 <= j <= la and d <= dhi -- one bit per cell of a mask made once per step.  E and F of masked cells stay as
// computed; they are read only by other masked cells or come out as minus infinity anyway:
//   rows i < 0, columns j < 0, columns j > la and diagonals > dhi have nothing but masked cells above them (a column leaves the
//       band upwards at dhi, where the last lane reads minus infinity), so their E derives from minus infinity; their F is read
//       to the right only, by cells of the same row that are masked as well (j > la, d > dhi) or take the left boundary (j < 0:
//       all of row i left of column 0 is masked, so F(i, 0) = max(z, f) of minus infinities = "F is minus infinity in column 0").
//   rows i > lb are read by rows > lb only.
//   Row 0 and column 0 then come out of the plain recurrence: H(0, j) = F = gap_open + j ge from H(0, 0), E(0, j) = minus
//       infinity, and likewise down column 0.  H(0, 0) = 0 itself: when a lane reaches row 0 (one compare per step, taken once)
//       it sets the diagonal input of diagonal 0 -- "H(-1, -1)" -- to minus the mismatch score; padding never matches, so the
//       diagonal move gives exactly 0 and E, F there are minus infinity.  That value is also read as "up" by (0, -1), whose H is
//       masked and whose E feeds column -1 only.
//
// No wrap.  Minus infinity is kBandNegInf = -2^30.  A value derived from it has gap costs added along one row of the band (F) or
// one column's stretch inside the band (E) before a masked H cuts the chain: at most 2048 cells of at most 1000 each, so it
// stays above -2^30 - 2.05e6 > -2^31 and below -2^30 + 2048 * 12.  True values: an in-band cell of the matrix always has a path
// from the origin inside the band (along row 0 or column 0, then its diagonal), so under (12, -116, -1000, -1000) at
// la = lb = 65535 every true H lies within [-2000 - 131070 * 1000, 12 * 65535] = [-1.311e8, 7.9e5]; z, e and f add at most two
// gap costs to that.  -1.32e8 > -2^30 + 2.5e4: a true value always beats a derived minus infinity, and nothing wraps.
//
// Capture.  GLOBAL: the lane and register that own diagonal la - lb hold z of (lb, la) after the step of row lb.  EXTEND: every
// lane keeps the first strict improvement of its row maximum over its running maximum, which starts at H(0, 0) = 0 -- rows come
// in rising i, and within a row it takes the leftmost cell; masked cells are minus infinity and never win.  The group reduces by
// (score, then i, then j); the position word is i << 16 | j (both <= 65535).
//
// TRACE (agx_sw_band_trace_kernel.hip; include/agx.h, "CIGARs for banded batches"; DESIGN.md 4.1h): the corner-capture build also
// leaves four bits per cell -- bits 0-1 where H came from (0 the diagonal, 1 E, 2 F; ties prefer the diagonal, then E), bit 2
// "E extended" (ue + ge > uz, strictly), bit 3 "F extended" (f + ge > zleft, strictly).  A lane's K nibbles of a step are
// sw_band_trace_words(K) dwords at trace + goff[group] + (t G + gl) words: step-major, a group's lanes side by side, one store
// per lane and step (dwordx4 at K = 32).  Only rows 0 .. lb of the group are written, so a pair takes (lb + G) G words dwords
// whatever the wave's step count is.  The walk (sw_walk_band) finds cell (i, j) at slot = j - i - dlo, lane slot / K, nibble
// slot % K, step i + lane.
// The trace does not mask E and F either, and the bits of masked or boundary cells cannot steer the walk.  The walk starts at
// the corner, a true cell, reads cells with 1 <= i <= lb, 1 <= j <= la inside the band only, and ends at row 0 or column 0
// without reading them.  Every such cell has the true cell (i - 1, j - 1) on its own diagonal, so max(s, ev, f) is a true
// value; by "No wrap" a true value always beats one derived from minus infinity, so H never takes a source derived from minus
// infinity and bits 0-1 always point at a true cell.  Bit 2 is read in state E at a cell whose E is true (H chose it, or the
// cell below extended from it strictly): then max(uz, ue + ge) is true, and the bit is set only if ue + ge is the true one.
// Bit 3 likewise.  A strict "extended" bit computed from two derived minus infinities belongs to a cell whose E (or F) is
// itself derived, where the walk never stands in that state.  Along the edges:
//   band's right edge (d = dhi): "up" is diagonal dhi + 1 -- a masked slot or the last lane's minus infinity; uz and ue are
//       derived, E is derived, H does not choose it and nothing below extends from it.  F comes from diagonal dhi - 1, true.
//   band's left edge (d = dlo): "left" is the first lane's minus infinity, F is derived; E comes from diagonal dlo + 1, true.
//   row 1 reads row 0 as "up": H(0, j) is true for j <= dhi, E(0, j) derives from the masked rows above, so bit 2 is clear
//       and the walk reaches row 0 in state H.  Column 1 reads column 0 as "left": F(i, 0) is a maximum of minus infinities,
//       H(i, 0) is true for i <= -dlo, so bit 3 is clear and the walk reaches column 0 in state H.
//
// AT (agx_sw_band_diag_kernel.hip; include/agx.h, "Banded alignment around a diagonal"; DESIGN.md 4.1i): builds for a band around
// a caller-given diagonal in the modes whose boundaries or capture differ -- LOCAL (zero floor z >= gf, no injection, ANY
// capture), FIT (H = 0 in every in-band cell of column 0: the injection follows that column's slot -(i + d0) from step to step)
// and EXTEND_QUERY; the last two capture the best cell of column la, slot la - i - d0, rows 0 .. lb, smallest row first.  That
// file's head restates "No wrap" for them.  Nothing above assumes that the band is centred on the main diagonal: dlo and dhi come
// from the group record, and the host may hand the fill a target that starts at a later row with the band shifted accordingly.
//
// PH (agx_sw_band_diag_trace_kernel.hip; include/agx.h, "CIGARs for batches banded around a diagonal"; DESIGN.md 4.1j): the traced
// build for a span that begins INSIDE the resident image.  The group record's `reserved` holds a start phase r = 0 .. 3 and the
// step counter runs as t' = t - r: rows, injection, capture and the trace are in terms of t', the two loaders in terms of t, so
// that both still read whole dwords at t = 0 (mod 4).  That file's head has the argument and says what the bytes outside the span
// do.  r = 0 is the plain traced build, step for step.
//
// ZD (agx_sw_band_zdrop_kernel.hip; include/agx.h, "Z-drop for banded extension"; DESIGN.md 4.1k): the EXTEND build that stops a
// pair once its alignment has fallen apart.  A row's maximum and its leftmost column travel along the group's lanes one lane per
// step, as z_last does; the group's last lane sees the rows complete and in order, keeps the running best and applies the rule.
// Once per four steps the wave leaves when each of its groups has terminated or passed its last row.  That file's head has the
// argument.
//
// MAT (agx_sw_band_diag_mat_kernel.hip, agx_sw_band_diag_trace_mat_kernel.hip; include/agx.h, "Banded alignment around a diagonal
// under a substitution matrix"; DESIGN.md 4.1l): the builds whose diagonal move adds a substitution-matrix entry -- the plain, AT
// and traced-with-PH builds again, nothing else changed.  What the points above become:
//   Symbols.  The image holds symbol numbers 1 .. 32 (the host writes code + 1) and 0 is the padding in rows and columns alike,
//       as in the anchored matrix fill.  A row outside 1 .. lb carries 0, not kBandRowPad.  The table is the kSwMatDim x kSwMatDim
//       int16 table of the other matrix fills: entry [y][x] = score - gf, and EVERY entry of row 0 and of column 0 is one constant
//       P = (the matrix minimum, <= 0) - gf.  Every symbol a lane can hold -- from the image, from a neighbour by DPP, the preset
//       of an idle lane -- is 0 .. 32, so the lookup stays inside the table's 2178 bytes.
//   Origin and FIT injection.  The plain build sets the diagonal input to minus the mismatch score so that the move over padding
//       gives exactly 0; here it sets -P.  Cell (0, 0) of the pinned modes reads table[0][x]: its row symbol is 0 whatever x is
//       (the padding left of a, or under PH the stray symbol a[a_begin - 1]), and row 0 of the table is P throughout.  An in-band
//       cell (i, 0) of FIT reads table[code(b_i)][0] -- or table[0][0] in row 0 --: its column symbol is the padding left of a
//       (FIT has no PH build), and column 0 of the table is P throughout.  Both give -P + P = 0.
//   LDS table.  One copy per workgroup, loaded by the kernel (the including file) before the `wave >= n_waves` return.
//   Lookup schedule.  A step's K entries depend on the window's bytes and the row symbol only, both known at the step's head: all
//       K reads are issued there, and the chain waits with a falling lgkmcnt, once per cell, for an entry that was asked for
//       before the injection, the mask and the cells to its left (the K = 8 disassembly: eight ds_read_u16 in a row about fifty
//       instructions ahead of the first use, then s_waitcnt lgkmcnt(7) .. (0); the entry is sign-extended by the SDWA add).
//       The price is K registers a step for the entries.
//   No wrap.  Entries are int8, so a diagonal move adds -128 .. 127 (as z: -128 - gf .. 127 - gf, within int16), over at most
//       65 535 moves of a path; gap costs are unchanged.  True values: an in-band cell still has its path from the origin along
//       row 0 or column 0 and then its diagonal, so a pinned H lies within [-2000 - 131070 * 1000 - 65535 * 128, 127 * 65535] =
//       [-1.395e8, 8.33e6]; z, e and f add at most two gap costs.  A value derived from minus infinity is -2^30 plus at most one
//       row's or one column stretch's gap costs (<= 0) plus at most one diagonal move before a masked H cuts the chain (a cell
//       that exists and takes it has a true competitor, below): within [-2^30 - 2.05e6 - 128, -2^30 + 2127].  -1.4e8 > -2^30 +
//       2127, so a true value still beats a derived one, and nothing comes near +-2^31.  LOCAL: the floor replaces a derived
//       value by 0 only in cells that exist, where 0 is true, and a LOCAL H lies in [0, 127 * 65535]; FIT's H is at least the
//       pinned one.  The traced build's argument -- every cell the walk reads has the true cell (i - 1, j - 1) on its diagonal,
//       so its maximum is true and bits 0-1 point at a true source -- reads the same with "plus the table's entry" for "plus
//       match or mismatch".
//   Walk.  sw_walk_band_at compares image bytes: under MAT symbol numbers, so '=' is "identical codes", as the contract words it.
//
// STATS (agx_sw_band_stats_kernel.hip; include/agx.h, "Statistics for batches banded around a diagonal"; DESIGN.md 4.1m): the
// builds whose states are tuples (score, L), L = matches << 16 | pairs of the state's best path, held as one int64
// score << 32 | L: the plain GLOBAL and EXTEND builds and the AT builds of LOCAL and EXTEND_QUERY again.  Max is a 64-bit compare,
// gaps add to the score word only, a diagonal move also counts its pair unless it runs over padding, a masked cell is (minus
// infinity, 0), every hand-over between lanes carries both words, and capture reads the score word alone: lstat[out] receives L
// of the cell the plain build would have captured.  That file's head has the argument, for the low word above all.
//
// DUAL (agx_sw_band_dual_kernel.hip; include/agx.h, "Banded alignment around a diagonal under two-piece gap costs"; DESIGN.md
// 4.1n): the builds whose gaps cost the cheaper of two affine pieces -- the plain GLOBAL and EXTEND builds and the three AT builds
// again.  A second pair of gap states, e2 per diagonal and f2 along the chain, runs beside e and f under the second piece's
// extension cost ge2; both read the one stored z = H + gf of the first piece plus dgf = gf2 - gf, and H takes the maximum over
// all five.  Every hand-over between lanes carries the second piece as well.  That file's head has the argument.
// With TRACE and PH as well (agx_sw_band_dual_trace_kernel.hip; include/agx.h, "CIGARs for batches banded around a diagonal under
// two-piece gap costs"; DESIGN.md 4.1o) a cell leaves a BYTE -- where H came from among five states, one strict "extended" bit
// per gap state -- in sw_band_dual_trace_words(K) = K / 4 dwords a lane and step; that file's head restates "No wrap", the
// masked cells and "no bit steers the walk" for five sources.
//
// (included by the ten agx_sw_band*_kernel.hip; opens an anonymous namespace that the including file closes after its kernels, ahead
// of its launch entry.  The foot of this file has what those entries are made of.)
#include "agx_sw.h"

namespace {

constexpr int kBandRowPad = 0x100; // never equals a byte
constexpr int kBandNegInf = -(1 << 30);

__device__ __forceinline__ int band_shr1(int old, int v)
{
    // DPP wave_shr:1 -- lane i receives lane i-1's v; lane 0 keeps old
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int band_shl1(int old, int v)
{
    // DPP wave_shl:1 -- lane i receives lane i+1's v; lane 63 keeps old
    return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xf, 0xf, false);
}

// A state: the score (int) or, in the STATS builds, the tuple score << 32 | L (long long).  One set of operations for both; on
// int they are the plain build's expressions.
template <bool STATS>
struct BandState {
    using type = int;
};
template <>
struct BandState<true> {
    using type = long long;
};
__device__ __forceinline__ int band_gap(int v, int c) { return v + c; }
__device__ __forceinline__ int band_max(int x, int y) { return max(x, y); }
__device__ __forceinline__ int band_score(int v) { return v; }
__device__ __forceinline__ uint32_t band_low(int) { return 0u; }
__device__ __forceinline__ long long band_tuple(int score, uint32_t l) { return (long long)(((unsigned long long)(uint32_t)score << 32) | l); }
__device__ __forceinline__ int band_score(long long v) { return (int)(v >> 32); }
__device__ __forceinline__ uint32_t band_low(long long v) { return (uint32_t)v; }
// the two words are added apart: nothing carries from L into the score
__device__ __forceinline__ long long band_gap(long long v, int c) { return band_tuple(band_score(v) + c, band_low(v)); }
__device__ __forceinline__ long long band_max(long long x, long long y) { return x > y ? x : y; }
// The diagonal move of a cell with window byte xs and row symbol yc.  A match is never over padding (kBandRowPad equals no byte,
// and the padding byte 0 no symbol); a mismatch counts its pair only in a row 1 .. lb (pair1) and a column 1 .. la (xs != 0).
__device__ __forceinline__ long long band_pair_move(long long zd, int xs, int yc, int s_match, int s_mis, uint32_t pair1)
{
    const bool same = xs == yc;
    return band_tuple(band_score(zd) + (same ? s_match : s_mis), band_low(zd) + (same ? 0x10001u : xs ? pair1 : 0u));
}
__device__ __forceinline__ long long band_shr1(long long old, long long v)
{
    return band_tuple(band_shr1(band_score(old), band_score(v)), (uint32_t)band_shr1((int)band_low(old), (int)band_low(v)));
}
__device__ __forceinline__ long long band_shl1(long long old, long long v)
{
    return band_tuple(band_shl1(band_score(old), band_score(v)), (uint32_t)band_shl1((int)band_low(old), (int)band_low(v)));
}

// A build of the body is a mask F of these variants, named above, and AT.  A kernel names the ones it is built with and nothing
// else: band_body<K, kBandTrace | kBandPh | kBandDual>(prm, img, groups, waves[wave], io).
enum : unsigned {
    kBandExt = 1u << 0,   // EXT: capture the best cell by the ANY rule, not the corner
    kBandTrace = 1u << 1, // TRACE
    kBandPh = 1u << 2,    // PH
    kBandZd = 1u << 3,    // ZD
    kBandMat = 1u << 4,   // MAT: the builds under a substitution matrix; sub is the table in LDS
    kBandStats = 1u << 5, // STATS: the builds on tuples; lstat receives L of the captured cell
    kBandDual = 1u << 6,  // DUAL: the builds under two-piece gap costs
};
// EXT of a kernel that is built per mode or capture: band_ext(MODE == AGX_SW_MODE_LOCAL) | kBandStats
constexpr unsigned band_ext(bool on) { return on ? (unsigned)kBandExt : 0u; }

// What a build reads and writes besides the records: a kernel sets the members its variants use.
struct BandIo {
    int32_t *scores = nullptr;
    uint32_t *pos = nullptr;        // EXT and the AT builds
    uint32_t *trace = nullptr;      // TRACE
    const uint64_t *goff = nullptr; // TRACE
    int zdrop = 0;                  // ZD
    int32_t *stops = nullptr;       // ZD
    const int16_t *sub = nullptr;   // MAT
    uint32_t *lstat = nullptr;      // STATS
    int ge2 = 0, dgf = 0;           // DUAL: the second piece's extension cost, and its first-cell cost less gf
};

// AT: -1 for the builds above; else the mode of a build of agx_sw_band_diag_kernel.hip (LOCAL: EXT is set, it captures by the
// ANY rule; FIT and EXTEND_QUERY capture column la).  Everything they add stands inside `if constexpr` blocks.
template <int K, unsigned F, int AT = -1>
__device__ __forceinline__ void band_body(const SwParams &prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                          const SwWave w, const BandIo &io)
{
    int32_t *__restrict__ const scores = io.scores;
    uint32_t *__restrict__ const pos = io.pos;
    uint32_t *const trace = io.trace;
    const uint64_t *const goff = io.goff;
    [[maybe_unused]] const int zdrop = io.zdrop;
    [[maybe_unused]] int32_t *__restrict__ const stops = io.stops;
    [[maybe_unused]] const int16_t *const sub = io.sub;
    [[maybe_unused]] uint32_t *__restrict__ const lstat = io.lstat;
    [[maybe_unused]] const int ge2 = io.ge2, dgf = io.dgf;
    constexpr bool EXT = F & kBandExt, TRACE = F & kBandTrace, PH = F & kBandPh, ZD = F & kBandZd, MAT = F & kBandMat, STATS = F & kBandStats,
                   DUAL = F & kBandDual;
    static_assert(!(TRACE && EXT), "the traced build captures the corner: an EXTEND span is traced as the global alignment it is");
    static_assert(K % 4 == 0 && K >= 4 && K <= 32, "the query window is whole dwords and the cell mask one dword");
    static_assert(AT == -1 || (!TRACE && EXT == (AT == AGX_SW_MODE_LOCAL) &&
                               (AT == AGX_SW_MODE_LOCAL || AT == AGX_SW_MODE_FIT || AT == AGX_SW_MODE_EXTEND_QUERY)),
                  "GLOBAL and EXTEND around a diagonal run the plain builds: their boundaries and captures are the same");
    static_assert(!PH || (TRACE && AT == -1), "the start phase belongs to the traced build");
    static_assert(!ZD || (EXT && !TRACE && AT == -1), "the z-drop belongs to the plain EXTEND build");
    static_assert(!MAT || !ZD, "no z-drop under a matrix");
    static_assert(!STATS || (!TRACE && !PH && !ZD && !MAT && AT != AGX_SW_MODE_FIT),
                  "statistics ride on the plain GLOBAL and EXTEND builds and on the LOCAL and EXTEND_QUERY builds around a diagonal");
    static_assert(!DUAL || (TRACE == PH && !ZD && !MAT && !STATS),
                  "two-piece gap costs: the untraced builds, and the traced build with the start phase (its batches are banded around a diagonal)");
    using V = typename BandState<STATS>::type;
    constexpr V kNeg = STATS ? (V)((unsigned long long)(uint32_t)kBandNegInf << 32) : (V)kBandNegInf; // STATS: (minus infinity, 0)
    constexpr bool AT_LOCAL = AT == AGX_SW_MODE_LOCAL, AT_FIT = AT == AGX_SW_MODE_FIT, AT_COL = AT_FIT || AT == AGX_SW_MODE_EXTEND_QUERY;
    constexpr int XW = K / 4;
    const int ge = prm.ge, gf = prm.gf, s_match = prm.hd, s_mis = prm.hd - prm.delta; // the diagonal move on z: score - gf
    // what a row outside 1 .. lb carries, and the diagonal input that the move over padding turns into exactly 0 (MAT: minus the
    // table's padding entry, which every entry of row 0 and of column 0 holds)
    constexpr int kRowPad = MAT ? 0 : kBandRowPad;
    [[maybe_unused]] int inject = 0;
    if constexpr (MAT) inject = -(int)sub[0];
    const int lane = threadIdx.x & 63;
    const int G = w.G;
    const int grp = lane / G;
    const int gl = lane - grp * G;
    const bool active = grp < (int)w.n_groups;
    const bool first = gl == 0, last = gl == G - 1;

    SwBandGroup g;
    g.x_dw = g.y_dw = g.la_lb = g.out = g.fpad = g.reserved = 0;
    g.dlo = g.dhi = 0;
    if (active) g = groups[w.first_group + grp];
    const int la = (int)(g.la_lb & 0xffffu), lb = (int)(g.la_lb >> 16);
    const int d0 = g.dlo + gl * K;
    const int kmax = min(K - 1, g.dhi - d0); // the last in-band slot of this lane (negative: none)
    const int k0 = -d0;                      // the slot of diagonal 0, if this lane owns it
    [[maybe_unused]] int ph = 0, glp = gl; // PH: the start phase, and gl + r: this lane's row at step t is t - glp
    if constexpr (PH) {
        ph = (int)(g.reserved & 3u);
        glp = gl + ph;
    }

    // the query window at step 0: a[j0 - 1 + k], j0 = d0 - gl
    uint32_t xw[XW];
    {
        const uint8_t *ab = reinterpret_cast<const uint8_t *>(img + g.x_dw) + g.fpad;
#pragma unroll
        for (int n = 0; n < XW; ++n) xw[n] = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int idx = d0 - (PH ? glp : gl) - 1 + k; // (PH: the row at step 0 is -gl - r)
            const uint32_t by = (active && idx >= 0 && idx < la) ? ab[idx] : 0u;
            xw[k >> 2] |= by << (8 * (k & 3));
        }
    }
    // the two loaders: b at the group's first lane, the query byte that enters the band at its last lane
    const bool feeder = active && first, loader = active && last;
    const uint32_t *yp = img + g.y_dw;
    const int nyq = (lb + (PH ? ph : 0) + 4) >> 2; // one byte in front of b (PH: and r more)
    auto row_quad = [&](int q) -> uint32_t { return (feeder && q < nyq) ? yp[q] : 0u; };
    const uint32_t *xp = img + g.x_dw;
    const int q0x = g.dlo + G * K - G;      // a[q0x + t] enters at step t
    const int rel0 = ((int)g.fpad + q0x - (PH ? ph : 0)) / 4; // exact: the host chose fpad so
    const int nxd = ((int)g.fpad + la + 3) >> 2;
    auto col_quad = [&](int q) -> uint32_t { return (loader && (uint32_t)(rel0 + q) < (uint32_t)nxd) ? xp[rel0 + q] : 0u; };

    V z[K], e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = e[k] = kNeg;
    V z_last = kNeg, f_last = kNeg;
    // DUAL: the second piece's E per diagonal and its F as the step's last cell left it
    [[maybe_unused]] V e2[DUAL ? K : 1];
    [[maybe_unused]] V f2_last = kNeg;
    if constexpr (DUAL) {
#pragma unroll
        for (int k = 0; k < K; ++k) e2[k] = kNeg;
    }
    int yc_prev = kRowPad;
    // STATS: L of the cell that `best` / `corner` / `cbest` was read from
    [[maybe_unused]] uint32_t hit_l = 0;
    int best = gf, hit_i = -1, hit_k = 0; // EXTEND: H(0, 0) = 0 as z
    int corner = 0;                       // GLOBAL
    const int dc = la - lb - g.dlo;       // GLOBAL: the corner's diagonal, counted from dlo
    const int kc = dc - gl * K;           // its slot here, if 0 <= kc < K
    [[maybe_unused]] int cbest = kBandNegInf, cap_i = -1; // AT_COL: the best z of column la so far and its row
    // ZD: the carrier -- the maximum of this lane's row over the lanes up to this one and its leftmost column, as this lane left
    // it in the step before -- and, meaningful in the group's last lane only, the running best B (as z) with its cell and the stop
    [[maybe_unused]] int car_m = kBandNegInf, car_c = 0, zb = gf, zbi = 0, zbj = 0, zstop = -1;

    // TRACE: this lane's nibbles of step t go to tp + t G TW
    constexpr int TW = DUAL ? sw_band_dual_trace_words(K) : sw_band_trace_words(K);
    uint32_t *tp = nullptr;
    if constexpr (TRACE) {
        if (active) tp = trace + goff[w.first_group + grp] + (uint32_t)(gl * TW);
        if constexpr (PH) tp -= ph * G * TW; // step t writes at t' = t - r; nothing is stored before t' = gl
    }

    uint32_t q0 = row_quad(0), q1 = row_quad(1), q2 = row_quad(2);
    uint32_t x0 = col_quad(0), x1 = col_quad(1), x2 = col_quad(2);
    const int steps = (int)w.steps;
    uint32_t rows = 0, xrows = 0;
    int t = 0;

    auto step = [&]() __attribute__((always_inline)) {
        const int i = t - (PH ? glp : gl);
        // (PH: 1 <= t' <= lb is 1 <= i <= lb in a group's first lane, and no other lane's `fresh` is read)
        const int fresh = (PH ? (uint32_t)(i - 1) < (uint32_t)lb : (t >= 1 && t <= lb)) ? (int)(rows & 0xffu) : kRowPad;
        rows >>= 8;
        const uint32_t xin = xrows & 0xffu;
        xrows >>= 8;
        V zl = band_shr1(kNeg, z_last);
        V fl = band_shr1(kNeg, f_last);
        int yc = band_shr1(fresh, yc_prev);
        [[maybe_unused]] V fl2 = kNeg;
        if constexpr (DUAL) fl2 = band_shr1(kNeg, f2_last);
        if (first) {
            zl = kNeg;
            fl = kNeg;
            yc = fresh;
            if constexpr (DUAL) fl2 = kNeg;
        }
        // MAT: the K entries of this step -- row yc of the table, the columns of the window's bytes -- depend on nothing the cell
        // chain computes: all K reads are issued here, ahead of the injection, the mask and the chain, which then waits for
        // each entry once it needs it and not for one LDS round trip per cell
        [[maybe_unused]] int sc[MAT ? K : 1];
        if constexpr (MAT) {
            const char *row = reinterpret_cast<const char *>(sub) + yc * (kSwMatDim * 2);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int xs = (int)((xw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                sc[k] = *reinterpret_cast<const int16_t *>(row + xs * 2);
            }
        }
        if constexpr (AT_FIT) {
            // column 0 of this lane's row: the diagonal input that makes H(i, 0) = 0 in every row 0 .. lb.  The slot moves down by
            // one per step and crosses the lanes; the branch is taken only while column 0 is inside the band (2w + 1 rows).
            int slot = -(i + d0);
            if ((uint32_t)slot < (uint32_t)K && (uint32_t)i <= (uint32_t)lb) {
                asm volatile("" : "+v"(slot));
#pragma unroll
                for (int k = 0; k < K; ++k) z[k] = k == slot ? (MAT ? inject : -s_mis) : z[k];
            }
        } else if constexpr (AT_LOCAL) {
            // no injection: a diagonal input of minus infinity under the zero floor gives H = 0 on row 0 and in column 0
        } else if (i == 0) { // row 0 of this lane: the diagonal input that makes H(0, 0) = 0
            // (the slot is compared here, once per lane: hoisted out of the loop the K compares hold K scalar register pairs)
            int slot = k0;
            asm volatile("" : "+v"(slot));
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if constexpr (STATS) z[k] = k == slot ? band_tuple(-s_mis, 0u) : z[k]; // the move over padding adds nothing to L
                else z[k] = k == slot ? (MAT ? inject : -s_mis) : z[k];
            }
        }
        // which of this step's cells exist
        const int j0 = i + d0;
        const int klo = max(0, -j0), khi = min(kmax, la - j0);
        const bool any = (uint32_t)i <= (uint32_t)lb && khi >= klo;
        const uint32_t mask = any ? ((2u << (khi & 31)) - 1u) & (~0u << (klo & 31)) : 0u;
        auto keep = [&](V v, int k) -> V {
            const int m = (int)(mask << (31 - k)) >> 31; // all ones where cell k exists
            if constexpr (STATS) return band_tuple((band_score(v) & m) | (kBandNegInf & ~m), band_low(v) & (uint32_t)m); // (minus infinity, 0)
            else return (v & m) | (kBandNegInf & ~m);
        };
        // STATS: what a mismatch adds to L in this step's row: its pair, unless the row lies outside 1 .. lb
        [[maybe_unused]] uint32_t pair1 = 0;
        if constexpr (STATS) pair1 = yc != kRowPad ? 1u : 0u;

        // TRACE, per cell: where H came from (diagonal, then E, then F) | E extended << 2 | F extended << 3, both strictly:
        // ue + ge > uz is ev > uz, and f + ge > zleft is the new f > the left cell's z, which z[k - 1] still holds.  Everything
        // the trace computes stands inside its own blocks: the untraced builds compile to the code they had without it.  The
        // nibble joins its dword at once and the chain passes through the same empty statement, so that no cell is begun before
        // the nibble of the cell on its left is made: left to the scheduler, s, ev and f of all K cells stay live to the step's end.
        [[maybe_unused]] uint32_t tw[TW];
        [[maybe_unused]] auto dirs = [](int s, int ev, int f, bool e_ext, bool f_ext) -> uint32_t {
            const uint32_t src = s >= max(ev, f) ? 0u : ev >= f ? 1u : 2u;
            return src | (e_ext ? 4u : 0u) | (f_ext ? 8u : 0u);
        };
        // TRACE with DUAL, per cell one byte: bits 0-1 where H came from as above (the RAW diagonal move first, then the better of
        // the two E, then of the two F), bit 2 "of piece 2" (piece 1 wins a tie within a direction), bits 4-7 E1, F1, E2, F2 extended,
        // each strictly under its own piece: ue2 + ge2 > uz + dgf is ev2 > uz + dgf, and its F twin.
        [[maybe_unused]] auto dirs2 = [](int s, int ev, int f, int ev2, int f2, bool e_ext, bool f_ext, bool e2_ext, bool f2_ext) -> uint32_t {
            const int em = max(ev, ev2), fm = max(f, f2);
            const uint32_t src = s >= max(em, fm) ? 0u : em >= fm ? (ev >= ev2 ? 1u : 5u) : (f >= f2 ? 2u : 6u);
            return src | (e_ext ? 16u : 0u) | (f_ext ? 32u : 0u) | (e2_ext ? 64u : 0u) | (f2_ext ? 128u : 0u);
        };

        // phase 1: the first cell
        V f, zleft;
        [[maybe_unused]] V f2 = kNeg;
        {
            const V ev = band_max(z[1], band_gap(e[1], ge));
            f = band_max(zl, band_gap(fl, ge));
            [[maybe_unused]] V ev2 = kNeg;
            if constexpr (DUAL) {
                ev2 = band_max(band_gap(z[1], dgf), band_gap(e2[1], ge2));
                f2 = band_max(band_gap(zl, dgf), band_gap(fl2, ge2));
            }
            V s;
            if constexpr (MAT) s = z[0] + sc[0];
            else {
                const int xs = (int)(xw[0] & 0xffu);
                if constexpr (STATS) s = band_pair_move(z[0], xs, yc, s_match, s_mis, pair1);
                else s = z[0] + (xs == yc ? s_match : s_mis);
            }
            if constexpr (DUAL) {
                if constexpr (TRACE) { // the byte is made here: it asks the RAW diagonal move, before s takes in E2 and F2
                    tw[0] = dirs2(s, ev, f, ev2, f2, ev > z[1], f > zl, ev2 > band_gap(z[1], dgf), f2 > band_gap(zl, dgf));
#pragma unroll
                    for (int n = 1; n < TW; ++n) tw[n] = 0;
                }
                s = band_max(s, band_max(ev2, f2)); // H over all five: the diagonal move and both pieces' E and F
            }
            if constexpr (AT_LOCAL) zleft = keep(band_gap(band_max(band_max(band_max(ev, f), s), (V)0), gf), 0); // the zero floor: z >= gf
            else zleft = keep(band_gap(band_max(band_max(ev, f), s), gf), 0);
            if constexpr (TRACE && DUAL) {
                asm volatile("" : "+v"(tw[0]), "+v"(zleft));
            } else if constexpr (TRACE) {
                tw[0] = dirs(s, ev, f, ev > z[1], f > zl);
#pragma unroll
                for (int n = 1; n < TW; ++n) tw[n] = 0;
                asm volatile("" : "+v"(tw[0]), "+v"(zleft));
            }
            e[0] = ev;
            if constexpr (DUAL) e2[0] = ev2;
            z[0] = zleft;
        }
        // phase 2: it is the up input of the left neighbour's last diagonal
        V rz = band_shl1(kNeg, z[0]);
        V re = band_shl1(kNeg, e[0]);
        [[maybe_unused]] V re2 = kNeg;
        if constexpr (DUAL) re2 = band_shl1(kNeg, e2[0]);
        if (last) {
            rz = re = kNeg;
            if constexpr (DUAL) re2 = kNeg;
        }
#pragma unroll
        for (int k = 1; k < K; ++k) {
            const V uz = k + 1 < K ? z[k + 1] : rz;
            const V ue = k + 1 < K ? e[k + 1] : re;
            const V ev = band_max(uz, band_gap(ue, ge));
            f = band_max(zleft, band_gap(f, ge));
            [[maybe_unused]] V ev2 = kNeg;
            if constexpr (DUAL) {
                const V ue2 = k + 1 < K ? e2[k + 1] : re2;
                ev2 = band_max(band_gap(uz, dgf), band_gap(ue2, ge2));
                f2 = band_max(band_gap(zleft, dgf), band_gap(f2, ge2));
            }
            V s;
            if constexpr (MAT) s = z[k] + sc[k];
            else {
                const int xs = (int)((xw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                if constexpr (STATS) s = band_pair_move(z[k], xs, yc, s_match, s_mis, pair1);
                else s = z[k] + (xs == yc ? s_match : s_mis);
            }
            if constexpr (DUAL) {
                if constexpr (TRACE)
                    tw[k >> 2] |= dirs2(s, ev, f, ev2, f2, ev > uz, f > z[k - 1], ev2 > band_gap(uz, dgf), f2 > band_gap(z[k - 1], dgf)) << (8 * (k & 3));
                s = band_max(s, band_max(ev2, f2));
            }
            if constexpr (AT_LOCAL) zleft = keep(band_gap(band_max(band_max(band_max(ev, f), s), (V)0), gf), k);
            else zleft = keep(band_gap(band_max(band_max(ev, f), s), gf), k);
            if constexpr (TRACE && DUAL) {
                asm volatile("" : "+v"(tw[k >> 2]), "+v"(zleft));
            } else if constexpr (TRACE) {
                tw[k >> 3] |= dirs(s, ev, f, ev > uz, f > z[k - 1]) << (4 * (k & 7));
                asm volatile("" : "+v"(tw[k >> 3]), "+v"(zleft));
            }
            e[k] = ev;
            if constexpr (DUAL) e2[k] = ev2;
            z[k] = zleft;
        }

        if constexpr (TRACE) { // rows 0 .. lb of this group only: the wave may step on for a longer neighbour
            if (active && (uint32_t)i <= (uint32_t)lb) {
                if constexpr (TW == 8) {
                    reinterpret_cast<uint4 *>(tp)[0] = make_uint4(tw[0], tw[1], tw[2], tw[3]);
                    reinterpret_cast<uint4 *>(tp)[1] = make_uint4(tw[4], tw[5], tw[6], tw[7]);
                } else if constexpr (TW == 4) *reinterpret_cast<uint4 *>(tp) = make_uint4(tw[0], tw[1], tw[2], tw[3]);
                else if constexpr (TW == 2) *reinterpret_cast<uint2 *>(tp) = make_uint2(tw[0], tw[1]);
                else tp[0] = tw[0];
            }
            tp += G * TW;
        }

        if constexpr (ZD) {
            // the row's maximum so far arrives from the lane that finished this row one step ago; this lane's own maximum wins on
            // a strict improvement only (the lower lanes hold the smaller columns), masked cells are minus infinity and never do
            int rm = band_shr1(kBandNegInf, car_m);
            int rc = band_shr1(0, car_c);
            if (first) rm = kBandNegInf;
            int m = z[0];
#pragma unroll
            for (int k = 1; k < K; ++k) m = max(m, z[k]);
            int col = 0;
#pragma unroll
            for (int k = K - 1; k >= 0; --k) col = z[k] == m ? k : col; // the leftmost cell of the row that holds it
            const bool mine = m > rm;
            car_m = mine ? m : rm;
            car_c = mine ? j0 + col : rc;
            // the rule, rows 1 .. lb in order (lb is the last row with an in-band cell: the host trims the rows to the band).  Every
            // lane runs it on what it holds; the group's last lane holds R(i) and c(i), and only its outcome is read
            if ((uint32_t)(i - 1) < (uint32_t)lb && zstop < 0) {
                if (car_m > zb) {
                    zb = car_m;
                    zbi = i;
                    zbj = car_c;
                } else if (zb - car_m > zdrop - ge * abs((i - zbi) - (car_c - zbj))) {
                    zstop = i - 1;
                }
            }
        } else if constexpr (EXT) {
            int m = band_score(z[0]);
#pragma unroll
            for (int k = 1; k < K; ++k) m = max(m, band_score(z[k]));
            if (m > best) { // a higher score than in any earlier row of this lane's diagonals
                int col = 0;
#pragma unroll
                for (int k = K - 1; k >= 0; --k) col = band_score(z[k]) == m ? k : col; // the leftmost cell of the row that holds it
                if constexpr (STATS) { // ... chosen by its score alone; L is read there
#pragma unroll
                    for (int k = K - 1; k >= 0; --k) hit_l = band_score(z[k]) == m ? band_low(z[k]) : hit_l;
                }
                best = m;
                hit_i = i;
                hit_k = col;
            }
        } else if constexpr (AT_COL) {
            // cell (i, la) stands in slot la - i - d0, which also moves by one per step; rows 0 .. lb only.  A masked cell is
            // exactly minus infinity and never improves on the start value; rows come in rising i, so the smallest i wins.
            int slot = la - i - d0;
            if ((uint32_t)slot < (uint32_t)K && (uint32_t)i <= (uint32_t)lb) {
                asm volatile("" : "+v"(slot));
                V v = kNeg;
#pragma unroll
                for (int k = 0; k < K; ++k) v = k == slot ? z[k] : v;
                if (band_score(v) > cbest) {
                    cbest = band_score(v);
                    cap_i = i;
                    if constexpr (STATS) hit_l = band_low(v);
                }
            }
        } else {
            if (i == lb) {
                int slot = kc; // (as above)
                asm volatile("" : "+v"(slot));
#pragma unroll
                for (int k = 0; k < K; ++k) corner = k == slot ? band_score(z[k]) : corner;
                if constexpr (STATS) {
#pragma unroll
                    for (int k = 0; k < K; ++k) hit_l = k == slot ? band_low(z[k]) : hit_l;
                }
            }
        }

        // the query window moves on by one symbol
        const uint32_t nb = (uint32_t)band_shl1(0, (int)xw[0]);
        const uint32_t top = last ? xin : nb >> 8;
#pragma unroll
        for (int n = 0; n + 1 < XW; ++n) xw[n] = __builtin_amdgcn_alignbyte(xw[n + 1], xw[n], 1);
        xw[XW - 1] = __builtin_amdgcn_alignbyte(top, xw[XW - 1], 1);

        z_last = zleft;
        f_last = f;
        if constexpr (DUAL) f2_last = f2;
        yc_prev = yc;
        ++t;
    };

    const int quads = steps >> 2;
    for (int q = 0; q < quads; ++q) {
        if constexpr (ZD) {
            // leave once every group of the wave has terminated or passed its last row: the vote of a group is its last lane's
            if (__builtin_amdgcn_ballot_w64(loader && zstop < 0 && t - gl <= lb) == 0) {
                t = steps;
                break;
            }
        }
        rows = q0;
        q0 = q1;
        q1 = q2;
        q2 = row_quad(q + 3);
        xrows = x0;
        x0 = x1;
        x1 = x2;
        x2 = col_quad(q + 3);
#pragma unroll
        for (int b = 0; b < 4; ++b) step();
    }
    rows = q0;
    xrows = x0;
#pragma unroll 1
    while (t < steps) step();

    if constexpr (ZD) {
        if (loader) {
            scores[g.out] = zb - gf;
            pos[g.out] = zbi == 0 ? 0xffffffffu : ((uint32_t)zbi << 16) | (uint32_t)zbj;
            stops[g.out] = zstop;
        }
    } else if constexpr (EXT) {
        best -= gf;
        uint32_t key = hit_i < 0 ? 0xffffffffu : ((uint32_t)hit_i << 16) | (uint32_t)(hit_i + d0 + hit_k);
        // over the group's lanes by the rule: score, then row, then column (G need not be a power of two)
        for (int o = 1; o < G; o <<= 1) {
            const int ob = __shfl_down(best, o);
            const uint32_t ok = (uint32_t)__shfl_down((int)key, o);
            [[maybe_unused]] uint32_t ol = 0;
            if constexpr (STATS) ol = (uint32_t)__shfl_down((int)hit_l, o);
            if (gl + o < G && (ob > best || (ob == best && ok < key))) {
                best = ob;
                key = ok;
                if constexpr (STATS) hit_l = ol; // L travels with the winner
            }
        }
        if (feeder) {
            scores[g.out] = best;
            pos[g.out] = key;
            if constexpr (STATS) lstat[g.out] = hit_l; // (0 where no cell beat H(0, 0) = 0: nothing consumed)
        }
    } else if constexpr (AT_COL) {
        // over the group's lanes: score, then row (no lane of an admitted pair's group is without a cell of column la)
        uint32_t key = (uint32_t)cap_i;
        for (int o = 1; o < G; o <<= 1) {
            const int ob = __shfl_down(cbest, o);
            const uint32_t ok = (uint32_t)__shfl_down((int)key, o);
            [[maybe_unused]] uint32_t ol = 0;
            if constexpr (STATS) ol = (uint32_t)__shfl_down((int)hit_l, o);
            if (gl + o < G && (ob > cbest || (ob == cbest && ok < key))) {
                cbest = ob;
                key = ok;
                if constexpr (STATS) hit_l = ol;
            }
        }
        if (feeder) {
            scores[g.out] = cbest - gf;
            pos[g.out] = key;
            if constexpr (STATS) lstat[g.out] = hit_l;
        }
    } else {
        if (active && kc >= 0 && kc < K) {
            scores[g.out] = corner - gf;
            if constexpr (STATS) lstat[g.out] = hit_l;
        }
    }
}

// ---- the host side of a translation unit, written once

// One fill launch.  kernels[c][m] is the unit's kernel for K = kSwBandClasses[c] and mode modes[m]; a unit with one build per
// class, whatever the mode, passes {mode}.  (Class by class, and within a class in the order of `modes`, is also the order in
// which the kernels stand in the unit's code object.)  Four waves a workgroup.
// -> 0, -1 the launch failed, -2 no such class or mode
template <typename Kernel, size_t N, typename... Args>
int band_launch_fill(const Kernel (&kernels)[kSwNumBandClasses][N], const int (&modes)[N], int K, int mode, uint32_t n_waves, hipStream_t s,
                     const Args &...args)
{
    if (n_waves == 0) return 0;
    const size_t c = std::find(kSwBandClasses, kSwBandClasses + kSwNumBandClasses, K) - kSwBandClasses;
    const size_t m = std::find(modes, modes + N, mode) - modes;
    if (c == kSwNumBandClasses || m == N) return -2;
    hipLaunchKernelGGL(kernels[c][m], dim3((n_waves + 3) / 4), dim3(256), 0, s, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// one walk launch: a lane per pair
template <typename Kernel>
int band_launch_walk(Kernel kernel, const SwBandWalkArgs &a, hipStream_t s)
{
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(kernel, dim3((a.n + 63u) / 64u), dim3(64), 0, s, a.recs, a.band, a.n, a.img, a.trace, a.slots, a.runs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// loads the unit's code object ahead of the first launch
inline void band_preload(std::initializer_list<const void *> kernels)
{
    hipFuncAttributes a;
    for (const void *k : kernels) (void)hipFuncGetAttributes(&a, k);
}

