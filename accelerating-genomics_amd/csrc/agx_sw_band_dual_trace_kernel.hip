// The TRACED banded fill and the walk UNDER TWO-PIECE AFFINE GAP COSTS (agx_sw_batch_create_align_band_diag_dual_cigar;
// include/agx.h, "CIGARs for batches banded around a diagonal under two-piece gap costs").  The body is
// agx_sw_band_kernel.inc built with TRACE, PH and DUAL together: the corner-capture, start-phase build of
// agx_sw_band_diag_trace_kernel.hip (records, phase, loaders and stray bytes as its head says) with the cell of
// agx_sw_band_dual_kernel.hip (five states, z = H + gf stored once, piece 2 reads it as z + dgf).  One build per K = diagonals per
// lane, sw_fill_band_trace_dual<K>, and one walk, sw_walk_band_dual.
//
// The cell's byte.  Each cell of rows 0 .. cb leaves eight bits:
//   bits 0-1  where H came from: 0 the diagonal move, 1 E (a D), 2 F (an I).  The RAW diagonal move s is asked, before the DUAL
//             code folds max(E2, F2) into it: 0 iff s >= max(E1, E2, F1, F2); else E iff max(E1, E2) >= max(F1, F2); else F
//   bit 2     the chosen direction's piece: clear if piece 1's value is >= piece 2's, set otherwise (meaningless with source 0)
//   bit 4     E1 extended:  E1(i - 1, j) + ge  > H(i - 1, j) + gf    i.e. ev  > uz          strictly
//   bit 5     F1 extended:  F1(i, j - 1) + ge  > H(i, j - 1) + gf    i.e. f   > zleft       ...
//   bit 6     E2 extended:  E2(i - 1, j) + ge2 > H(i - 1, j) + gf2   i.e. ev2 > uz + dgf
//   bit 7     F2 extended:  F2(i, j - 1) + ge2 > H(i, j - 1) + gf2   i.e. f2  > zleft + dgf
//   (bit 3 is always clear.)
// A lane's K bytes of a step are sw_band_dual_trace_words(K) = K / 4 dwords at trace + goff[group] + (t' G + gl) K / 4: step-major,
// a group's lanes side by side, rows 0 .. cb only, so a pair takes (cb + G) G K / 4 dwords rounded up to four -- goff is a multiple
// of four dwords and (t' G + gl) K / 4 a multiple of K / 4, so the dword store of K = 4 is 4-byte aligned, the dwordx2 of K = 8
// 8-byte aligned and the dwordx4 stores of K = 16 (one) and K = 32 (two) 16-byte aligned.  The largest pair, 65 535 rows in 64
// lanes of K = 32, takes (65 535 + 64) x 64 x 8 dwords = 134 MB; no pair is refused for its size.  The byte joins its dword at
// once and the cell chain passes through the same empty statement, as in the plain traced build.
//
// The walk (agx_sw_band_walk.inc with AT and DUAL).  States H, E1, F1, E2, F2; cell (i', j') of the span stands at
// slot = j' - i' - dlo', lane slot / K, byte k = slot % K of dword ((i' + lane) G + lane) K / 4 + k / 4.
//   H:   source 0 emits '=' or 'X' and moves diagonally; source 1 or 2 enters the gap state of that direction and of the piece bit 2
//        names, at the same cell.
//   Ep:  emits D, stays in Ep iff the cell's "Ep extended" bit is set, else returns to H; moves up.   Fp: I, its own bit, left.
// Guards, failure marker, emit and the right-aligned slots are the plain walk's; sw_gather packs the runs.
//
// What the three arguments of the plain traced build (agx_sw_band_kernel.inc, TRACE) become with five sources.
//   No wrap.  The traced build computes the very values of the untraced DUAL build (the trace reads them and feeds nothing back), so
//       "No wrap" of agx_sw_band_dual_kernel.hip holds word for word: every true value lies within [-1.32e8, 7.9e5] plus at most
//       two gap costs and one |dgf| <= 2000, a value derived from minus infinity within [-2^30 - 2.06e6, -2^30 + 2.7e4], a true
//       value always beats a derived one, and nothing comes near -2^31.  The comparisons of the extended bits set values the fill
//       computes anyway (ev, f, ev2, f2) against a neighbour's stored z and z + dgf, which the fill forms too: no new value.
//   Masked garbage.  Only H is masked.  E2 and F2 of a cell that does not exist stay as computed, like E1 and F1, and have the
//       readers E1 and F1 have: the cell below (E2) and the cell to the right (F2).  The argument of agx_sw_band_dual_kernel.hip
//       ("only H is masked") shows that they are then read by masked cells, or derive from minus infinity.  Under PH the bytes
//       outside the span are other symbols of the pair; a symbol is used once, in the diagonal move of its own cell, and such a
//       cell is masked or has a masked diagonal input (agx_sw_band_diag_trace_kernel.hip, "Stray bytes"): every value of the fill
//       is what a span packed by itself gives.  The BYTES of masked cells hold whatever their comparisons of derived values give.
//   No bit of a masked or boundary cell steers the walk.  The walk starts at the corner in state H, tests 1 <= i' <= cb,
//       1 <= j' <= ca and the band before every load, and ends at row 0 or column 0 without loading: it reads bytes of cells that
//       exist only.  Every such cell has the true cell (i' - 1, j' - 1) on its own diagonal, so the raw diagonal move s is true
//       and max(s, E1, E2, F1, F2) is true; a true value beats a derived one, so bits 0-2 name s or a gap state whose value is
//       TRUE (the maximum of a set that holds a true value is attained by a true one, and within the chosen direction the piece
//       bit names the larger value, true again).  The walk therefore stands in state Ep (Fp) only at cells whose Ep (Fp) is true:
//       it entered there by a true source, or came from the cell below (right) through a set "extended" bit.  At such a cell
//       Ep = max(uz + gf_p, ue_p + ge_p) is true, so the larger term is true, and the strict bit is set only if the extension is
//       the larger one: the walk then moves to a cell whose Ep is true.  A strict bit computed from two derived values belongs to
//       a cell whose Ep is derived, where the walk never stands in that state.  Along the edges, for p = 1 and 2 alike:
//         the band's right edge (d = dhi'): "up" is diagonal dhi' + 1, a masked slot or the last lane's minus infinity; uz, ue1 and
//             ue2 are derived, so E1 and E2 are derived, H does not choose them and nothing below extends from them.
//         the band's left edge (d = dlo'): "left" is the first lane's minus infinity for z, f AND f2; F1 and F2 are derived.
//         row 1 reads row 0 as "up": H(0, j') is true for j' <= dhi', E1(0, j') and E2(0, j') derive from the masked rows above, so
//             bits 4 and 6 are clear (derived + ge_p > true + gf_p is false) and the walk reaches row 0 in state H.  Column 1
//             reads column 0 as "left": F1(i', 0) and F2(i', 0) are maxima of minus infinities, bits 5 and 7 are clear, and the
//             walk reaches column 0 in state H.  The run along the boundary is the literal gap of its length: H(0, j') =
//             max(F1, F2) = max(gap_open + j' ge, gap_open2 + j' ge2).
//
// Merged runs.  The walk may leave a piece-1 stretch for H and enter a piece-2 stretch of the same direction at once: one run of
// the CIGAR.  include/agx.h has the argument why the CIGAR still rescores to the score under the literal cost.
#include "agx_sw_band_kernel.inc"

template <int K>
__global__ void __launch_bounds__(256) sw_fill_band_trace_dual(const SwParams prm, const SwDualGap dg, const uint32_t *__restrict__ img,
                                                               const SwBandGroup *__restrict__ groups, const SwWave *__restrict__ waves,
                                                               uint32_t n_waves, int32_t *__restrict__ scores, uint32_t *__restrict__ trace,
                                                               const uint64_t *__restrict__ goff)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.trace = trace, io.goff = goff, io.ge2 = dg.ge2, io.dgf = dg.dgf;
    band_body<K, kBandTrace | kBandPh | kBandDual>(prm, img, groups, waves[wave], io);
}

__global__ void __launch_bounds__(64) sw_walk_band_dual(const SwWalkRec *__restrict__ recs, const SwBandWalkRec *__restrict__ band, uint32_t n,
                                                        const uint32_t *__restrict__ img, const uint32_t *__restrict__ trace,
                                                        uint32_t *__restrict__ slots, uint32_t *__restrict__ runs)
{
    constexpr bool AT = true;
    constexpr bool DUAL = true;
#include "agx_sw_band_walk.inc"
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_trace_dual<KK>},
static constexpr decltype(&sw_fill_band_trace_dual<4>) kFills[kSwNumBandClasses][1] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW

int agx_sw_band_trace_dual_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    const int modes[] = {mode}; // one build per class, whatever the mode
    return band_launch_fill(kFills, modes, K, mode, a.n_waves, s, a.prm, a.dual_gap, a.img, a.groups, a.waves, a.n_waves, a.scores, a.trace, a.goff);
}

int agx_sw_band_walk_dual_launch(const SwBandWalkArgs &a, hipStream_t s) { return band_launch_walk(sw_walk_band_dual, a, s); }

void agx_sw_band_trace_dual_preload() { band_preload({(const void *)&sw_fill_band_trace_dual<8>, (const void *)&sw_walk_band_dual}); }
