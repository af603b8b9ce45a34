// The banded fills UNDER TWO-PIECE AFFINE GAP COSTS (include/agx.h, "Banded alignment around a diagonal under two-piece gap
// costs"): a gap of L >= 1 symbols scores max(gap_open + L gap_extend, gap_open2 + L gap_extend2).  The body is
// agx_sw_band_kernel.inc built with DUAL, whose head says how the fill works.  Five builds per K = diagonals per lane
// (AGX_SW_FOR_EACH_BAND_CLASS): the pinned fills sw_fill_band_dual<K, false> (GLOBAL: the corner) and <K, true> (EXTEND), and the
// fills around a diagonal sw_fill_band_dual_at<K, LOCAL>, <K, FIT> and <K, EXTEND_QUERY>.  GLOBAL and EXTEND have builds of their
// own here, unlike under a matrix: the cell itself changes.  The traced build (TRACE and PH with DUAL) is
// agx_sw_band_dual_trace_kernel.hip; there is no ZD, MAT or STATS build.
//
// The cell.  Over the in-band cells
//     E1(i, j) = max(H(i - 1, j) + gf,  E1(i - 1, j) + ge)      gf  = gap_open  + gap_extend,  ge  = gap_extend
//     E2(i, j) = max(H(i - 1, j) + gf2, E2(i - 1, j) + ge2)     gf2 = gap_open2 + gap_extend2, ge2 = gap_extend2
//     F1, F2 likewise from (i, j - 1);   H = max(diagonal move, E1, F1, E2, F2)   (LOCAL: and 0)
// which is the gap cost above: a gap that stays in one piece's states from its first symbol to its last costs that piece, H takes
// the better one, and a gap that changed pieces halfway would cost at least one more open -- so it never beats both.
// One stored form: z = H + gf, as in every other build.  Piece 2 reads it as z + dgf, dgf = gf2 - gf (-2000 .. 2000), one add in
// front of the maximum; storing a second z would cost a register per diagonal and a second masked value per cell.  Per cell the
// build adds, to the plain one: uz + dgf, ue2 + ge2 and their maximum (E2), zleft + dgf, f2 + ge2 and their maximum (F2), and one
// three-way maximum into H -- the K = 8 and K = 32 disassemblies show exactly those (four v_add, two v_max, one v_max3 a cell).
// SwParams is the plain builds': ge2 and dgf travel beside it in a struct of their own (SwDualGap), so no other kernel's argument
// block changes.
//
// State and hand-overs.  Per diagonal z, e and e2 (3 K words a lane); along the chain f and f2.  Between lanes, each step:
//   to the right (wave_shr:1)   z_last, f_last AND f2_last of the lane's last cell: the left input of the next lane's first
//                               cell.  A group's first lane substitutes minus infinity for all three.
//   to the left (wave_shl:1)    z[0], e[0] AND e2[0] of the first cell (phase 1): the up input of the left neighbour's last
//                               diagonal (phase 2).  A group's last lane substitutes minus infinity for all three.
// A horizontal gap that runs across a lane boundary while piece 2 is the better one lives in f2 alone -- f holds the worse piece-1
// cost, z of the cells it passes may come from elsewhere -- so a build that left f2_last behind would restart the gap at the
// boundary with a new open; the vertical case is e2 and the left hand-over.  tests/test_sw_band_dual_gpu.py plants such gaps.
//
// Boundaries.  As in the plain builds, from the recurrence itself: H(0, 0) = 0 is injected as a diagonal input, row 0 to its right
// is then max(F1, F2) = max(gap_open + j ge, gap_open2 + j ge2), the two-piece cost of a gap of j, and likewise down column 0 by
// E1 and E2.  FIT's column 0 and LOCAL's floor are untouched; gaps opened from their zero cells are <= 0 under either piece.
//
// No wrap.  Minus infinity is kBandNegInf = -2^30; each of the four gap numbers lies in -1000 .. 0.
//   true values     the two-piece cost of a gap is >= its piece-1 cost, so every path scores at least what it scores under piece 1
//                   alone and every true H is bounded below by the one-piece bound at the head of agx_sw_band_kernel.inc,
//                   -1.311e8; above by 12 * 65535.  z, e, f, e2, f2 and z + dgf add at most two gap costs and |dgf| <= 2000.
//   derived values  a value derived from minus infinity gains one dgf (<= 2000) and then only extension costs (<= 0) along one
//                   row of the band (F1, F2) or one column's stretch inside it (E1, E2) before a masked H cuts the chain: at most
//                   2048 cells of at most 1000 each.  It stays within [-2^30 - 2.05e6 - 2000, -2^30 + 2000 + 2048 * 12]: above
//                   -2^31, and below every true value (-1.32e8 > -2^30 + 2.7e4).  A true value always beats a derived one.
//   only H is masked  E2 and F2 of cells that do not exist stay as computed, like E and F, and for the same reason: they have the
//                   same readers.  E2 of a row < 0, a column < 0 or > la, or a diagonal > dhi is read by the cell below it, which
//                   is masked as well or is the first real cell of its column, whose whole column above is masked H: that E2
//                   derives from minus infinity, as E does.  F2 of a masked cell is read to the right only, by cells of the same
//                   row that are masked too (j > la, d > dhi) or stand in column 0 with nothing but masked H on their left, so it
//                   is a maximum of derived values.  Rows > lb are read by rows > lb only.  Nothing about the mask changed.
//   LOCAL, FIT      the floor replaces a derived value by 0 only in cells that exist, where 0 is true; masked cells go back to
//                   exactly minus infinity after it.  The bounds of agx_sw_band_diag_kernel.hip hold as they stand.
//
// Capture and the reductions over a group read z alone and are the plain builds' code: the result and tie rules depend on scores
// only, so nothing about "which piece" enters them.
#include "agx_sw_band_kernel.inc"

template <int K, bool EXT>
__global__ void __launch_bounds__(256) sw_fill_band_dual(const SwParams prm, const SwDualGap dg, const uint32_t *__restrict__ img,
                                                         const SwBandGroup *__restrict__ groups, const SwWave *__restrict__ waves, uint32_t n_waves,
                                                         int32_t *__restrict__ scores, uint32_t *__restrict__ pos)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos, io.ge2 = dg.ge2, io.dgf = dg.dgf;
    band_body<K, band_ext(EXT) | kBandDual>(prm, img, groups, waves[wave], io);
}

template <int K, int MODE>
__global__ void __launch_bounds__(256) sw_fill_band_dual_at(const SwParams prm, const SwDualGap dg, const uint32_t *__restrict__ img,
                                                            const SwBandGroup *__restrict__ groups, const SwWave *__restrict__ waves,
                                                            uint32_t n_waves, int32_t *__restrict__ scores, uint32_t *__restrict__ pos)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos, io.ge2 = dg.ge2, io.dgf = dg.dgf;
    band_body<K, band_ext(MODE == AGX_SW_MODE_LOCAL) | kBandDual, MODE>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_dual<KK, true>, sw_fill_band_dual<KK, false>},
static constexpr decltype(&sw_fill_band_dual<4, true>) kFills[kSwNumBandClasses][2] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModes[] = {AGX_SW_MODE_EXTEND, AGX_SW_MODE_GLOBAL};
#define AGX_SW_ROW(KK) {sw_fill_band_dual_at<KK, AGX_SW_MODE_LOCAL>, sw_fill_band_dual_at<KK, AGX_SW_MODE_FIT>, sw_fill_band_dual_at<KK, AGX_SW_MODE_EXTEND_QUERY>},
static constexpr decltype(&sw_fill_band_dual_at<4, AGX_SW_MODE_LOCAL>) kFillsAt[kSwNumBandClasses][3] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModesAt[] = {AGX_SW_MODE_LOCAL, AGX_SW_MODE_FIT, AGX_SW_MODE_EXTEND_QUERY};

int agx_sw_band_dual_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    if (mode == AGX_SW_MODE_GLOBAL || mode == AGX_SW_MODE_EXTEND)
        return band_launch_fill(kFills, kModes, K, mode, a.n_waves, s, a.prm, a.dual_gap, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos);
    return band_launch_fill(kFillsAt, kModesAt, K, mode, a.n_waves, s, a.prm, a.dual_gap, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos);
}

void agx_sw_band_dual_preload() { band_preload({(const void *)&sw_fill_band_dual<8, false>}); }
