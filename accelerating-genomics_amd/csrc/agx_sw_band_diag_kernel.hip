// The banded fills of agx_sw_batch_create_align_band_diag (include/agx.h, "Banded alignment around a diagonal")
// that the plain banded builds cannot serve: LOCAL (zero floor, ANY capture), FIT (H = 0 down column 0, column capture) and
// EXTEND_QUERY (pinned start, column capture).  The body is agx_sw_band_kernel.inc built with AT = the mode; its head says how
// the fill works.  GLOBAL and EXTEND around a diagonal have the boundaries and captures of sw_fill_band and run those builds.
// One build per K = diagonals per lane (AGX_SW_FOR_EACH_BAND_CLASS) and mode.
//
// What the builds add to the cell and the step (everything else, the band's position included, comes from the group record:
// the body never assumed that the band is centred on the main diagonal, only that diagonal 0 has a slot where it injects):
//   LOCAL         max(.., 0) before gf is added: one v_max per cell.  Masked cells stay minus infinity (the mask is applied
//                 after the floor).  No injection: the diagonal input of a cell of row 0 or column 0 is minus infinity, the floor
//                 makes its H = 0.  E down column 0 and F along row 0 are then gaps opened from a zero cell; they are <= 0 and
//                 the floor hides them in the cells they reach.
//   FIT           cell (i, 0) stands in slot -(i + d0) of the lane that owns diagonal -i.  While that slot exists (rows 0 .. lb)
//                 its diagonal input is set to minus the mismatch score before the cell is computed, as the plain build does
//                 once for (0, 0): the padding symbol of column 0 matches nothing, so the diagonal move gives exactly 0;
//                 F(i, 0) is a maximum of the masked cells on its left, minus infinity; E(i, 0) = a gap opened from H(i - 1, 0)
//                 = 0 is <= 0 and stays in column 0.  Row 0 right of (0, 0) comes out of the recurrence as in the pinned builds.
//                 The other way -- a second one-hot mask word that substitutes gf after the cell -- compiles to a compare and a
//                 select in every cell of every step (13 instructions a cell against 11; DESIGN.md 4.1i has both disassemblies);
//                 this one costs a compare and an exec-masked block of 2 K instructions that only the steps execute in which
//                 some lane of the wave holds column 0: 2w + 1 rows of a pair.
//   column la     (FIT, EXTEND_QUERY) cell (i, la) stands in slot la - i - d0; read for rows 0 .. lb under the same kind of
//                 exec-masked block (2 K instructions, executed in the 2w + 1 rows in which column la is inside the band), kept
//                 on a strict improvement of a maximum that starts at minus infinity, reduced over the group by (score, row).
// No wrap: the floor and the free start add nothing to minus infinity -- the floor replaces a derived minus infinity by 0 only in
// cells that exist, where 0 is the true value, and masked cells are set back to exactly minus infinity after it -- and true
// values only get closer to 0: a LOCAL H lies in [0, 12 * 65535], a FIT H is at least the pinned one.  The bounds of the head of
// agx_sw_band_kernel.inc hold as they stand.
#include "agx_sw_band_kernel.inc"

template <int K, int MODE>
__global__ void __launch_bounds__(256) sw_fill_band_at(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                       const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                       uint32_t *__restrict__ pos)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos;
    band_body<K, band_ext(MODE == AGX_SW_MODE_LOCAL), MODE>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_at<KK, AGX_SW_MODE_LOCAL>, sw_fill_band_at<KK, AGX_SW_MODE_FIT>, sw_fill_band_at<KK, AGX_SW_MODE_EXTEND_QUERY>},
static constexpr decltype(&sw_fill_band_at<4, AGX_SW_MODE_LOCAL>) kFills[kSwNumBandClasses][3] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModes[] = {AGX_SW_MODE_LOCAL, AGX_SW_MODE_FIT, AGX_SW_MODE_EXTEND_QUERY};

int agx_sw_band_at_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    return band_launch_fill(kFills, kModes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos);
}

void agx_sw_band_at_preload() { band_preload({(const void *)&sw_fill_band_at<8, AGX_SW_MODE_FIT>}); }
