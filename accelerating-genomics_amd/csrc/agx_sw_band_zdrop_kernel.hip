// The banded EXTEND fill with z-drop termination, behind agx_sw_batch_create_align_band_zdrop (include/agx.h, "Z-drop for banded
// extension").  The body is agx_sw_band_kernel.inc built with ZD; its head says how the fill works.  One build per
// K = diagonals per lane (AGX_SW_FOR_EACH_BAND_CLASS).
//
// The rule is sequential in rows: with R(i) the maximum of row i over its in-band cells and c(i) its leftmost column, the running
// best B (cell (bi, bj), starting as D[0][0] = 0 at (0, 0)) takes R(i) on a strict improvement; otherwise the extension
// terminates at row i if B - R(i) > zdrop + |ge| |(i - bi) - (c(i) - bj)|.  In the fill the lanes own diagonals and lane gl is gl
// rows behind the group's first lane, so no step holds a whole row.  What the build adds:
//   the carrier   (row maximum as z, its leftmost column) of the row a lane has just filled, over the lanes up to that lane.  It
//                 moves one lane per step with the wave_shr:1 exchange that carries z_last: lane gl - 1 finished row i one step
//                 before lane gl does.  A group's first lane starts it at minus infinity, so nothing crosses a group border, and a
//                 lane puts its own maximum in only on a strict improvement: the lower lanes hold the smaller columns.  Masked
//                 cells are exactly minus infinity and never win.  K compares and selects per step find the column.
//   the decision  the group's last lane receives R(i), c(i) of rows 0, 1, 2, .. complete and in order.  It keeps B, bi, bj and
//                 applies the rule for 1 <= i <= lb only -- the host gives the fill the rows 0 .. last = min(lb, la - dlo), so its
//                 lb IS the last row with an in-band cell, and every such row has one -- and freezes them once it terminates.
//                 All lanes run the same instructions on what they hold; only the last lane's outcome is read.  It writes
//                 score, position word (i << 16 | j, 0xffffffff for a score of 0) and stop (i - 1 of the terminating row, else
//                 -1) with ordinary stores.  The running best visits the rows in order and takes strict improvements from a
//                 leftmost column: without a termination it is the hit of the plain EXTEND build (score, then row, then column).
//   leaving       once per four steps, where the loaders turn over, the wave leaves the loop if no group's last lane still has a
//                 row to decide: it has terminated, or its row t - gl is beyond lb.  A terminated group steps on while a
//                 wave-mate runs; its B, bi, bj and stop are guarded by the stop itself and do not change, and its values reach
//                 no other group (the `first` / `last` substitutions cut z, f, e, the symbols and the carrier alike).
// No wrap.  B and R(i) are z values of true cells (every row 0 .. last has an in-band cell, and by the head of
// agx_sw_band_kernel.inc a true H lies in [-1.311e8, 7.9e5], z adds one gap cost), so B - R(i) <= 7.9e5 + 1.32e8.  The right side
// is at most AGX_SW_ZDROP_MAX + 1000 * (65535 + 65535) = 1e9 + 1.32e8 < 2^31.  Hence zdrop = AGX_SW_ZDROP_MAX never fires.  In
// the lanes whose outcome is not read the carrier may still be minus infinity: B - (-2^30) < 1.08e9 does not wrap either.
#include "agx_sw_band_kernel.inc"

template <int K>
__global__ void __launch_bounds__(256) sw_fill_band_zd(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                       const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                       uint32_t *__restrict__ pos, int32_t zdrop, int32_t *__restrict__ stops)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos, io.zdrop = zdrop, io.stops = stops;
    band_body<K, kBandExt | kBandZd>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_zd<KK>},
static constexpr decltype(&sw_fill_band_zd<4>) kFills[kSwNumBandClasses][1] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW

int agx_sw_band_zdrop_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    const int modes[] = {mode}; // one build per class, whatever the mode
    return band_launch_fill(kFills, modes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos, a.zdrop, a.stops);
}

void agx_sw_band_zdrop_preload() { band_preload({(const void *)&sw_fill_band_zd<8>}); }
