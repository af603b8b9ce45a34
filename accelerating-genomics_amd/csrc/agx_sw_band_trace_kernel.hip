// The TRACED banded fill and the walk over its directions (agx_sw_batch_create_align_band_cigar; include/agx.h, "CIGARs for
// banded batches").  The fill is agx_sw_band_kernel.inc with TRACE, corner capture, one build per K = diagonals
// per lane; the head of that file says what a nibble holds and why no bit of a masked or boundary cell can steer the walk.
//
// The walk is the state machine of agx_sw_walk_kernel.hip on a trace laid out by diagonals: one lane per pair, from the corner
// (cb, ca) in state H; cell (i, j) is nibble slot % K of lane slot / K at step i + lane, slot = j - i - dlo.  Before every load
// it tests dlo <= j - i <= dhi, i <= cb and j <= ca, so slot < G K and step < cb + G: no word of the block, whatever it holds,
// can lead a load out of the pair's own directions.  A path that leaves the band (or a boundary run outside it) stores
// kSwWalkFailed in runs[pair].  Runs land right-aligned in the pair's slot of ca + cb words; sw_gather packs them.  Its body
// stands in agx_sw_band_walk.inc, which the walk of spans that begin inside the image shares.
#include "agx_sw_band_kernel.inc"

template <int K>
__global__ void __launch_bounds__(256) sw_fill_band_trace(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                          const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                          uint32_t *__restrict__ trace, const uint64_t *__restrict__ goff)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.trace = trace, io.goff = goff;
    band_body<K, kBandTrace>(prm, img, groups, waves[wave], io);
}

__global__ void __launch_bounds__(64) sw_walk_band(const SwWalkRec *__restrict__ recs, const SwBandWalkRec *__restrict__ band, uint32_t n,
                                                   const uint32_t *__restrict__ img, const uint32_t *__restrict__ trace,
                                                   uint32_t *__restrict__ slots, uint32_t *__restrict__ runs)
{
    constexpr bool AT = false;
    constexpr bool DUAL = false;
#include "agx_sw_band_walk.inc"
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_trace<KK>},
static constexpr decltype(&sw_fill_band_trace<4>) kFills[kSwNumBandClasses][1] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW

int agx_sw_band_trace_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    const int modes[] = {mode}; // one build per class, whatever the mode
    return band_launch_fill(kFills, modes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.trace, a.goff);
}

int agx_sw_band_walk_launch(const SwBandWalkArgs &a, hipStream_t s) { return band_launch_walk(sw_walk_band, a, s); }

void agx_sw_band_trace_preload() { band_preload({(const void *)&sw_fill_band_trace<8>, (const void *)&sw_walk_band}); }
