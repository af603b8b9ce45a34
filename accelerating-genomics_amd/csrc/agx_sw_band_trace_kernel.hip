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
    band_body<K, false, true>(prm, img, groups, waves[wave], scores, nullptr, trace, goff);
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

int agx_sw_band_trace_launch_class(int diags_per_lane, const SwParams &prm, const uint32_t *img, const SwBandGroup *groups, const SwWave *waves,
                                   uint32_t n_waves, int32_t *scores, uint32_t *trace, const uint64_t *goff, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (diags_per_lane) {
#define AGX_SW_CASE(KK)                                                                                                                    \
    case KK:                                                                                                                               \
        hipLaunchKernelGGL((sw_fill_band_trace<KK>), dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, trace, goff); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

int agx_sw_band_walk_launch(const SwWalkRec *recs, const SwBandWalkRec *band, uint32_t n, const uint32_t *img, const uint32_t *trace,
                            uint32_t *slots, uint32_t *runs, hipStream_t s)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(sw_walk_band, dim3((n + 63u) / 64u), dim3(64), 0, s, recs, band, n, img, trace, slots, runs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void agx_sw_band_trace_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_band_trace<8>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_walk_band));
}
