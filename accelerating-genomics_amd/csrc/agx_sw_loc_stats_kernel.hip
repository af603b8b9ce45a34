// Match/mismatch build of the locating fill WITH alignment statistics (agx_sw_batch_create_align_stats, the begin pass of mode
// LOCAL): the body of agx_sw_loc_kernel.inc with its STATS flag -- every state a (score, matches << 12 | pairs)
// tuple -- which also says how it works.  A translation unit of its own, so the plain builds' code objects are the ones they were.
#include "agx_sw_loc_kernel.inc"

template <int C>
__global__ void __launch_bounds__(256) sw_fill_loc_stats(const SwParams prm, const uint32_t *__restrict__ img, const SwGroup *__restrict__ groups,
                                                         const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                         uint32_t *__restrict__ ends, uint32_t *__restrict__ lstat)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    loc_body<C, false, true>(prm, img, groups, waves[wave], scores, ends, nullptr, lstat);
}

} // namespace

int agx_sw_loc_stats_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                  uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC)                                                                                                                        \
    case CC:                                                                                                                                   \
        hipLaunchKernelGGL(sw_fill_loc_stats<CC>, dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, ends, lstat); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_STATS_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_loc_stats_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_loc_stats<kSwStatsTopClass>));
}
