// Substitution-matrix build of the anchored fill WITH alignment statistics (agx_sw_batch_create_align_stats: the fill of the modes
// GLOBAL / EXTEND / EXTEND_QUERY, and FIT's begin pass): the body of agx_sw_anch_kernel.inc with its STATS
// flag and its MAT flag, the table in LDS -- every state a (score, matches << 12 | pairs) tuple.  A translation unit of its own, so the plain builds' code
// objects are the ones they were.
#include "agx_sw_anch_kernel.inc"

template <int C, bool COL>
__global__ void __launch_bounds__(256) sw_fill_anch_mat_stats(const SwParams prm, const int flags, const uint32_t *__restrict__ img,
                                                              const SwGroup *__restrict__ groups, const SwWave *__restrict__ waves, uint32_t n_waves,
                                                              int32_t *__restrict__ scores, uint32_t *__restrict__ ends, uint32_t *__restrict__ lstat, const int16_t *__restrict__ table)
{
    __shared__ int16_t sub[kSwMatDim * kSwMatDim];
    for (int k = threadIdx.x; k < kSwMatDim * kSwMatDim; k += 256) sub[k] = table[k];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    anch_body<C, COL, true, true>(prm, flags, img, groups, waves[wave], scores, ends, sub, lstat);
}

} // namespace

// capture: 0 = ANY (EXTEND), 1 = COL; flags: 1 = free target start, 2 = report the corner (GLOBAL)
int agx_sw_anch_mat_stats_launch_class(int cols_per_lane, int capture, int flags, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                                   const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat, const int16_t *table, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC)                                                                                                                                                \
    case CC:                                                                                                                                                           \
        if (capture)                                                                                                                                                   \
            hipLaunchKernelGGL((sw_fill_anch_mat_stats<CC, true>), dim3(blocks), dim3(256), 0, s, prm, flags, img, groups, waves, n_waves, scores, ends, lstat, table);  \
        else                                                                                                                                                           \
            hipLaunchKernelGGL((sw_fill_anch_mat_stats<CC, false>), dim3(blocks), dim3(256), 0, s, prm, flags, img, groups, waves, n_waves, scores, ends, lstat, table); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_STATS_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_anch_mat_stats_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_anch_mat_stats<kSwStatsTopClass, true>));
}
