// Match/mismatch build of the locating fill (agx_sw_batch_create_align, mode LOCAL): the body is agx_sw_loc_kernel.inc,
// which also says how it works; the substitution-matrix build is agx_sw_loc_mat_kernel.hip.
#include "agx_sw_loc_kernel.inc"

template <int C>
__global__ void __launch_bounds__(256) sw_fill_loc(const SwParams prm, const uint32_t *__restrict__ img, const SwGroup *__restrict__ groups,
                                                   const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                   uint32_t *__restrict__ ends)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    loc_body<C, false>(prm, img, groups, waves[wave], scores, ends, nullptr);
}

} // namespace

int agx_sw_loc_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                            uint32_t n_waves, int32_t *scores, uint32_t *ends, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC)                                                                                                    \
    case CC:                                                                                                               \
        hipLaunchKernelGGL(sw_fill_loc<CC>, dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, ends); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_loc_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_loc<38>));
}
