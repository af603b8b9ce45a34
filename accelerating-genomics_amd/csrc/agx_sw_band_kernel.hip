// The banded fill of agx_sw_batch_create_align_band (modes GLOBAL and EXTEND): the body is agx_sw_band_kernel.inc, which also says
// how it works.  One build per K = diagonals per lane (AGX_SW_FOR_EACH_BAND_CLASS) and capture.
#include "agx_sw_band_kernel.inc"

template <int K, bool EXT>
__global__ void __launch_bounds__(256) sw_fill_band(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                    const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                    uint32_t *__restrict__ pos)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    band_body<K, EXT>(prm, img, groups, waves[wave], scores, pos);
}

} // namespace

// extend: 0 = GLOBAL (scores[out] = D[lb][la]), 1 = EXTEND (scores[out] = the maximum, pos[out] = i << 16 | j of its first cell)
int agx_sw_band_launch_class(int diags_per_lane, int extend, const SwParams &prm, const uint32_t *img, const SwBandGroup *groups,
                             const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *pos, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (diags_per_lane) {
#define AGX_SW_CASE(KK)                                                                                                               \
    case KK:                                                                                                                          \
        if (extend)                                                                                                                   \
            hipLaunchKernelGGL((sw_fill_band<KK, true>), dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, pos);  \
        else                                                                                                                          \
            hipLaunchKernelGGL((sw_fill_band<KK, false>), dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, pos); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_band_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_band<8, false>));
}
