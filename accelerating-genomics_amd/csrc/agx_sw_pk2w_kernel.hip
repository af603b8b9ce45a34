// The biased packed Smith-Waterman fill (agx_sw_pk2_kernel.inc) with column classes of period C / 2 ("wide"): every class
// holds exactly two of a lane's columns, a lane wraps once a step instead of at every fourth column, and the running maxima
// pair without leftovers.  Built for the classes sw_pk2_period (agx_sw.h) names; the host launches these kernels only for a
// batch whose values stay in range with the larger class offsets (agx_sw.cpp, "class period"), the period of four otherwise.
#include "agx_sw_pk2_kernel.inc"

#include <hip/hip_ext.h>

namespace {

template <int C>
__global__ void __launch_bounds__(256) sw_fill_pk2w(const SwParams prm, const uint32_t *__restrict__ img,
                                                    const SwGroup2 *__restrict__ groups,
                                                    const SwWave *__restrict__ waves, uint32_t n_waves,
                                                    int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    pk2_body<C, 4, true>(prm, img, groups, waves[wave], scores);
}

// the same with the staged wave priority (SwParams::stage; agx_sw_pk2_kernel.inc, "Staged priority"): kernels of their own, so
// that the unstaged ones stay what they are
template <int C>
__global__ void __launch_bounds__(256) sw_fill_pk2w_staged(const SwParams prm, const uint32_t *__restrict__ img,
                                                           const SwGroup2 *__restrict__ groups,
                                                           const SwWave *__restrict__ waves, uint32_t n_waves,
                                                           int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    pk2_body<C, 4, true, true>(prm, img, groups, waves[wave], scores);
}

__global__ void __launch_bounds__(256) sw_fill_pk2w_any_staged(const SwParams prm, const uint32_t *__restrict__ img,
                                                               const SwGroup2 *__restrict__ groups,
                                                               const SwWave *__restrict__ waves, uint32_t n_waves,
                                                               int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    const SwWave w = waves[wave];
    switch (__builtin_amdgcn_readfirstlane(w.reserved) & 0xffffu) { // columns per lane of this wave
#define AGX_SW_CASE(CC) \
    case CC: pk2_body<CC, 4, true, true>(prm, img, groups, w, scores); break;
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: break;
    }
}

// the one launch of a mixed batch (sw_fill_pk2_any<4>): every class at its own period
__global__ void __launch_bounds__(256) sw_fill_pk2w_any(const SwParams prm, const uint32_t *__restrict__ img,
                                                        const SwGroup2 *__restrict__ groups,
                                                        const SwWave *__restrict__ waves, uint32_t n_waves,
                                                        int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    const SwWave w = waves[wave];
    switch (__builtin_amdgcn_readfirstlane(w.reserved) & 0xffffu) { // columns per lane of this wave
#define AGX_SW_CASE(CC) \
    case CC: pk2_body<CC, 4, true>(prm, img, groups, w, scores); break;
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: break;
    }
}

template <int C>
int launch(const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves, uint32_t n_waves,
           int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    if constexpr (sw_pk2_period(C) > 4) {
        const uint32_t blocks = (n_waves + 3) / 4;
        if (prm.stage)
            AGX_SW_PK2_LAUNCH((sw_fill_pk2w_staged<C>), blocks, s, stop, prm, img, groups, waves, n_waves, scores);
        else
            AGX_SW_PK2_LAUNCH((sw_fill_pk2w<C>), blocks, s, stop, prm, img, groups, waves, n_waves, scores);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    } else
        return -2; // no wide build of this class
}

} // namespace

int agx_sw_pk2w_launch_any(const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves, uint32_t n_waves,
                           int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    if (prm.stage)
        AGX_SW_PK2_LAUNCH(sw_fill_pk2w_any_staged, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    else
        AGX_SW_PK2_LAUNCH(sw_fill_pk2w_any, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int agx_sw_pk2w_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves,
                             uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    if (n_waves == 0) return 0;
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC) \
    case CC: return launch<CC>(prm, img, groups, waves, n_waves, scores, s, stop);
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_pk2w_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_pk2w_any));
}
