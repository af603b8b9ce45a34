// The biased packed Smith-Waterman fill (agx_sw_pk2_kernel.inc): its kernels with the plain cell (KC = 0), the rising cell
// (KC = 1) and the rising cell with column classes of period four (KC = 4).  The column classes of period C / 2 are built in
// agx_sw_pk2w_kernel.hip.
#include "agx_sw_pk2_kernel.inc"

#include <hip/hip_ext.h>

namespace {

template <int C, int KC>
__global__ void __launch_bounds__(256) sw_fill_pk2(const SwParams prm, const uint32_t *__restrict__ img,
                                                   const SwGroup2 *__restrict__ groups,
                                                   const SwWave *__restrict__ waves, uint32_t n_waves,
                                                   int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    pk2_body<C, KC>(prm, img, groups, waves[wave], scores);
}

// The column classes of period four (KC = 4) with the staged wave priority (SwParams::stage; agx_sw_pk2_kernel.inc, "Staged
// priority"): kernels of their own, so that the unstaged ones stay what they are.  The host stages no other cell.
template <int C>
__global__ void __launch_bounds__(256) sw_fill_pk2_staged(const SwParams prm, const uint32_t *__restrict__ img,
                                                          const SwGroup2 *__restrict__ groups,
                                                          const SwWave *__restrict__ waves, uint32_t n_waves,
                                                          int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    pk2_body<C, 4, false, true>(prm, img, groups, waves[wave], scores);
}

__global__ void __launch_bounds__(256) sw_fill_pk2_any_staged(const SwParams prm, const uint32_t *__restrict__ img,
                                                              const SwGroup2 *__restrict__ groups,
                                                              const SwWave *__restrict__ waves, uint32_t n_waves,
                                                              int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    const SwWave w = waves[wave];
    switch (__builtin_amdgcn_readfirstlane(w.reserved) & 0xffffu) { // columns per lane of this wave
#define AGX_SW_CASE(CC) \
    case CC: pk2_body<CC, 4, false, true>(prm, img, groups, w, scores); break;
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: break;
    }
}

// Mixed batches: ONE launch for every lane-tiling class.  Each wavefront reads its class (columns per lane)
// from its record and runs that class's fill; the kernel is allocated the registers of the widest class
// (214 VGPRs as its code object states them -- tools/kernel_resources.py --, two waves per SIMD: the fill is bound by
// VALU issue, not by occupancy).  Against one launch
// per class this (a) lets the planner use every width, so padding shrinks, (b) dispatches the waves of ALL
// classes longest first, (c) has no stream fork/join and no per-launch ramp.
template <int KC>
__global__ void __launch_bounds__(256) sw_fill_pk2_any(const SwParams prm, const uint32_t *__restrict__ img,
                                                       const SwGroup2 *__restrict__ groups,
                                                       const SwWave *__restrict__ waves, uint32_t n_waves,
                                                       int32_t *__restrict__ scores)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    const SwWave w = waves[wave];
    switch (__builtin_amdgcn_readfirstlane(w.reserved) & 0xffffu) { // columns per lane of this wave
#define AGX_SW_CASE(CC) \
    case CC: pk2_body<CC, KC>(prm, img, groups, w, scores); break;
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: break;
    }
}

template <int C, int KC>
int launch(const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves, uint32_t n_waves,
           int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    const uint32_t blocks = (n_waves + 3) / 4;
    if (KC == 4 && prm.stage)
        AGX_SW_PK2_LAUNCH((sw_fill_pk2_staged<C>), blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    else
        AGX_SW_PK2_LAUNCH((sw_fill_pk2<C, KC>), blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace

int agx_sw_pk2_launch_any(int rising, bool wide, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves,
                          uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    if (n_waves == 0) return 0;
    if (rising == 4 && wide) return agx_sw_pk2w_launch_any(prm, img, groups, waves, n_waves, scores, s, stop);
    const uint32_t blocks = (n_waves + 3) / 4;
    if (rising == 4 && prm.stage)
        AGX_SW_PK2_LAUNCH(sw_fill_pk2_any_staged, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    else if (rising == 4)
        AGX_SW_PK2_LAUNCH(sw_fill_pk2_any<4>, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    else if (rising)
        AGX_SW_PK2_LAUNCH(sw_fill_pk2_any<1>, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    else
        AGX_SW_PK2_LAUNCH(sw_fill_pk2_any<0>, blocks, s, stop, prm, img, groups, waves, n_waves, scores);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int agx_sw_pk2_launch_class(int cols_per_lane, int rising, bool wide, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups,
                            const SwWave *waves, uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop)
{
    if (n_waves == 0) return 0;
    // (a class without a wide build -- sw_pk2_period -- runs the period of four: the host's rule then holds all the more)
    if (rising == 4 && wide && sw_pk2_period(cols_per_lane) > 4)
        return agx_sw_pk2w_launch_class(cols_per_lane, prm, img, groups, waves, n_waves, scores, s, stop);
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC) \
    case CC: return rising == 4 ? launch<CC, 4>(prm, img, groups, waves, n_waves, scores, s, stop) : rising ? launch<CC, 1>(prm, img, groups, waves, n_waves, scores, s, stop) : launch<CC, 0>(prm, img, groups, waves, n_waves, scores, s, stop);
        AGX_SW_FOR_EACH_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

// Loads this file's code object now: the first launch of a kernel otherwise pays for it (1-2 ms in a fresh process --
// inside hipvers' launch -> scores window).  Called when a batch that will use these kernels is created.
void agx_sw_pk2_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_pk2_any<4>));
}
