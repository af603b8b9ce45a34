// Substitution-matrix build of the TRACED anchored fill (agx_sw_batch_cigars): the body of agx_sw_anch_kernel.inc
// with its TRACE flag and its MAT flag, the table in LDS, COL capture, launched with the GLOBAL flag.  A translation unit of
// its own, so the plain builds' code objects are the ones they were.
#include "agx_sw_anch_kernel.inc"

template <int C>
__global__ void __launch_bounds__(256) sw_fill_trace_mat(const SwParams prm, const uint32_t *__restrict__ img, const SwGroup *__restrict__ groups,
                                                         const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                         uint32_t *__restrict__ ends, uint32_t *__restrict__ trace,
                                                         const uint64_t *__restrict__ goff, const int16_t *__restrict__ table)
{
    __shared__ int16_t sub[kSwMatDim * kSwMatDim];
    for (int k = threadIdx.x; k < kSwMatDim * kSwMatDim; k += 256) sub[k] = table[k];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    anch_body<C, true, true, false, true>(prm, 2, img, groups, waves[wave], scores, ends, sub, nullptr, trace, goff);
}

} // namespace

int agx_sw_trace_mat_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                  uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *trace, const uint64_t *goff, const int16_t *table,
                                  hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
    switch (cols_per_lane) {
#define AGX_SW_CASE(CC)                                                                                                                               \
    case CC:                                                                                                                                          \
        hipLaunchKernelGGL((sw_fill_trace_mat<CC>), dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, ends, trace, goff, table); \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_TRACE_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
}

void agx_sw_trace_mat_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_trace_mat<kSwTraceTopClass>));
}
