// The banded fills of agx_sw_batch_create_align_band_diag_matrix (include/agx.h, "Banded alignment around a diagonal under a
// substitution matrix"): all five modes of a band around a caller-given diagonal with the diagonal move read from
// a substitution matrix.  The body is agx_sw_band_kernel.inc built with MAT; its head says how the fill works and what the matrix
// changes (symbols, injection, the table in LDS, the lookup schedule, "No wrap").  GLOBAL and EXTEND are the plain builds with
// MAT, LOCAL, FIT and EXTEND_QUERY the AT builds with MAT.  One build per K = diagonals per lane and mode.  A translation unit of
// its own, so the match/mismatch code objects are the ones they were.
//
// The table: kSwMatDim x kSwMatDim int16 entries score - gf (2178 bytes), one copy per workgroup.  EVERY wave of the workgroup
// copies its share and passes the barrier before a surplus wave of the last workgroup returns: returning first, it would leave
// its quarter of the entries uncopied and the other waves at a barrier that it never reaches.
#include "agx_sw_band_kernel.inc"

template <int K, int MODE>
__global__ void __launch_bounds__(256) sw_fill_band_mat(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                        const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                        uint32_t *__restrict__ pos, const int16_t *__restrict__ table)
{
    __shared__ int16_t sub[kSwMatDim * kSwMatDim];
    for (int k = threadIdx.x; k < kSwMatDim * kSwMatDim; k += 256) sub[k] = table[k];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    if constexpr (MODE == AGX_SW_MODE_GLOBAL || MODE == AGX_SW_MODE_EXTEND)
        band_body<K, MODE == AGX_SW_MODE_EXTEND, false, -1, false, false, true>(prm, img, groups, waves[wave], scores, pos, nullptr, nullptr, 0, nullptr, sub);
    else
        band_body<K, MODE == AGX_SW_MODE_LOCAL, false, MODE, false, false, true>(prm, img, groups, waves[wave], scores, pos, nullptr, nullptr, 0, nullptr, sub);
}

} // namespace

// scores[out] and pos[out] as agx_sw_band_launch_class (GLOBAL, EXTEND) and agx_sw_band_at_launch_class (LOCAL, FIT, EXTEND_QUERY)
// write them; table: the device copy of the batch's kSwMatDim x kSwMatDim entries
int agx_sw_band_mat_launch_class(int diags_per_lane, int mode, const SwParams &prm, const uint32_t *img, const SwBandGroup *groups,
                                 const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *pos, const int16_t *table, hipStream_t s)
{
    if (n_waves == 0) return 0;
    const uint32_t blocks = (n_waves + 3) / 4;
#define AGX_SW_MAT(KK, MM) \
    hipLaunchKernelGGL((sw_fill_band_mat<KK, MM>), dim3(blocks), dim3(256), 0, s, prm, img, groups, waves, n_waves, scores, pos, table)
    switch (diags_per_lane) {
#define AGX_SW_CASE(KK)                                                                      \
    case KK:                                                                                 \
        if (mode == AGX_SW_MODE_LOCAL) AGX_SW_MAT(KK, AGX_SW_MODE_LOCAL);                    \
        else if (mode == AGX_SW_MODE_GLOBAL) AGX_SW_MAT(KK, AGX_SW_MODE_GLOBAL);             \
        else if (mode == AGX_SW_MODE_FIT) AGX_SW_MAT(KK, AGX_SW_MODE_FIT);                   \
        else if (mode == AGX_SW_MODE_EXTEND) AGX_SW_MAT(KK, AGX_SW_MODE_EXTEND);             \
        else if (mode == AGX_SW_MODE_EXTEND_QUERY) AGX_SW_MAT(KK, AGX_SW_MODE_EXTEND_QUERY); \
        else return -2;                                                                      \
        return hipGetLastError() == hipSuccess ? 0 : -1;
        AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_CASE)
#undef AGX_SW_CASE
    default: return -2;
    }
#undef AGX_SW_MAT
}

void agx_sw_band_mat_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_fill_band_mat<8, AGX_SW_MODE_FIT>));
}
