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
    BandIo io;
    io.scores = scores, io.pos = pos, io.sub = sub;
    if constexpr (MODE == AGX_SW_MODE_GLOBAL || MODE == AGX_SW_MODE_EXTEND)
        band_body<K, band_ext(MODE == AGX_SW_MODE_EXTEND) | kBandMat>(prm, img, groups, waves[wave], io);
    else
        band_body<K, band_ext(MODE == AGX_SW_MODE_LOCAL) | kBandMat, MODE>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_mat<KK, AGX_SW_MODE_LOCAL>, sw_fill_band_mat<KK, AGX_SW_MODE_GLOBAL>, sw_fill_band_mat<KK, AGX_SW_MODE_FIT>, sw_fill_band_mat<KK, AGX_SW_MODE_EXTEND>, sw_fill_band_mat<KK, AGX_SW_MODE_EXTEND_QUERY>},
static constexpr decltype(&sw_fill_band_mat<4, AGX_SW_MODE_LOCAL>) kFills[kSwNumBandClasses][5] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModes[] = {AGX_SW_MODE_LOCAL, AGX_SW_MODE_GLOBAL, AGX_SW_MODE_FIT, AGX_SW_MODE_EXTEND, AGX_SW_MODE_EXTEND_QUERY};

int agx_sw_band_mat_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    return band_launch_fill(kFills, kModes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos, a.table);
}

void agx_sw_band_mat_preload() { band_preload({(const void *)&sw_fill_band_mat<8, AGX_SW_MODE_FIT>}); }
