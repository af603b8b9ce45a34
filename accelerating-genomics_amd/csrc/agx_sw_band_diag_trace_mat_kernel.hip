// The TRACED banded fill under a substitution matrix, for spans that begin inside the resident image
// (agx_sw_batch_create_align_band_diag_matrix_cigar; include/agx.h, "Banded alignment around a diagonal under a substitution
// matrix").  The body is agx_sw_band_kernel.inc with TRACE, PH and MAT: the build of
// agx_sw_band_diag_trace_kernel.hip -- whose head has the argument for the start phase and the stray bytes -- with the diagonal
// move read from the table in LDS.  Under MAT a stray byte of a is a symbol number 1 .. 32 like any other and indexes inside the
// table; row 0 carries symbol 0, whose table row holds the padding entry in every column, so the injected diagonal input still
// gives H(0, 0) = 0 exactly next to whatever symbol a[a_begin - 1] is.  The walk is sw_walk_band_at unchanged: it compares image
// bytes, here symbol numbers, so '=' is "identical codes".  The table is loaded as in agx_sw_band_diag_mat_kernel.hip.
#include "agx_sw_band_kernel.inc"

template <int K>
__global__ void __launch_bounds__(256) sw_fill_band_trace_mat(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                              const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                              uint32_t *__restrict__ trace, const uint64_t *__restrict__ goff,
                                                              const int16_t *__restrict__ table)
{
    __shared__ int16_t sub[kSwMatDim * kSwMatDim];
    for (int k = threadIdx.x; k < kSwMatDim * kSwMatDim; k += 256) sub[k] = table[k];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.trace = trace, io.goff = goff, io.sub = sub;
    band_body<K, kBandTrace | kBandPh | kBandMat>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_trace_mat<KK>},
static constexpr decltype(&sw_fill_band_trace_mat<4>) kFills[kSwNumBandClasses][1] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW

int agx_sw_band_trace_mat_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    const int modes[] = {mode}; // one build per class, whatever the mode
    return band_launch_fill(kFills, modes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.trace, a.goff, a.table);
}

void agx_sw_band_trace_mat_preload() { band_preload({(const void *)&sw_fill_band_trace_mat<8>}); }
