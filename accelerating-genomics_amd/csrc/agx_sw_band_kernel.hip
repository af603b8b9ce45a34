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
    BandIo io;
    io.scores = scores, io.pos = pos;
    band_body<K, band_ext(EXT)>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band<KK, true>, sw_fill_band<KK, false>},
static constexpr decltype(&sw_fill_band<4, true>) kFills[kSwNumBandClasses][2] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModes[] = {AGX_SW_MODE_EXTEND, AGX_SW_MODE_GLOBAL};

int agx_sw_band_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    return band_launch_fill(kFills, kModes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos);
}

void agx_sw_band_preload() { band_preload({(const void *)&sw_fill_band<8, false>}); }
