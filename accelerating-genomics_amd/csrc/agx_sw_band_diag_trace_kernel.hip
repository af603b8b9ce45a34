// The TRACED banded fill and the walk for spans that begin INSIDE the resident image (agx_sw_batch_create_align_band_diag_cigar;
// include/agx.h, "CIGARs for batches banded around a diagonal").  A LOCAL or FIT span of a batch banded around a
// diagonal begins at (b_begin, a_begin), and in FIT b_begin is the read's place in its window.  The batch's image was packed for a
// fill from its row 0; agx_sw_batch_cigars uploads no symbol, so this build starts anywhere in that image.  The body is
// agx_sw_band_kernel.inc with TRACE and PH: corner capture, pinned start, one build per K = diagonals per lane.
//
// The span's record (agx_sw_band_span_record makes it on the host).  With s = b_begin - row0 the span's first row in the image,
// r = s mod 4 the START PHASE and ca x cb the span:
//   la_lb     ca | cb << 16
//   dlo, dhi  the pair's band in span coordinates: cell (i', j') of the span is (s + i', a_begin + j') of the image's matrix, so
//             j' - i' = (j - i) - a_begin + s and both limits move by s - a_begin.  The width stays: class and G are the batch's.
//             The origin and the corner are in the band because the begin and end cells of the hit are.
//   y_dw      the image's y_dw + (s - r) / 4
//   fpad      the image's fpad + a_begin: byte fpad + n of x is the span's a'[n]
//   reserved  r
// The step counter runs as t' = t - r: lane gl fills row i' = t' - gl at step t, so rows, the injection of H(0, 0), the corner
// capture and the trace are those of the plain traced build r steps later, and the wave steps max(cb + r) + G times.
//
// Why one phase re-aligns both loaders.  The feeder consumes byte t mod 4 of dword t / 4 behind y_dw at step t: byte t of the
// record's y, which is byte (s - r) + t = s + t' of the image's y, and behind the one byte in front of b that is b'[t' - 1], the
// symbol of row t' -- live for 1 <= t' <= cb only, so row 0 still carries kBandRowPad.  The column loader hands the group's last
// lane a'[q0x' + t'] at step t, q0x' = dlo' + G K - G: byte fpad' + q0x' - r + t of x, and
//   fpad' + q0x' - r = (fpad + a_begin) + (q0x - a_begin + s) - r = (fpad + q0x) + (s - r) = 0 (mod 4),
// the first because the host chose fpad so for the planned image, the second by the choice of r.  So both loaders still read one
// aligned dword per four steps, three quads ahead, and the first dword index (fpad' + q0x' - r) / 4 is exact (it may be negative,
// as in the plain build: such dwords read as 0).  The query window of step 0 is a'[d0' - gl - r - 1 + k], tested against
// 0 <= idx < ca.
//
// Stray bytes.  The zeros that used to stand outside a and b are now other symbols of the pair: a before a_begin and behind a_end
// (the column loader reads dwords up to the one that holds a_end; the window of step 0 does not), b behind b_end (the feeder's
// `fresh` is the pad outside 1 <= t' <= cb, so no byte of b outside the span ever enters).  A symbol has exactly one use: it
// chooses between match and mismatch in s, the diagonal move of ITS cell.  E and F of a cell read z, e and f of its neighbours
// and no symbol.  A stray byte of a stands in a column j' < 1 or j' > ca; in column 0 the diagonal input is the masked cell
// (i' - 1, -1), so s derives from minus infinity whatever it adds; every other such column is masked, and a masked cell's H is
// replaced by minus infinity after it is computed.  So every value of the fill -- H, E and F of cells that exist and of masked
// cells alike -- is what the same fill gives on a span packed by itself with zeros around it: "No wrap" (agx_sw_band_kernel.inc)
// holds word for word, with la = ca, lb = cb.  What does change is bits 0-1 of the nibbles of masked cells, where s takes part in
// a comparison of derived minus infinities, and "bits cannot steer the walk" covers them as it stands: the walk starts at the
// corner, reads cells with 1 <= i' <= cb, 1 <= j' <= ca inside the band only -- it tests that before every load -- and ends at row 0
// or column 0 without reading them.  Row 0 carries the pad, which equals no byte, so the injected diagonal input still gives
// H(0, 0) = 0 exactly, next to whatever byte a[a_begin - 1] is.
//
// The trace is laid out as in the plain build, indexed by t': (cb + G) G sw_band_trace_words(K) dwords a pair, rows 0 .. cb
// only.  A lane stores at step t' = i' + gl for 0 <= i' <= cb, so the first word it writes is its own of step gl >= 0 and the
// last that of step cb + G - 1: the r steps in front write nothing.
//
// The walk is the body of sw_walk_band (agx_sw_band_walk.inc) built with AT: the same state machine and guards; y[i' - 1] stands r bytes
// further behind the record's y_dw, x[j' - 1] behind fpad' bytes.
#include "agx_sw_band_kernel.inc"

template <int K>
__global__ void __launch_bounds__(256) sw_fill_band_trace_at(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                             const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                             uint32_t *__restrict__ trace, const uint64_t *__restrict__ goff)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.trace = trace, io.goff = goff;
    band_body<K, kBandTrace | kBandPh>(prm, img, groups, waves[wave], io);
}

__global__ void __launch_bounds__(64) sw_walk_band_at(const SwWalkRec *__restrict__ recs, const SwBandWalkRec *__restrict__ band, uint32_t n,
                                                      const uint32_t *__restrict__ img, const uint32_t *__restrict__ trace,
                                                      uint32_t *__restrict__ slots, uint32_t *__restrict__ runs)
{
    constexpr bool AT = true;
    constexpr bool DUAL = false;
#include "agx_sw_band_walk.inc"
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_trace_at<KK>},
static constexpr decltype(&sw_fill_band_trace_at<4>) kFills[kSwNumBandClasses][1] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW

int agx_sw_band_trace_at_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    const int modes[] = {mode}; // one build per class, whatever the mode
    return band_launch_fill(kFills, modes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.trace, a.goff);
}

int agx_sw_band_walk_at_launch(const SwBandWalkArgs &a, hipStream_t s) { return band_launch_walk(sw_walk_band_at, a, s); }

void agx_sw_band_trace_at_preload() { band_preload({(const void *)&sw_fill_band_trace_at<8>, (const void *)&sw_walk_band_at}); }
