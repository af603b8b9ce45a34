// The banded fills WITH alignment statistics (include/agx.h, "Statistics for batches banded around a diagonal"):
// the body is agx_sw_band_kernel.inc built with STATS, whose head says how the fill works.  Every state -- z, e, f and what the
// lanes hand each other -- is the tuple (score, L) held as one int64, score << 32 | L with L = matches << 16 | pairs, and lstat[out]
// receives L of the captured cell.  Four builds per K = diagonals per lane: the pinned fills sw_fill_band<K, false> (GLOBAL) and
// <K, true> (EXTEND), and the fills around a diagonal sw_fill_band_at<K, LOCAL> and <K, EXTEND_QUERY>, which are also the begin
// passes of LOCAL and FIT -- a stats batch in those two modes keeps its plain forward fill and takes L from the begin pass, so
// there is no FIT build; nor is there a TRACE, PH, ZD or MAT one.  All four K are built: the code objects report no scratch, no
// spill, no AGPRs and no LDS, K = 32 at 184 to 191 VGPRs (DESIGN.md 4.1m has the table).
//
// The tuple.  One signed 64-bit compare orders tuples by score, then matches, then pairs (the low word compares as unsigned
// under a signed high word), so max is v_cmp_gt_i64 and two selects.  A gap adds to the score word only.  A diagonal move adds
// match or mismatch to the score word and, to the low word, 0x10001 for a match, 1 for a mismatch -- and NOTHING when its row lies
// outside 1 .. lb (the row symbol is kBandRowPad) or its column outside 1 .. la (the window's byte is 0, the padding; byte 0x00 is
// refused on input, so no symbol of a is 0).  The two words are added separately: no carry can pass from L into the score, whatever
// L holds.
//
// L never wraps, and every L that is read is the count of a path.
//   true cells     a path to (i, j), 0 <= i <= lb, 0 <= j <= la, holds at most min(i, j) pairs, each in a row 1 .. lb and a column
//                  1 .. la, so matches <= pairs <= min(la, lb) <= 65 535: the low word reaches exactly 0xFFFFFFFF (an identical
//                  pair of 65 535 x 65 535) and not more.  E and F of a true cell are gap moves from true cells: the same L.
//   masked cells   after a cell is computed its H is replaced by exactly (-2^30, 0) unless the cell exists -- both words, so
//                  what a diagonal move or a gap then derives from it starts from L = 0.
//   E and F of masked cells  stay as computed, as in the plain build, and are read only by other masked cells (the head of
//                  agx_sw_band_kernel.inc says which).  They are gap moves: their L is that of the H they opened from -- a true
//                  cell's (rows > lb read row lb as "up", columns > la read column la as "left") or a masked one's 0 -- so it
//                  is again at most min(la, lb) in both fields.
//   the rows a wave steps on   a group's lanes run lb + G steps and the wave may run more for a longer neighbour.  Those rows
//                  are > lb: every cell is masked, every diagonal move in them adds nothing to L (their row symbol is the pad),
//                  and their gap moves carry an L that was already within the bound.  The same holds for rows < 0 before a
//                  lane's first row and for the columns < 0 and > la of every row.
// Hence the only additions to a low word happen in cells with 1 <= i <= lb and 1 <= j <= la, onto the L of the cell
// (i - 1, j - 1): a true cell's, or 0 from a masked one (LOCAL, or a cell the band has just admitted).
//
// The origin.  The pinned builds make H(0, 0) = 0 by setting the diagonal input of cell (0, 0) to (-mismatch, 0): the move over
// padding adds the mismatch score to the score word and, row 0 being outside 1 .. lb, nothing to L, so H(0, 0) = (0, 0).  LOCAL's
// floor is the tuple (0, 0) = int64 0.  Under {1, 0, 0, 0} a move over padding scores 0; had it counted a pair, (0, 1) would beat
// the floor and every stat would be one pair too high.
//
// No wrap of the score word: it holds exactly the values of the plain builds (the tuple's score never depends on L), so "No
// wrap" at the head of agx_sw_band_kernel.inc and of agx_sw_band_diag_kernel.hip holds as it stands.
//
// Capture reads the score word alone -- EXTEND's and LOCAL's first strict improvement of the row maximum with the leftmost cell
// that holds it, column la's smallest row, the corner, and the reductions over a group's lanes -- so hits are those of the plain
// builds bit for bit; L is read at the cell so chosen and travels with the winner.
#include "agx_sw_band_kernel.inc"

template <int K, bool EXT>
__global__ void __launch_bounds__(256) sw_fill_band_stats(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                          const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                          uint32_t *__restrict__ pos, uint32_t *__restrict__ lstat)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos, io.lstat = lstat;
    band_body<K, band_ext(EXT) | kBandStats>(prm, img, groups, waves[wave], io);
}

template <int K, int MODE>
__global__ void __launch_bounds__(256) sw_fill_band_at_stats(const SwParams prm, const uint32_t *__restrict__ img, const SwBandGroup *__restrict__ groups,
                                                             const SwWave *__restrict__ waves, uint32_t n_waves, int32_t *__restrict__ scores,
                                                             uint32_t *__restrict__ pos, uint32_t *__restrict__ lstat)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;
    BandIo io;
    io.scores = scores, io.pos = pos, io.lstat = lstat;
    band_body<K, band_ext(MODE == AGX_SW_MODE_LOCAL) | kBandStats, MODE>(prm, img, groups, waves[wave], io);
}

} // namespace

#define AGX_SW_ROW(KK) {sw_fill_band_stats<KK, false>, sw_fill_band_stats<KK, true>, sw_fill_band_at_stats<KK, AGX_SW_MODE_LOCAL>, sw_fill_band_at_stats<KK, AGX_SW_MODE_EXTEND_QUERY>},
static constexpr decltype(&sw_fill_band_stats<4, false>) kFills[kSwNumBandClasses][4] = {AGX_SW_FOR_EACH_BAND_CLASS(AGX_SW_ROW)};
#undef AGX_SW_ROW
static constexpr int kModes[] = {AGX_SW_MODE_GLOBAL, AGX_SW_MODE_EXTEND, AGX_SW_MODE_LOCAL, AGX_SW_MODE_EXTEND_QUERY};

int agx_sw_band_stats_launch(int K, int mode, const SwBandArgs &a, hipStream_t s)
{
    return band_launch_fill(kFills, kModes, K, mode, a.n_waves, s, a.prm, a.img, a.groups, a.waves, a.n_waves, a.scores, a.pos, a.lstat);
}

void agx_sw_band_stats_preload() { band_preload({(const void *)&sw_fill_band_stats<8, false>}); }
