// Device work records of the Smith-Waterman fill (shared by scheduler and kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/agx.h"

// One alignment pair = one group of G lanes.  Offsets are in 4-byte words into the packed
// image: x (the shorter sequence, zero-padded to G*C bytes rounded up to 4, plus one spare word),
// y (the longer, padded to 4).
struct SwGroup {
    uint32_t x_dw;
    uint32_t y_dw;
    uint32_t lx_ly; // lx | (1 = the pair's SECOND sequence is the shorter one) << 15 | ly << 16; the fills read ly only
    uint32_t out;   // index into scores[] = the caller's pair number
};

// Scoring, as the kernels consume it (built by the host from agx_sw_scoring).  With z = H + gf the
// state both gap recurrences read, a cell is  e = max(z_up, e + ge),  f = max(z_left, f + ge),
// s = H_diag + match - {0, delta},  H = max(e, f, s, 0),  z = H + gf.
struct SwParams {
    int32_t ge;      // gap extend (<= 0): every further gap cell
    int32_t gf;      // first gap cell = open + extend (<= 0)
    int32_t hd;      // match - gf: turns z_diag into H_diag + match
    int32_t delta;   // match - mismatch (> 0)
    int32_t shift;   // packed kernel: symbols are compared as byte << shift, 2^shift >= delta
    // the same, replicated into both 16-bit halves for the packed kernels
    uint32_t ge2, gf2, hd2, delta2;
    // biased packed kernel (agx_sw_pk2_kernel.hip): |ge|, |gf| and the bias B added to every stored half
    uint32_t age2, agf2, bias2;
    // slots of the scores array a launch may write (packed kernels: a vacant half points at slot n_pairs, which exists in
    // the device array but not in a caller's page-locked one -- agx_sw_batch_bind_scores)
    uint32_t n_out;
    // biased packed kernel: staged wave priority (agx_sw_pk2_kernel.inc, "Staged priority").  0 = none; 1 = a wave lowers its
    // priority at 1/2, 3/4 and 7/8 of its quads of steps; 2 = at equal quarters (tools/sw_wave_timeline.py only)
    uint32_t stage;
};

// Packed kernel: one group of G lanes carries two pairs (index 0 = low 16 bits, 1 = high 16 bits
// of every state register).  A group without a second pair points [1] at an all-zero sequence
// of length 0 and at the spare score slot scores[n_pairs].
struct SwGroup2 {
    uint32_t x_dw[2];
    uint32_t y_dw[2];
    uint32_t lx_ly[2];
    uint32_t out[2];
};

// One wavefront: n_groups groups of G lanes, all stepping `steps` rows
// (= max(ly) + G - 1 over its groups).
struct SwWave {
    uint32_t first_group;
    uint16_t n_groups;
    uint16_t G;
    uint32_t steps;
    uint32_t reserved; // class word: bits 0..15 columns per lane of this wave's class (read by the one-launch kernel of
                       // mixed batches); bit 16 set on the device by sw_pack_dna: every pair of the wave is DNA-coded
};

// Column-per-lane classes the kernels are instantiated for (any width works: a lane's symbols are
// byte-aligned on load), every even width so that common lengths tile with little padding.
#define AGX_SW_FOR_EACH_CLASS(X) \
    X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32) X(34) X(36) X(38) X(40)
// wide classes: int32 kernel only, for shorter sides beyond 64 x 40 columns (agx_sw_wide_kernel.hip)
#define AGX_SW_FOR_EACH_WIDE_CLASS(X) X(80) X(120) X(160)
static const int kSwClasses[] = {4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 80, 120, 160};
static const int kSwPackedMaxShort = 64 * 40; // the packed kernel has no wide classes
static const int kSwNumClasses = sizeof(kSwClasses) / sizeof(kSwClasses[0]);
// Measured lane time per padded cell of each class, relative to the widest one (MI355X,
// tools/calibrate_classes.py, profiles/r01_calibration*.log): narrow classes amortise the
// per-step work (DPP shifts, row symbol, loop control) over fewer cells.
static const double kSwClassCost[] = {1.373, 1.250, 1.178, 1.138, 1.112, 1.080, 1.051, 1.033, 1.025, 1.022, 1.014, 1.014, 1.011, 1.007, 1.007, 1.004, 1.004, 1.004, 1.000, 1.6, 2.2, 4.0};
// same for the packed int16 kernel
static const double kSwPkClassCost[] = {1.543, 1.358, 1.278, 1.210, 1.173, 1.136, 1.111, 1.086, 1.068, 1.037, 1.025, 1.025, 1.019, 1.012, 1.006, 1.006, 1.006, 1.000, 1.000, 0, 0, 0}; // 0 = not built
// and for its biased formulation (agx_sw_pk2_kernel.hip, the DNA-coded rising cell with column classes; tools/cal_sw_pk.py,
// profiles/r02h_cal_sw_pk2.log: 0.0951 ps per padded cell at 40 columns)
static const double kSwPk2ClassCost[] = {1.851, 1.581, 1.450, 1.367, 1.318, 1.263, 1.196, 1.184, 1.145, 1.097, 1.095, 1.056, 1.049, 1.053, 1.025, 1.023, 1.022, 1.016, 1.000, 0, 0, 0};

// the 32-bit fill on the packed plan's coded image (agx_sw_i32d_kernel.hip): the int32 kernel's per-class costs, no wide classes
static const double kSwI32dClassCost[] = {1.373, 1.250, 1.178, 1.138, 1.112, 1.080, 1.051, 1.033, 1.025, 1.022, 1.014, 1.014, 1.011, 1.007, 1.007, 1.004, 1.004, 1.004, 1.000, 0, 0, 0};

// substitution-matrix mode: symbol numbers 1..32 in the image, 0 = padding; the device table is
// kSwMatDim x kSwMatDim int16 entries score - (gap_open + gap_extend)
constexpr int kSwMatDim = 33;
int agx_sw_mat_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                            const SwWave *waves, uint32_t n_waves, int32_t *scores, const int16_t *table, hipStream_t s);
// Builds the image the records describe from the caller's raw arrays, on the device (agx_sw_pack_kernel.hip).
// raw = bases[base ..), off = the caller's offsets (absolute), groups = SwGroup (slots 1) or SwGroup2 (slots 2)
// records, code = substitution-matrix byte map or NULL, flag[2] = {offending pairs, smallest of them}.
int agx_sw_pack_launch(bool matrix, int slots, const uint8_t *raw, const uint64_t *off, uint64_t base, const void *groups,
                       uint32_t n_groups, uint32_t n_pairs, uint32_t *img, const uint8_t *code, uint32_t *flag, int n_cu,
                       hipStream_t s);
// The biased packed fill's variant: one pack wavefront per fill wavefront, DNA-codes the waves whose pairs all qualify
// (rewrites their group records' lengths and sets bit 16 of the wave records' class word).
int agx_sw_pack_dna_launch(const uint8_t *raw, const uint64_t *off, uint64_t base, void *groups, void *waves, uint32_t n_waves,
                           uint32_t n_pairs, uint32_t *img, uint32_t *flag, int n_cu, hipStream_t s);
int agx_sw_pk_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups,
                           const SwWave *waves, uint32_t n_waves, int32_t *scores, hipStream_t s);
// The biased packed fill's column classes (rising == 4): column j of a lane carries (j mod P) |ge|.  P = 4 ("narrow") in every
// class, or P = C / 2 ("wide", agx_sw_pk2w_kernel.hip) from 14 columns per lane on: the host chooses per batch (agx_sw.cpp,
// "class period").  This is the period of class C's wide build; classes named in AGX_SW_PK2_KEEP_NARROW keep four there too
// (their wide build passes 256 VGPRs or spills).
#define AGX_SW_PK2_KEEP_NARROW(C) (false)
constexpr int sw_pk2_period(int C) { return C >= 14 && !AGX_SW_PK2_KEEP_NARROW(C) ? C / 2 : 4; }
// stop (the biased fill's launchers only): an event the dispatch itself carries as its stop event, so that the batch's fetch can wait
// for this launch alone (agx_sw.cpp, "Completion on the dispatch"); NULL: a plain launch
int agx_sw_pk2_launch_class(int cols_per_lane, int rising, bool wide, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups,
                            const SwWave *waves, uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop = nullptr);
int agx_sw_pk2w_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves,
                             uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop = nullptr);
int agx_sw_pk2w_launch_any(const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves, uint32_t n_waves,
                           int32_t *scores, hipStream_t s, hipEvent_t stop = nullptr);
// one launch of 256-thread workgroups: with stop, hipExtLaunchKernelGGL binds that event to the kernel's own packet
#define AGX_SW_PK2_LAUNCH(kernel, blocks, s, stop, ...)                                                            \
    do {                                                                                                           \
        if (stop)                                                                                                  \
            hipExtLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, nullptr, stop, 0, __VA_ARGS__);           \
        else                                                                                                       \
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, __VA_ARGS__);                                \
    } while (0)
void agx_sw_pk2w_preload();
// every class of a mixed batch in one launch: waves[].reserved holds each wave's columns per lane
void agx_sw_pk2_preload();
void agx_sw_pack_preload();
void agx_sw_i32_preload();
int agx_sw_pk2_launch_any(int rising, bool wide, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves,
                          uint32_t n_waves, int32_t *scores, hipStream_t s, hipEvent_t stop = nullptr);
// the 32-bit fill with the DNA-coded match: the packed plan's records and image, one pair of a lane group at a time
int agx_sw_i32d_launch_any(const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves, uint32_t n_waves, int32_t *scores,
                           hipStream_t s);
int agx_sw_i32d_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup2 *groups, const SwWave *waves,
                             uint32_t n_waves, int32_t *scores, hipStream_t s);
void agx_sw_i32d_preload();
int agx_sw_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                        const SwWave *waves, uint32_t n_waves, int32_t *scores, hipStream_t s);
int agx_sw_wide_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                             const SwWave *waves, uint32_t n_waves, int32_t *scores, hipStream_t s);
// the locating fill of align batches (agx_sw_loc_kernel.hip): the int32 kernel's records and byte image with the pair's FIRST
// sequence across the lanes; besides scores[out] it writes ends[out] = row (position in the second sequence) << 12 | column
// (position in the first) of the first cell in (row, column) order that holds the maximum, 0xffffffff when the score is 0
constexpr int kSwLocColBits = 12;
int agx_sw_loc_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                            uint32_t n_waves, int32_t *scores, uint32_t *ends, hipStream_t s);
void agx_sw_loc_preload();
// the anchored fill of the align modes GLOBAL / FIT / EXTEND / EXTEND_QUERY (agx_sw_anch_kernel.hip): the locating fill's plan,
// no zero floor, gap-initialised boundaries.  capture 0 = the first maximum anywhere (EXTEND), 1 = in the query's last column;
// flags: 1 = free target start (FIT), 2 = report the corner cell (GLOBAL).  ends[out] = (row + 1) << 12 | (column + 1).
int agx_sw_anch_launch_class(int cols_per_lane, int capture, int flags, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                             const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *ends, hipStream_t s);
void agx_sw_anch_preload();
// the two align fills under a substitution matrix (agx_sw_loc_mat_kernel.hip, agx_sw_anch_mat_kernel.hip): the
// same records, plans and ends[] words on the matrix image of agx_sw_mat_launch_class (symbol numbers, 0 = padding) with its table
int agx_sw_loc_mat_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                uint32_t n_waves, int32_t *scores, uint32_t *ends, const int16_t *table, hipStream_t s);
void agx_sw_loc_mat_preload();
int agx_sw_anch_mat_launch_class(int cols_per_lane, int capture, int flags, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                                 const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *ends, const int16_t *table, hipStream_t s);
void agx_sw_anch_mat_preload();
// the align fills WITH alignment statistics (agx_sw_*_stats_kernel.hip): the same records, plans, images and
// ends[] words; every state carries L = matches << 12 | pairs of its best path beside the score, and lstat[out] receives L of
// the captured cell.  Built for the classes below only (see DESIGN.md 4.1e for the ones left out).
#define AGX_SW_FOR_EACH_STATS_CLASS(X) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28)
constexpr int kSwStatsTopClass = 28; // 64 x 28 = AGX_SW_STATS_MAX_QUERY_LEN
// the int32 kernel's relative costs for the classes that are built (unmeasured for these kernels), 0 = not built
static const double kSwStatsClassCost[] = {1.373, 1.250, 1.178, 1.138, 1.112, 1.080, 1.051, 1.033, 1.025, 1.022, 1.014, 1.014, 1.011, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr int kSwStatColBits = 12; // L = matches << 12 | pairs
int agx_sw_loc_stats_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                  uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat, hipStream_t s);
int agx_sw_loc_mat_stats_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                      uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat, const int16_t *table, hipStream_t s);
int agx_sw_anch_stats_launch_class(int cols_per_lane, int capture, int flags, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                                   const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat, hipStream_t s);
int agx_sw_anch_mat_stats_launch_class(int cols_per_lane, int capture, int flags, const SwParams &prm, const uint32_t *img, const SwGroup *groups,
                                       const SwWave *waves, uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *lstat,
                                       const int16_t *table, hipStream_t s);
void agx_sw_loc_stats_preload();
void agx_sw_loc_mat_stats_preload();
void agx_sw_anch_stats_preload();
void agx_sw_anch_mat_stats_preload();
// the TRACED anchored fill (agx_sw_trace_kernel.hip, agx_sw_trace_mat_kernel.hip): COL capture with the GLOBAL flag
// only.  Besides score and end cell every cell leaves four bits -- where H came from and whether E / F extended -- at
// trace + goff[group] + (step * G + lane) * W dwords, W = sw_trace_words(C); goff holds one 64-bit dword offset per group record.
// Built for the classes below only: the matrix build reports a spilled register from 34 columns on, the match/mismatch build from
// 36 (DESIGN.md 4.1f has the table), and one list serves both.
#define AGX_SW_FOR_EACH_TRACE_CLASS(X) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32)
constexpr int kSwTraceTopClass = 32; // 64 x 32 = AGX_SW_CIGAR_MAX_QUERY_LEN
// the int32 kernel's relative costs for the classes that are built (unmeasured for these kernels), 0 = not built
static const double kSwTraceClassCost[] = {1.373, 1.250, 1.178, 1.138, 1.112, 1.080, 1.051, 1.033, 1.025, 1.022, 1.014, 1.014, 1.011, 1.007, 1.007, 0, 0, 0, 0, 0, 0, 0};
static_assert(64 * kSwTraceTopClass == AGX_SW_CIGAR_MAX_QUERY_LEN, "the query limit of a cigar batch follows the widest traced class");
constexpr int sw_trace_words(int C) { return (C + 7) / 8; } // dwords of one lane's nibbles of one step
// the dwords a traced pair of ly rows occupies in class C on G lanes: steps 0 .. ly + G - 2 of G lanes
inline uint64_t sw_trace_dwords(int G, uint32_t ly, int C) { return ((uint64_t)ly + (uint64_t)G - 1u) * (uint64_t)G * (uint64_t)sw_trace_words(C); }
int agx_sw_trace_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                              uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *trace, const uint64_t *goff, hipStream_t s);
int agx_sw_trace_mat_launch_class(int cols_per_lane, const SwParams &prm, const uint32_t *img, const SwGroup *groups, const SwWave *waves,
                                  uint32_t n_waves, int32_t *scores, uint32_t *ends, uint32_t *trace, const uint64_t *goff, const int16_t *table,
                                  hipStream_t s);
void agx_sw_trace_preload();
void agx_sw_trace_mat_preload();
// the walk over a traced fill's directions (agx_sw_walk_kernel.hip): one lane per pair, from the corner in state H by the tie
// rule of include/agx.h ("Alignment itself").  Operations (length << 4 | BAM code) land right-aligned in the pair's slot of
// ca + cb words, so they read forwards; runs[pair] receives their number.  The gather kernel packs them at dst[pair].
struct SwWalkRec {
    uint64_t goff;       // the pair's directions, in dwords from the trace block
    uint64_t slot;       // first word of its slot
    uint32_t x_dw, y_dw; // its symbols in the image, as its group record has them
    uint32_t ca, cb;     // columns (query), rows (target)
    uint16_t G, C;       // lanes of its group, columns per lane
    uint32_t reserved;
};
int agx_sw_walk_launch(const SwWalkRec *recs, uint32_t n, const uint32_t *img, const uint32_t *trace, uint32_t *slots, uint32_t *runs,
                       hipStream_t s);
int agx_sw_gather_launch(const SwWalkRec *recs, uint32_t n, const uint32_t *slots, const uint32_t *runs, const uint64_t *dst, uint32_t *out,
                         hipStream_t s);
void agx_sw_walk_preload();

// ---- the banded fill of agx_sw_batch_create_align_band (agx_sw_band_kernel.hip): the lanes of a group own the
// diagonals dlo .. dhi of one pair, K consecutive ones per lane.  Its image is bytes: a (the query) behind fpad zero bytes, b (the
// target) behind one byte, each padded with zeros to a dword; its waves are SwWave records (G lanes per group, steps = max lb + G).
struct SwBandGroup {
    uint32_t x_dw;    // a: fpad zero bytes, la symbols, zeros to the dword
    uint32_t y_dw;    // b: one byte, lb symbols, zeros to the dword
    uint32_t la_lb;   // la | lb << 16
    int32_t dlo, dhi; // the band: dlo <= j - i <= dhi
    uint32_t out;     // the caller's pair number
    uint32_t fpad;    // (-(dlo + G K - G)) mod 4: the byte the group's last lane loads at step t is dword-aligned when t % 4 == 0
    uint32_t reserved; // host only (no kernel reads it): a band around a diagonal starts b at this row, dlo / dhi are shifted by it
                       // (the span records of sw_fill_band_trace_at alone carry their start phase here)
};
#define AGX_SW_FOR_EACH_BAND_CLASS(X) X(4) X(8) X(16) X(32)
static const int kSwBandClasses[] = {4, 8, 16, 32};
constexpr int kSwNumBandClasses = 4;
static_assert(64 * 32 == AGX_SW_BAND_MAX_WIDTH, "the widest band is 64 lanes of the widest class");
// ---- the launch interface of the banded family.  Ten translation units build the body (agx_sw_band_kernel.inc) in its variants;
// each exports ONE fill entry of the type below and one preload, the traced ones a walk.  agx_sw_host::band_fill
// (agx_sw_band.cpp) picks a batch's SwBandFill row; the launch, the create's preloads and the traced fills of agx_sw_batch_cigars
// all go through that row.
// The second piece of TWO-PIECE gap costs: prm holds the first piece exactly as a plain batch's does, this travels beside it.
struct SwDualGap {
    int32_t ge2; // the second piece's gap_extend
    int32_t dgf; // (gap_open2 + gap_extend2) - prm.gf: what piece 2 adds to the stored z = H + gf
};
// What a fill launch is given: the members every build reads, then those of single variants (an entry reads its own; the rest
// may stay zero).
struct SwBandArgs {
    SwParams prm;
    SwDualGap dual_gap; // two-piece builds
    const uint32_t *img;
    const SwBandGroup *groups;
    const SwWave *waves; // of this launch's class
    uint32_t n_waves;
    int32_t *scores;
    uint32_t *pos;        // untraced builds: EXTEND and LOCAL i << 16 | j of the best cell's first occurrence (z-drop, LOCAL: 0xffffffff if
                          // none beats 0), FIT and EXTEND_QUERY the smallest best row i of column la; GLOBAL writes none
    uint32_t *trace;      // traced builds: the directions, and one 64-bit dword offset per group record
    const uint64_t *goff;
    int32_t zdrop;        // z-drop build
    int32_t *stops;       // z-drop build: the last row looked at (counted from 0 in b) of a pair that terminated, -1 of one that ran through
    uint32_t *lstat;      // stats builds: matches << kSwBandStatBits | pairs of the captured cell's best path
    const int16_t *table; // matrix builds: the device copy of the kSwMatDim x kSwMatDim entries of agx_sw_mat_launch_class
};
// -> 0, -1 the launch failed (hipGetLastError says why), -2 the unit builds no such class K or mode
using SwBandFillFn = int (*)(int K, int mode, const SwBandArgs &a, hipStream_t s);
// the band-aware walk: pair p's SwWalkRec (G = lanes, C = diagonals per lane, x_dw / y_dw of its band image) and its band.  It
// tests dlo <= j - i <= dhi, i <= cb, j <= ca before every load; a violation leaves kSwWalkFailed in runs[p].
struct SwBandWalkRec {
    int32_t dlo, dhi;
    uint32_t fpad;   // zero bytes in front of a in the image
    uint32_t kshift; // log2 of the diagonals per lane
};
constexpr uint32_t kSwWalkFailed = 0xffffffffu;
struct SwBandWalkArgs {
    const SwWalkRec *recs;
    const SwBandWalkRec *band;
    uint32_t n;
    const uint32_t *img, *trace;
    uint32_t *slots, *runs;
};
using SwBandWalkFn = int (*)(const SwBandWalkArgs &a, hipStream_t s);
// a row of the selection table
struct SwBandFill {
    const char *name; // the kernel, as a failed launch names it: name<K> or, of a build per mode, name<K, mode>
    bool per_mode;
    unsigned needs;   // kSwBand*: what a batch's kind must include for a create to preload this row
    SwBandFillFn launch;
    void (*preload)();
    SwBandWalkFn walk; // traced fills: the walk over their directions
};
enum : unsigned { kSwBandAt = 1, kSwBandZdrop = 2, kSwBandStats = 4, kSwBandDual = 8, kSwBandMatrix = 16, kSwBandTraced = 32 };

// agx_sw_band_kernel.hip: modes GLOBAL (scores[out] = D[lb][la]) and EXTEND (the maximum and pos)
int agx_sw_band_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_preload();
// the builds of the same body for a band around a caller-given diagonal (agx_sw_band_diag_kernel.hip): mode LOCAL,
// FIT or EXTEND_QUERY; GLOBAL and EXTEND run agx_sw_band_launch
int agx_sw_band_at_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_at_preload();
// the EXTEND build with z-drop termination (agx_sw_band_zdrop_kernel.hip): scores and pos as EXTEND writes them
int agx_sw_band_zdrop_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_zdrop_preload();
// the builds WITH alignment statistics (agx_sw_band_stats_kernel.hip): mode GLOBAL, EXTEND, LOCAL or EXTEND_QUERY (the
// last two are also the begin passes of LOCAL and FIT); records, scores and pos as the plain builds of that mode write them.
// Every class of AGX_SW_FOR_EACH_BAND_CLASS is built: none spills or takes scratch, AGPRs or LDS (DESIGN.md 4.1m has the table),
// so a stats batch is tiled like a plain one.
constexpr int kSwBandStatBits = 16; // L = matches << 16 | pairs: both up to 65 535
int agx_sw_band_stats_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_stats_preload();
// the builds under TWO-PIECE gap costs (agx_sw_band_dual_kernel.hip): all five modes -- sw_fill_band_dual in GLOBAL
// and EXTEND, sw_fill_band_dual_at in the others; records, scores and pos as the plain builds of that mode write them.  Every
// class is built without scratch, AGPRs or LDS.
int agx_sw_band_dual_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_dual_preload();
// the TRACED banded fill and its walk (agx_sw_band_trace_kernel.hip): corner capture only, whatever the mode.  Every
// cell of rows 0 .. lb leaves four bits at trace + goff[group] + (step * G + lane) * sw_band_trace_words(K) dwords, nibble k of the
// lane's K diagonals; goff holds one 64-bit dword offset per group record, a multiple of four (the K = 32 build stores 16 bytes at once).
constexpr int sw_band_trace_words(int K) { return (K + 7) / 8; }
// the dwords a traced pair of lb rows occupies in class K on G lanes: steps 0 .. lb + G - 1 of G lanes, rounded up to four
inline uint64_t sw_band_trace_dwords(int G, uint32_t lb, int K)
{
    return (((uint64_t)lb + (uint64_t)G) * (uint64_t)G * (uint64_t)sw_band_trace_words(K) + 3u) & ~(uint64_t)3u;
}
int agx_sw_band_trace_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
int agx_sw_band_walk_launch(const SwBandWalkArgs &a, hipStream_t s);
void agx_sw_band_trace_preload();
// the same for a span that begins inside the resident image (agx_sw_band_diag_trace_kernel.hip): the group record
// is the span's (agx_sw_band_span_record: la_lb the span, dlo / dhi and fpad shifted, y_dw moved by whole dwords) with the start
// phase 0 .. 3 in `reserved`, and the wave steps max(cb + phase) + G times; the walk's SwWalkRec.reserved holds the phase too
int agx_sw_band_trace_at_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
int agx_sw_band_walk_at_launch(const SwBandWalkArgs &a, hipStream_t s);
void agx_sw_band_trace_at_preload();
// the traced build and the walk UNDER TWO-PIECE gap costs (agx_sw_band_dual_trace_kernel.hip): the span records,
// the start phase, scores and goff of agx_sw_band_trace_at_launch; every cell leaves EIGHT bits -- bits 0-1 where H came
// from, bit 2 "of piece 2", bits 4-7 E1, F1, E2, F2 extended -- at trace + goff[group] + (step * G + lane) *
// sw_band_dual_trace_words(K) dwords, byte k of the lane's K diagonals (K = 32: two stores of 16 bytes)
constexpr int sw_band_dual_trace_words(int K) { return K / 4; }
inline uint64_t sw_band_dual_trace_dwords(int G, uint32_t lb, int K)
{
    return (((uint64_t)lb + (uint64_t)G) * (uint64_t)G * (uint64_t)sw_band_dual_trace_words(K) + 3u) & ~(uint64_t)3u;
}
int agx_sw_band_trace_dual_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
int agx_sw_band_walk_dual_launch(const SwBandWalkArgs &a, hipStream_t s);
void agx_sw_band_trace_dual_preload();
// the builds of the banded body under a substitution matrix (agx_sw_band_diag_mat_kernel.hip, agx_sw_band_diag_trace_mat_kernel.hip;
// DESIGN.md 4.1l): a band around a caller-given diagonal in all five modes, and the traced build with the start phase.  The image
// holds symbol numbers 1 .. 32 (0 = padding) where the other banded builds hold bytes.  Records, scores, pos, trace and goff are
// those of the builds above; the walk of a traced span is agx_sw_band_walk_at_launch
int agx_sw_band_mat_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_mat_preload();
int agx_sw_band_trace_mat_launch(int K, int mode, const SwBandArgs &a, hipStream_t s);
void agx_sw_band_trace_mat_preload();

// ---- device-side planning (agx_sw_plan_kernel.hip): the O(pairs) passes of the planner as kernels
constexpr uint32_t kSwPlanEmptyKey = 1u << 27;           // sort key of a pair with an empty side: behind every bucket
constexpr uint32_t kSwPlanWaveKeyMax = (1u << 24) - 1u;  // wave dispatch key = this - steps x columns per lane
constexpr int kSwPlanBuckets = kSwNumClasses * 64;       // bucket id = class index * 64 + (64 - lanes per group)
struct SwPlanArgs {
    const uint32_t *len;        // the caller's len[], on the device
    uint32_t n_pairs, n_fill;   // pairs / pairs with work
    const uint32_t *seg_first;  // tiling table: segments of shorter length lx are [seg_first[lx], seg_first[lx + 1])
    const uint32_t *segs;       // ly_from | class index << 16 | lanes per group << 24
    uint32_t longest;           // longest longer side of the batch
    const uint32_t *buckets;    // kSwPlanBuckets x {first entry, entries, first group, groups, first wave}
    uint32_t img0;              // image word the first block starts at
    int slots;                  // pairs per lane group (2 = packed kernels)
    uint32_t n_waves;
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b;                       // n_pairs words each
    uint32_t *wave_keys_a, *wave_keys_b, *wave_ids_a, *wave_ids_b;   // n_waves words each
    SwWave *waves_tmp, *waves;                                        // n_waves records each; `waves` receives the dispatch order
    uint32_t *groups;                                                 // SwGroup / SwGroup2 records
    unsigned long long *padded;                                       // += padded cells
    void *temp;
    size_t temp_bytes;
    int n_cu;
};
size_t agx_sw_plan_temp_bytes(uint32_t n_pairs, uint32_t n_waves);
int agx_sw_plan_launch(const SwPlanArgs &a, hipStream_t s);
void agx_sw_plan_preload();
