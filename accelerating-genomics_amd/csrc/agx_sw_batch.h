// Private to the host side of the Smith-Waterman path -- agx_sw.cpp (create, launch, scores), agx_sw_plan.cpp (its planner),
// agx_sw_align.cpp (align batches: hits, statistics), agx_sw_band.cpp (banded batches: create, launch, hits),
// agx_sw_band_plan.cpp (their planner) and agx_sw_cigar.cpp (CIGARs) -- and included by nothing else: the batch object and what
// those files need of each other.  No kernel includes it.
#pragma once
#include "agx_sw.h"

#include <algorithm>

#include "agx_internal.h"

// (hidden: what crosses a file boundary is still no export of the library)
namespace agx_sw_host __attribute__((visibility("hidden"))) {

struct ClassLaunch {
    int C = 0;
    uint32_t first_wave = 0, n_waves = 0;
};

} // namespace agx_sw_host

struct agx_sw_batch {
    agx_ctx *ctx = nullptr; // retained
    int family = 0;         // 0 int32, 1 packed signed, 2 packed biased, 3 int32 on the packed plan's coded image, 4 locating int32, 5 anchored int32
    // align batches (agx_sw_batch_create_align): 0 = a score-only batch, else AGX_SW_ALIGN_ENDS / _SPANS
    int align = 0;
    int mode = 0; // AGX_SW_MODE_*: anything but LOCAL runs the anchored fill (agx_sw_anch_kernel.hip)
    // agx_sw_batch_create_align_stats: 0 = no statistics; 1 = a stats batch whose own fill is the plain one (LOCAL,
    // FIT: the begin pass carries L); 2 = this batch's fill is the stats build and writes L = matches << 12 | pairs per pair
    // agx_sw_batch_create_align_band_diag_stats: the same on a batch banded around a diagonal, whose L is
    // matches << 16 | pairs (kSwBandStatBits); lstat is zeroed at create, so a pair without a fill reads 0
    int stats = 0;
    DevBuf lstat;       // stats == 2: L of every pair's captured cell
    PinBuf lstat_stage; // its page-locked landing block
    // agx_sw_batch_create_align_cigar: 0 = no CIGARs; 1 = a cigar batch (a SPANS batch that keeps its sequences
    // and answers agx_sw_batch_cigars); 2 = the internal GLOBAL batch of one chunk of spans, whose fill is the traced build
    int cigar = 0;
    // cigar == 2: where every group's directions start (dwords), one walk record per pair, and the extents they add up to;
    // the trace block itself is lent by cigars_impl for the time of one chunk
    std::vector<uint64_t> tr_goff;
    std::vector<SwWalkRec> tr_walk;
    uint64_t tr_dwords = 0, tr_slot_words = 0;
    DevBuf goff, walkrec;
    uint32_t *trace_p = nullptr;
    // cigar == 1: the answer of the last agx_sw_batch_cigars, kept until the next launch
    bool cig_valid = false;
    std::vector<agx_sw_hit> cig_hits;
    std::vector<uint64_t> cig_off;
    std::vector<uint32_t> cig_ops;
    agx_sw_cigar_info cig_info{};
    // modes other than LOCAL: pairs with an empty side whose score is not the zero the device array holds for them
    std::vector<int64_t> fix_pair;
    std::vector<int32_t> fix_score;
    // agx_sw_batch_create_align_band: a banded batch -- align = SPANS, mode GLOBAL or EXTEND, its records are
    // SwBandGroup, its image bytes, launches[].C the diagonals per lane; band_pos receives EXTEND's i << 16 | j per pair
    bool banded = false;
    int32_t band = 0;
    DevBuf band_pos;
    PinBuf band_pos_stage;
    // agx_sw_batch_create_align_band_cigar: banded with cigar == 1.  The traced fills of agx_sw_batch_cigars read
    // the resident image through copies of the group records with the span's lengths: the records in plan order, every pair's
    // record (kNoBandRec: an empty side) and its tiling; seq / seq_off hold the symbols for the host's checks
    std::vector<SwBandGroup> band_groups;
    std::vector<uint32_t> band_rec;
    std::vector<uint8_t> band_cls, band_G;
    // agx_sw_batch_create_align_band_diag: banded with band_at set; align = ENDS or SPANS, any mode.  Per pair
    // the centre diagonal and the first row the fill was given (kNoBandRow: no fill -- an empty side, or a LOCAL band that
    // misses the matrix); the fill's rows are counted from there.  SPANS in LOCAL and FIT keep seq / seq_off for the begin pass
    // agx_sw_batch_create_align_band_diag_cigar: band_at with cigar == 1 and align = SPANS; it keeps band_groups,
    // band_rec, band_cls, band_G and seq like a banded cigar batch, in every mode
    // agx_sw_batch_create_align_band_zdrop[_cigar]: a band_at batch in mode EXTEND whose fill is the z-drop build;
    // band_stop receives per pair the last row looked at, or -1
    bool band_at = false, zdrop_on = false;
    int32_t zdrop = 0;
    DevBuf band_stop;
    PinBuf band_stop_stage;
    std::vector<int32_t> band_diag;
    std::vector<uint32_t> band_row0;
    // agx_sw_batch_create_align_band_diag_dual: a band_at batch under two-piece gap costs.  scoring and prm hold
    // the first piece exactly as the plain batch on the same pairs would (its plan is that batch's); dual_sc all six numbers,
    // dual_gap what the fills take beside prm
    bool dual = false;
    agx_sw_scoring_dual dual_sc{};
    SwDualGap dual_gap{};
    agx_sw_scoring scoring{};
    DevBuf ends;        // per pair: row << kSwLocColBits | column of the end cell, written by the locating fill
    PinBuf ends_stage;  // its page-locked landing block
    // SPANS: the sequences, dense, for the begin pass (the caller's arrays need not outlive the create)
    std::vector<uint8_t> seq;
    std::vector<uint64_t> seq_off;
    std::vector<uint32_t> seq_len;
    SwParams prm{};
    int64_t n_pairs = 0;
    DevBuf img, groups, waves, scores;
    DevBuf table; // substitution-matrix mode: kSwMatDim^2 int16 entries
    int rising = 0; // biased packed fill: 1 = stored values rise by |ge| per step, 4 = and by |ge| per column in classes of four (agx_sw_pk2_kernel.hip, KC)
    bool wide = false; // rising == 4: the column classes' period is C / 2 in the classes built that way (sw_pk2_period), not four
    int stage = 0; // biased packed fill: SwParams::stage of this batch's launches (set at create: all of its waves are resident at once)
    PinBuf out_stage; // page-locked landing block of the scores, taken at create: agx_sw_batch_scores allocates nothing
                      // (a first hipHostMalloc costs milliseconds, and hipvers' timed window is launch -> scores)
    bool matrix = false;
    agx_sw_matrix mat{}; // ... and the caller's matrix itself: an align batch's begin pass creates its own batch from it
    std::vector<agx_sw_host::ClassLaunch> launches;
    agx_sw_info info{};
    // A batch created without the closing wait (the pieces of agx_sw_score): its upload, planning and pack kernels may
    // still be running; the temporaries they use, the event a launch has to wait for and the symbol check's verdict
    // are held here until finish_create().
    struct SwPending *pending = nullptr;
    // agx_sw_batch_bind_scores: a page-locked array of the caller's that launches write their scores into themselves
    // (only a batch planned in file order does: its waves then write consecutive bytes)
    bool file_order = false;
    int32_t *bound = nullptr;
    // bind_scores changed `bound` and no launch has run since: neither the caller's array nor the device array holds what a
    // fetch would promise, so agx_sw_batch_scores refuses until the next launch
    bool rebound = false;
    // Completion on the dispatch (agx_sw.cpp, ensure_done_event): the event this batch's one launch carries as its stop event
    // (null: none), and agx_ctx::enqueued as that launch left it (0: no such launch yet)
    hipEvent_t done = nullptr;
    uint64_t done_at = 0;
};

namespace agx_sw_host __attribute__((visibility("hidden"))) {

// AGX_TRACE_CREATE: the launches as every plan digest takes them
inline void hash_launches(Fnv1a &f, const std::vector<ClassLaunch> &launches)
{
    for (const ClassLaunch &cl : launches) {
        f.field((int32_t)cl.C);
        f.field(cl.first_wave);
        f.field(cl.n_waves);
    }
}

constexpr uint32_t kNoBandRec = 0xffffffffu;
constexpr uint32_t kNoBandRow = 0xffffffffu;

// The band of a pair: GLOBAL widens it by the length difference, EXTEND keeps it around the main diagonal.
inline void band_limits(int mode, int64_t w, int64_t la, int64_t lb, int64_t &dlo, int64_t &dhi)
{
    const int64_t diff = mode == AGX_SW_MODE_GLOBAL ? la - lb : 0;
    dlo = std::min<int64_t>(0, diff) - w;
    dhi = std::max<int64_t>(0, diff) + w;
}

// agx_sw_batch_create_align_band_diag's part of create_band: what to report and the centre diagonal of every pair (NULL: 0)
// agx_sw_batch_create_align_band_zdrop adds its z-drop (zdrop_on; EXTEND only)
// agx_sw_batch_create_align_band_diag_stats its statistics (stats: agx_sw_batch::stats -- 1 = answers agx_sw_batch_stats from its
// begin pass, 2 = its own fill is the stats build)
struct BandAt {
    int what;
    const int32_t *diag;
    bool zdrop_on = false;
    int32_t zdrop = 0;
    int stats = 0;
    const agx_sw_scoring_dual *dual = nullptr; // agx_sw_batch_create_align_band_diag_dual: all six numbers (scoring is then unused)
};

// ---- agx_sw.cpp
int create_batch(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, const uint8_t *bases,
                 const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool defer = false, int align = 0, int mode = 0,
                 int stats = 0, int cigar = 0);
// make_constants for a batch under a matrix that create_batch does not make (create_band): the matrix validated as every matrix
// batch validates it, sc = {1, 0, gap_open, gap_extend}, the kernel constants and the kSwMatDim x kSwMatDim table
int matrix_constants(const agx_sw_matrix *matrix, agx_sw_scoring &sc, SwParams &prm, std::vector<int16_t> &table);

// ---- agx_sw_plan.cpp: the host planner, stage by stage as create_batch calls it ("create pipeline")
struct Tiling {
    int cls; // index into kSwClasses
    int G;
};

// The choice for one shorter length lx as a function of the longer length ly: cost_i(ly) = (ly + G_i - 1) * w_i
// is a line per class, the best class is their lower envelope -- a handful of segments.
struct TilingSeg {
    uint32_t ly_from; // the segment covers [ly_from, next segment's ly_from)
    uint8_t cls, G;
    double w;
};
struct TilingTable {
    std::vector<uint32_t> first; // index of lx's first segment; first[lx + 1] ends it (no segment = no class spans lx)
    std::vector<TilingSeg> segs;
    inline bool pick(uint32_t lx, uint32_t ly, Tiling *t, double *cost) const
    {
        const uint32_t a = first[lx], b = first[lx + 1];
        if (a == b) return false;
        uint32_t k = a;
        while (k + 1 < b && segs[k + 1].ly_from <= ly) ++k;
        const TilingSeg &s = segs[k];
        *t = Tiling{s.cls, s.G};
        if (cost) *cost = (double)(ly + s.G - 1) * s.w;
        return true;
    }
};
// The full tiling table of a kernel family (every class allowed, no tail term, every shorter length up to the
// family's limit): what a device-planned batch is tiled with.  Made once per process.
const TilingTable &full_tiling_table(int family);
// per-class cost table of the kernel family a batch runs (relative lane time per padded cell)
const double *class_costs(int family);
// knobs of the tuning build that the create reads as well as the planner (each read once per process)
double tail_beta_override(); // AGX_SW_TAIL_BETA; < 0 = none
int max_classes_override();  // AGX_SW_MAX_CLASSES; 0 = none

constexpr uint8_t kClsEmpty = 255;   // an empty side: nothing to fill
constexpr uint8_t kClsUntiled = 254; // pass A done, no tiling yet
struct PairPlan {                    // 12 bytes: the sorts move these
    uint32_t pair;
    uint32_t ly;
    uint16_t lxo; // lx | (1 = sequence 2p+1 is the shorter one) << 15, as the group records carry it
    uint8_t cls;
    uint8_t G;
    uint32_t lx() const { return lxo & 0x7fffu; }
};
// pair p as pass A leaves it: oriented (an align batch keeps its first sequence across the lanes), empty or not yet tiled
inline void init_pair_plan(PairPlan &pp, int64_t p, uint32_t la, uint32_t lb, int align)
{
    pp = PairPlan{};
    pp.pair = (uint32_t)p;
    pp.cls = kClsEmpty;
    if (la == 0 || lb == 0) return; // no interior cell: score stays 0
    const bool second_short = !align && lb < la; // ties keep file order (antidiagonalSmithWaterman.c:229-244)
    pp.lxo = (uint16_t)((second_short ? lb : la) | (second_short ? 0x8000u : 0u));
    pp.ly = second_short ? la : lb;
    pp.cls = kClsUntiled;
}

// Boyer-Moore majority vote over a sample of at most 512 pairs, every stride-th one below n_pairs.  shape_at(p, &sh): false
// for a pair with nothing to fill.  -> the votes left (> 0: *cand may be a majority, to be counted)
template <typename ShapeAt>
int sampled_majority_shape(size_t n_pairs, size_t stride, ShapeAt shape_at, uint32_t *cand)
{
    int votes = 0;
    for (size_t k = 0; k < 512 && k * stride < n_pairs; ++k) {
        uint32_t sh;
        if (!shape_at(k * stride, &sh)) continue;
        if (votes == 0) {
            *cand = sh;
            votes = 1;
        } else
            votes += sh == *cand ? 1 : -1;
    }
    return votes;
}

// the kernel a batch runs and what the planner needs to know of it (choose_kernel, agx_sw.cpp)
struct KernelChoice {
    int family = 0, rising = 0;
    bool packed = false;     // families 1 .. 3: two pairs per lane group
    bool coded_plan = false; // the packed plan of the biased fill (one launch for all classes)
    const double *costs = nullptr;
    int slots = 1;
};

// one (class, G) run of the sorted plan: entry j of the run is slot j % slots of its group j / slots,
// a wave takes 64 / G groups
struct Bucket {
    size_t first = 0, count = 0;     // entries of plan[]
    size_t group0 = 0, n_groups = 0; // group records
    size_t wave0 = 0, n_waves = 0;
    int cls = 0, G = 0;
};

// what the rest of a create needs of a plan, whoever made it
struct PlanLayout {
    size_t n_groups = 0, n_waves_total = 0, groups_bytes = 0, waves_bytes = 0, img_dw = 0;
    std::vector<ClassLaunch> launches;
    uint32_t launched_classes = 0; // bit k: some wave runs kSwClasses[k]
    int64_t padded = 0;
    // host-made plans only: the runs of plan[], the wave records and every entry's image offsets
    std::vector<Bucket> buckets;
    std::vector<SwWave> waves;
    std::vector<uint32_t> x_dw, y_dw;
};

// uniform batches: one tiling for the whole shape, file order kept.  false: no class fits, the host planner takes the batch
bool plan_uniform(std::vector<PairPlan> &all, uint32_t shape, int n_cu, const KernelChoice &kc, bool matrix, std::vector<PairPlan> &plan);
// passes B and C: tiling per pair, the batch-level rules, the two sorts.  Empties `all`; *t_plan: when the tiling was done
int plan_host(std::vector<PairPlan> &all, const std::vector<uint8_t> &present, uint32_t longest_long, int n_cu, const KernelChoice &kc, bool matrix,
              std::vector<PairPlan> &plan, double *t_plan);
// pass D of a device-made plan: extents from the pairs per (class, G) bucket; bt receives the planner kernels' table
// (entries before, count, first group, groups, first wave of each bucket), *entries the pairs with something to fill
PlanLayout layout_from_buckets(const std::vector<uint32_t> &hist, int slots, uint32_t *bt, size_t *entries);
// pass D of a host-made plan: buckets, waves in dispatch order, launches, image offsets
int layout_from_plan(const std::vector<PairPlan> &plan, const KernelChoice &kc, size_t img0, PlanLayout &lay);
void write_group_records(const PlanLayout &lay, const std::vector<PairPlan> &plan, const KernelChoice &kc, int64_t n_pairs, void *groups_data);
void write_trace_records(const PlanLayout &lay, const std::vector<PairPlan> &plan, int64_t n_pairs, agx_sw_batch *b);

// ---- agx_sw_align.cpp
agx_sw_hit empty_side_hit(int mode, int what, const agx_sw_scoring &sc, uint32_t la, uint32_t lb);
// ... under two-piece gap costs: the lone gap costs the cheaper piece
agx_sw_hit empty_side_hit_dual(int mode, int what, const agx_sw_scoring_dual &sc, uint32_t la, uint32_t lb);
int create_align(const char *who, agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, int what,
                 const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool stats = false,
                 bool cigar = false);
int hits_impl(agx_sw_batch *b, agx_sw_hit *hits, std::vector<uint32_t> *L);

// What a begin pass fills again: the pairs that have a begin to find (LOCAL: those with a score; fit: those that consume some of
// b) and their prefixes a[a_end..0], b[b_end..0], reversed and dense, as the arrays of a batch of their own.
struct RevPrefixes {
    std::vector<int64_t> pick;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> bytes;
};
void reversed_prefixes(const agx_sw_batch *b, const agx_sw_hit *hits, bool fit, int64_t grain, RevPrefixes &r);

// A one-shot call behind its create: launch, the answer (hits, stats or cigars), destroy.
template <typename Answer>
int align_once(agx_sw_batch *b, Answer answer)
{
    int rc = agx_sw_batch_launch(b);
    if (!rc) rc = answer(b);
    if (rc && b->ctx) (void)hipStreamSynchronize(b->ctx->stream); // the blocks go back to the pools: nothing may still run on them
    agx_sw_batch_destroy(b);
    return rc;
}

// ---- agx_sw_band_plan.cpp: the planner of banded batches, stage by stage as create_band calls it ("create
// pipeline"); none of it touches the device
// what kind of banded batch a create makes: the arguments of create_band that select checks, kernels and limits, and the entry
// point's name for the messages
struct BandKind {
    int mode;
    int32_t band;
    bool cigar;
    const BandAt *at;
    const agx_sw_matrix *matrix;
    const char *who;
};
struct BandPlan { // one pair with work, as the sort moves it
    uint32_t pair, la, lb;
    int32_t dlo, dhi;
    uint8_t cls, G;
    uint32_t row0; // a band around a diagonal: the fill is given b[row0 .. row0 + lb) and the band shifted by row0; else 0
};
// pass A's result: the pairs with work, (around a diagonal) every pair's first row or kNoBandRow, the cells of every matrix
struct BandPairs {
    std::vector<BandPlan> plan;
    std::vector<uint32_t> row0s;
    int64_t cells = 0;
};
// every check that runs before pass A; create_band binds the context between the two.  sc: what the batch is scored with
int check_band_kind(const BandKind &kind);
int check_band_arrays(const BandKind &kind, const agx_sw_scoring *scoring, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                      agx_sw_scoring &sc);
int plan_band_pairs(const BandKind &kind, const uint8_t *bases, const uint32_t *len, int64_t n_pairs, BandPairs &out);
void sort_band_plan(std::vector<BandPlan> &plan);
// The one wave builder of the banded plans, for create_band's pairs and for the spans of a cigar chunk (band_trace,
// agx_sw_cigar.cpp): waves of 64 / G groups of one (class, lanes per group), a launch per class.  sorted: by class, lanes per
// group, then rows falling; E has cls, G and lb (its rows).  -> the padded cells
template <typename E>
int64_t layout_band_waves(const std::vector<E> &sorted, std::vector<SwWave> &waves, std::vector<ClassLaunch> &launches)
{
    int64_t padded = 0;
    for (size_t k = 0, end = 0, n = sorted.size(); k < n; k = end) {
        const E &h = sorted[k];
        const int K = kSwBandClasses[h.cls], G = h.G, per_wave = 64 / G;
        while (end < n && end - k < (size_t)per_wave && sorted[end].cls == h.cls && sorted[end].G == h.G) ++end;
        SwWave w{};
        w.first_group = (uint32_t)k;
        w.n_groups = (uint16_t)(end - k);
        w.G = (uint16_t)G;
        w.steps = h.lb + (uint32_t)G; // the wave's longest target comes first
        w.reserved = (uint32_t)K;
        if (launches.empty() || launches.back().C != K) {
            ClassLaunch cl;
            cl.C = K;
            cl.first_wave = (uint32_t)waves.size();
            launches.push_back(cl);
        }
        ++launches.back().n_waves;
        waves.push_back(w);
        padded += (int64_t)w.steps * 64 * K;
    }
    return padded;
}
// the group records in plan order and the image's extent; AGX_E_LIMIT beyond the 16 GiB an image may take
int write_band_groups(const std::vector<BandPlan> &plan, std::vector<SwBandGroup> &groups, uint64_t &img_dw);
// the image bytes of groups [lo, hi) into dst (code: a matrix's byte map, or NULL) -> the first pair of the range that breaks the
// symbol rule, or -1
int64_t build_band_image(const std::vector<SwBandGroup> &groups, int64_t lo, int64_t hi, const uint8_t *bases, const uint64_t *off,
                         const uint32_t *len, const uint8_t *code, uint8_t *dst);

// ---- agx_sw_band.cpp
int create_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool cigar = false, const BandAt *at = nullptr,
                const agx_sw_matrix *matrix = nullptr);
// The selection table of the banded fills (agx_sw.h, SwBandFill), in the order a create preloads its rows, and the row of a
// batch's own fill -- or, traced, of the fill and walk of its CIGARs.  band_launch, keep_band_host_state and band_trace
// (agx_sw_cigar.cpp) read nothing else.  band_fill_failed words a failed launch of the row's kernel -> AGX_E_HIP.
constexpr int kNumBandFills = 11;
const SwBandFill *band_fills();
const SwBandFill &band_fill(const agx_sw_batch *b, bool traced);
int band_fill_failed(const SwBandFill &fill, int K, int mode);
int band_launch(agx_sw_batch *b);
// L (agx_sw_batch_stats): also the word matches << kSwBandStatBits | pairs of every pair, 0 where no fill says otherwise
int band_at_hits(agx_sw_batch *b, agx_sw_hit *hits, bool begins, std::vector<uint32_t> *L = nullptr);
int band_hits(agx_sw_batch *b, agx_sw_hit *hits);

} // namespace agx_sw_host
