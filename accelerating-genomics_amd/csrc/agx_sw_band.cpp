// ------------------------------------------------------------------ banded batches (include/agx.h, "Banded alignment")
// Their create (around the main diagonal or a given one) as a driver over stages -- the planner's are in agx_sw_band_plan.cpp,
// the ones that fill the batch object and the device are here -- their launch and their hits; the CIGARs of banded batches are
// in agx_sw_cigar.cpp.
#include "agx_sw_batch.h"

#include <string>

#include "agx_parallel.h"

using namespace agx_sw_host;

namespace {

// ---- AGX_TRACE_CREATE: the banded plan and its image as numbers (Fnv1a, field by field), in lines that
// tests/test_sw_band_plan_digest_cpu.py pins per kind of batch (tests/sw_band_plan_cases.py)

// what a banded plan says before its records: the kind, the kernel constants, the launches
void hash_band_head(Fnv1a &f, const agx_sw_batch *b)
{
    for (int32_t v : {(int32_t)b->mode, b->band, (int32_t)b->align, (int32_t)b->band_at, b->zdrop_on ? b->zdrop : -1, (int32_t)b->cigar,
                      (int32_t)b->matrix, b->prm.ge, b->prm.gf, b->prm.hd, b->prm.delta})
        f.field(v);
    f.field(b->prm.n_out);
    if (b->stats) f.field((int32_t)b->stats); // (the other kinds keep the digests they have)
    hash_launches(f, b->launches);
}
void hash_band_waves(Fnv1a &f, const std::vector<SwWave> &waves)
{
    for (const SwWave &w : waves) f.field(w.first_group), f.field(w.n_groups), f.field(w.G), f.field(w.steps), f.field(w.reserved);
}
void hash_band_groups(Fnv1a &f, const std::vector<SwBandGroup> &groups)
{
    for (const SwBandGroup &g : groups)
        f.field(g.x_dw), f.field(g.y_dw), f.field(g.la_lb), f.field(g.dlo), f.field(g.dhi), f.field(g.out), f.field(g.fpad), f.field(g.reserved);
}

// The kind line, the digest and the parts line.  The digest covers the head, every wave and group record, the first rows, the
// centre diagonals of a batch around a diagonal and the tables a cigar batch keeps for its traced fills (band_rec, band_cls,
// band_G) -- made here from the plan itself, since a plan-only batch does not keep them.  The parts line hashes head, waves and
// groups afresh, so that two digests that differ say where, and counts what shows that a case reached its branch: the groups,
// how many have each fpad, the rows of b the fills are not given, the diagonals per lane of every launch.
void trace_band_plan(const agx_sw_batch *b, const std::vector<SwWave> &waves, const std::vector<SwBandGroup> &groups,
                     const std::vector<uint32_t> &row0s, const int32_t *diag, const uint32_t *len)
{
    fprintf(stderr, "[agx_sw_batch_create_band] kind: mode %d band %d align %d at %d zdrop %d cigar %d matrix %d%s\n", b->mode, b->band, b->align,
            (int)b->band_at, b->zdrop_on ? b->zdrop : -1, b->cigar, (int)b->matrix,
            b->dual ? " dual" : b->stats == 2 ? " stats 2" : b->stats ? " stats 1" : "");
    Fnv1a all, head, wv, gr;
    hash_band_head(all, b), hash_band_head(head, b);
    hash_band_waves(all, waves), hash_band_waves(wv, waves);
    hash_band_groups(all, groups), hash_band_groups(gr, groups);
    for (uint32_t r : row0s) all.field(r);
    if (b->band_at)
        for (int64_t p = 0; p < b->n_pairs; ++p) all.field(diag ? diag[p] : (int32_t)0);
    if (b->cigar) {
        std::vector<uint32_t> rec((size_t)b->n_pairs, kNoBandRec);
        for (size_t k = 0; k < groups.size(); ++k) rec[groups[k].out] = (uint32_t)k;
        for (uint32_t r : rec) all.field(r);
        for (int tab = 0; tab < 2; ++tab) // band_cls, then band_G: every group has its wave's
            for (const SwWave &w : waves) {
                const int cls = (int)(std::find(kSwBandClasses, kSwBandClasses + kSwNumBandClasses, (int)w.reserved) - kSwBandClasses);
                for (uint32_t k = 0; k < w.n_groups; ++k) all.field((uint8_t)(tab ? w.G : cls));
            }
    }
    size_t fpad[4] = {0, 0, 0, 0};
    unsigned long long trimmed = 0;
    for (const SwBandGroup &g : groups) {
        ++fpad[g.fpad & 3u];
        trimmed += len[2 * (size_t)g.out + 1] - (g.la_lb >> 16);
    }
    std::string ks;
    for (const ClassLaunch &cl : b->launches) ks += " " + std::to_string(cl.C);
    fprintf(stderr, "[agx_sw_batch_create_band] plan digest %016llx\n", (unsigned long long)all.h);
    fprintf(stderr,
            "[agx_sw_batch_create_band] plan parts: head %016llx waves %016llx groups %016llx; %zu groups; fpad %zu/%zu/%zu/%zu; trimmed rows %llu; "
            "launch K%s\n",
            (unsigned long long)head.h, (unsigned long long)wv.h, (unsigned long long)gr.h, groups.size(), fpad[0], fpad[1], fpad[2], fpad[3], trimmed,
            ks.empty() ? " none" : ks.c_str());
}

// the image as the fills read it (the pinned block that is uploaded; plan only: a block built for this line alone)
void trace_band_image(const void *img, size_t bytes, int64_t first_bad)
{
    Fnv1a f;
    f.bytes(img, bytes);
    fprintf(stderr, "[agx_sw_batch_create_band] image digest %016llx, first bad pair %lld\n", (unsigned long long)f.h, (long long)first_bad);
}

// ---- the device side of a create, in the order create_band calls it

// the batch object of a banded create, before its plan: the kind's flags and the kernel constants
agx_sw_batch *init_band_batch(agx_ctx *ctx, const BandKind &kind, const agx_sw_scoring &sc, int64_t n_pairs)
{
    const BandAt *at = kind.at;
    agx_sw_batch *b = new agx_sw_batch();
    agx_ctx_retain(ctx);
    b->ctx = ctx;
    b->n_pairs = n_pairs;
    b->banded = true;
    b->band = kind.band;
    b->cigar = kind.cigar ? 1 : 0;
    b->family = 5;
    b->align = at ? at->what : AGX_SW_ALIGN_SPANS;
    b->band_at = at != nullptr;
    b->zdrop_on = at && at->zdrop_on;
    b->zdrop = b->zdrop_on ? at->zdrop : 0;
    b->stats = at ? at->stats : 0;
    b->mode = kind.mode;
    b->scoring = sc;
    b->matrix = kind.matrix != nullptr;
    if (kind.matrix) b->mat = *kind.matrix;
    b->prm.ge = sc.gap_extend;
    b->prm.gf = sc.gap_open + sc.gap_extend;
    b->prm.hd = sc.match - b->prm.gf;
    b->prm.delta = sc.match - sc.mismatch;
    b->prm.n_out = (uint32_t)n_pairs;
    if (at && at->dual) { // (sc is its first piece: prm, and with it the plan's digest, are the plain batch's)
        b->dual = true;
        b->dual_sc = *at->dual;
        b->dual_gap.ge2 = at->dual->gap_extend2;
        b->dual_gap.dgf = at->dual->gap_open2 + at->dual->gap_extend2 - b->prm.gf;
    }
    return b;
}

// what agx_sw_batch_info answers
void set_band_info(agx_sw_batch *b, int64_t cells, int64_t padded, uint64_t img_dw, size_t n_waves)
{
    b->info.n_pairs = b->n_pairs;
    b->info.cells = cells;
    b->info.padded_cells = padded;
    b->info.input_bytes = (int64_t)(img_dw * 4);
    b->info.n_launches = (int32_t)b->launches.size();
    b->info.n_waves = (int32_t)n_waves;
}

// the whole image into dst, a range of groups per host thread -> the first pair that breaks the symbol rule, or -1
int64_t build_band_image_all(const std::vector<SwBandGroup> &groups, const agx_sw_matrix *matrix, const uint8_t *bases, const uint64_t *off,
                             const uint32_t *len, uint8_t *dst)
{
    std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
    agx_parallel_for((int64_t)groups.size(), 64, [&](int64_t lo, int64_t hi, int t) {
        bad[(size_t)t] = build_band_image(groups, lo, hi, bases, off, len, matrix ? matrix->code : nullptr, dst);
    });
    int64_t first_bad = -1;
    for (int64_t v : bad)
        if (v >= 0 && (first_bad < 0 || v < first_bad)) first_bad = v;
    return first_bad;
}

// What a batch on a device keeps on the host long after the create: the kernels it will launch, loaded now; the lengths; around
// a diagonal the first rows and the centres; the sequences where the begin pass, the traced fills of the spans or the host's
// checks need them; for a cigar batch the group records, every pair's record and its tiling.
void keep_band_host_state(agx_sw_batch *b, const BandKind &kind, const BandPairs &pairs, const std::vector<SwBandGroup> &groups,
                          const uint8_t *bases, const uint64_t *off, const uint32_t *len)
{
    const BandAt *at = kind.at;
    const int64_t n_pairs = b->n_pairs;
    // every row whose needs the batch's kind includes, in the table's order: not its own fill alone
    const unsigned have = (b->band_at ? kSwBandAt : 0u) | (b->zdrop_on ? kSwBandZdrop : 0u) | (b->stats ? kSwBandStats : 0u) |
                          (b->dual ? kSwBandDual : 0u) | (b->matrix ? kSwBandMatrix : 0u) | (b->cigar ? kSwBandTraced : 0u);
    void (*loaded)() = nullptr;
    for (int k = 0; k < kNumBandFills; ++k) {
        const SwBandFill &f = band_fills()[k];
        if ((f.needs & ~have) || f.preload == loaded) continue; // (two rows of one translation unit stand together)
        f.preload();
        loaded = f.preload;
    }
    if (kind.cigar) agx_sw_walk_preload();
    if (n_pairs > 0) b->seq_len.assign(len, len + 2 * n_pairs);
    if (at) {
        b->band_row0 = pairs.row0s;
        if (at->diag) b->band_diag.assign(at->diag, at->diag + n_pairs);
        else b->band_diag.assign((size_t)n_pairs, 0);
    }
    if (kind.cigar || (at && at->what == AGX_SW_ALIGN_SPANS && (kind.mode == AGX_SW_MODE_LOCAL || kind.mode == AGX_SW_MODE_FIT))) {
        b->seq_off.resize((size_t)n_pairs * 2);
        uint64_t at_byte = 0;
        for (int64_t k = 0; k < 2 * n_pairs; ++k) {
            b->seq_off[(size_t)k] = at_byte;
            at_byte += len[k];
        }
        b->seq.resize((size_t)at_byte);
        agx_parallel_for(2 * n_pairs, 8192, [&](int64_t lo, int64_t hi, int) {
            for (int64_t k = lo; k < hi; ++k)
                if (len[k] && bases) memcpy(b->seq.data() + b->seq_off[(size_t)k], bases + off[k], len[k]);
        }); // (bases == NULL: every pair has an empty side, and a lone run of I or D reads no symbol)
    }
    if (!kind.cigar) return;
    const std::vector<BandPlan> &plan = pairs.plan;
    b->band_groups = groups;
    b->band_rec.assign((size_t)n_pairs, kNoBandRec);
    b->band_cls.resize(plan.size());
    b->band_G.resize(plan.size());
    for (size_t k = 0; k < plan.size(); ++k) {
        b->band_rec[plan[k].pair] = (uint32_t)k;
        b->band_cls[k] = plan[k].cls;
        b->band_G[k] = plan[k].G;
    }
}

// The image, built on the host in page-locked memory, and everything a batch with fills has on the device: the records, the
// image, the matrix's table, the results and their landing blocks.  Returns when the copies have landed.  Every exit releases
// the page-locked temporaries, an error exit behind a queued copy only once the copy stream has drained: `drain` does both.
int upload_band(agx_ctx *ctx, agx_sw_batch *b, const BandKind &kind, const std::vector<SwBandGroup> &groups, const std::vector<SwWave> &waves,
                uint64_t img_dw, const std::vector<int16_t> &mat_table, const uint8_t *bases, const uint64_t *off, const uint32_t *len, bool trace)
{
    const size_t img_bytes = (size_t)img_dw * 4, groups_bytes = groups.size() * sizeof(SwBandGroup), waves_bytes = waves.size() * sizeof(SwWave);
    PinBuf h_img, h_groups, h_waves;
    DrainOnError drain(ctx, [&] {
        for (PinBuf *v : {&h_img, &h_groups, &h_waves}) v->release();
    });
    int rc = h_img.alloc(ctx, img_bytes);
    if (!rc) rc = h_groups.alloc(ctx, groups_bytes);
    if (!rc) rc = h_waves.alloc(ctx, waves_bytes);
    if (rc) return rc;
    memcpy(h_groups.p, groups.data(), groups_bytes);
    memcpy(h_waves.p, waves.data(), waves_bytes);
    const int64_t first_bad = build_band_image_all(groups, kind.matrix, bases, off, len, (uint8_t *)h_img.p);
    if (trace) trace_band_image(h_img.p, img_bytes, first_bad);
    if (first_bad >= 0) {
        if (kind.matrix) agx_set_error("pair %lld contains a byte outside the substitution matrix's alphabet", (long long)first_bad);
        else agx_set_error("pair %lld contains byte 0x00, which is reserved as the padding symbol", (long long)first_bad);
        return AGX_E_SYMBOL;
    }
    rc = b->img.alloc(ctx, img_bytes);
    if (!rc && kind.matrix) rc = b->table.alloc(ctx, mat_table.size() * sizeof(int16_t));
    if (!rc) rc = b->groups.alloc(ctx, groups_bytes);
    if (!rc) rc = b->waves.alloc(ctx, waves_bytes);
    if (!rc && b->launches.size() > 1) rc = agx_ctx_prepare_fanout(ctx);
    if (rc) return rc;
    hipStream_t cs = ctx->copy;
    AGX_HIP(hipMemcpyAsync(b->img.p, h_img.p, img_bytes, hipMemcpyHostToDevice, cs));
    AGX_HIP(hipMemcpyAsync(b->groups.p, h_groups.p, groups_bytes, hipMemcpyHostToDevice, cs));
    AGX_HIP(hipMemcpyAsync(b->waves.p, h_waves.p, waves_bytes, hipMemcpyHostToDevice, cs));
    // (pageable: the runtime stages it before the call returns; mat_table outlives the wait below in any case)
    if (kind.matrix) AGX_HIP(hipMemcpyAsync(b->table.p, mat_table.data(), mat_table.size() * sizeof(int16_t), hipMemcpyHostToDevice, cs));
    // results and their landing blocks
    const size_t words = (size_t)b->n_pairs * sizeof(uint32_t);
    rc = b->scores.alloc(ctx, words);
    if (!rc) rc = b->band_pos.alloc(ctx, words);
    if (!rc) rc = b->out_stage.alloc(ctx, words);
    if (!rc) rc = b->band_pos_stage.alloc(ctx, words);
    if (!rc && b->zdrop_on) rc = b->band_stop.alloc(ctx, words);
    if (!rc && b->zdrop_on) rc = b->band_stop_stage.alloc(ctx, words);
    if (!rc && b->stats == 2) rc = b->lstat.alloc(ctx, words);
    if (!rc && b->stats == 2) rc = b->lstat_stage.alloc(ctx, words);
    if (rc) return rc;
    if (b->stats == 2) AGX_HIP(hipMemsetAsync(b->lstat.p, 0, words, cs)); // a pair no wave writes reads {0, 0}
    AGX_HIP(hipStreamSynchronize(cs));
    drain.ok = true;
    return AGX_OK;
}

} // namespace

namespace agx_sw_host {

// The create of every banded batch: the stages of agx_sw_band_plan.cpp and the ones above, top to bottom.
int create_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool cigar, const BandAt *at, const agx_sw_matrix *matrix)
{
    const bool zd = at && at->zdrop_on;
    const char *who = at && at->dual  ? (cigar ? "agx_sw_batch_create_align_band_diag_dual_cigar" : "agx_sw_batch_create_align_band_diag_dual")
                      : at && at->stats ? "agx_sw_batch_create_align_band_diag_stats"
                      : matrix      ? (cigar ? "agx_sw_batch_create_align_band_diag_matrix_cigar" : "agx_sw_batch_create_align_band_diag_matrix")
                      : zd   ? (cigar ? "agx_sw_batch_create_align_band_zdrop_cigar" : "agx_sw_batch_create_align_band_zdrop")
                      : at   ? (cigar ? "agx_sw_batch_create_align_band_diag_cigar" : "agx_sw_batch_create_align_band_diag")
                             : (cigar ? "agx_sw_batch_create_align_band_cigar" : "agx_sw_batch_create_align_band");
    if (!out) {
        agx_set_error("%s: out is NULL", who);
        return AGX_E_ARG;
    }
    *out = nullptr;
    const BandKind kind{mode, band, cigar, at, matrix, who};
    // under a matrix (a batch around a diagonal without z-drop only: the entry points see to that) it is validated before anything
    // else that can fail; scoring is then its gaps around a match/mismatch pair that nothing reads
    agx_sw_scoring mat_sc{}, sc{};
    SwParams mat_prm{};
    std::vector<int16_t> mat_table;
    int rc = matrix ? matrix_constants(matrix, mat_sc, mat_prm, mat_table) : AGX_OK;
    if (rc) return rc;
    if ((rc = check_band_kind(kind))) return rc;
    // ctx == NULL: plan only (no device needed) -- the batch answers agx_sw_batch_info() and nothing else
    if ((rc = ctx ? agx_bind(ctx) : AGX_OK)) return rc;
    if ((rc = check_band_arrays(kind, matrix ? &mat_sc : scoring, off, len, n_pairs, sc))) return rc;

    // ---- the plan: per pair, sorted, in waves, as records
    BandPairs pairs;
    if ((rc = plan_band_pairs(kind, bases, len, n_pairs, pairs))) return rc;
    sort_band_plan(pairs.plan);
    std::vector<SwWave> waves;
    std::vector<ClassLaunch> launches;
    const int64_t padded = layout_band_waves(pairs.plan, waves, launches);
    std::vector<SwBandGroup> groups;
    uint64_t img_dw = 0;
    if ((rc = write_band_groups(pairs.plan, groups, img_dw))) return rc;

    // ---- the batch.  Every exit from here: on an error the copy stream drained (upload_band has seen to its own temporaries),
    // then the half-built batch destroyed
    agx_sw_batch *b = init_band_batch(ctx, kind, sc, n_pairs);
    DrainOnError done(ctx, [&] { agx_sw_batch_destroy(b); });
    b->launches = launches;
    set_band_info(b, pairs.cells, padded, img_dw, waves.size());
    const bool trace = agx_tune("AGX_TRACE_CREATE") != nullptr;
    if (trace) trace_band_plan(b, waves, groups, pairs.row0s, at ? at->diag : nullptr, len);
    if (ctx) {
        keep_band_host_state(b, kind, pairs, groups, bases, off, len);
        if (!groups.empty() && (rc = upload_band(ctx, b, kind, groups, waves, img_dw, mat_table, bases, off, len, trace))) return rc;
        if (groups.empty() && trace) trace_band_image(nullptr, 0, -1);
    } else if (trace) { // plan only: no image and no symbol check, but for the image digest
        std::vector<uint8_t> im((size_t)img_dw * 4);
        trace_band_image(im.data(), im.size(), groups.empty() ? -1 : build_band_image_all(groups, matrix, bases, off, len, im.data()));
    }
    *out = b;
    b = nullptr;
    done.ok = true;
    return AGX_OK;
}

// ---- the selection table: one row per fill kernel of the banded family, in the order a create preloads them
// (keep_band_host_state).  band_fill picks a batch's row; band_launch and band_trace (agx_sw_cigar.cpp) launch through it.
enum { kFillPlain, kFillMat, kFillAt, kFillZd, kFillStats, kFillDual, kFillDualAt, kFillTrace, kFillTraceAt, kFillTraceDual, kFillTraceMat };
const SwBandFill *band_fills()
{
    static const SwBandFill rows[kNumBandFills] = {
        {"sw_fill_band", false, 0, agx_sw_band_launch, agx_sw_band_preload, nullptr},
        {"sw_fill_band_mat", true, kSwBandMatrix, agx_sw_band_mat_launch, agx_sw_band_mat_preload, nullptr},
        {"sw_fill_band_at", true, kSwBandAt, agx_sw_band_at_launch, agx_sw_band_at_preload, nullptr},
        {"sw_fill_band_zd", false, kSwBandZdrop, agx_sw_band_zdrop_launch, agx_sw_band_zdrop_preload, nullptr},
        {"sw_fill_band_stats", true, kSwBandStats, agx_sw_band_stats_launch, agx_sw_band_stats_preload, nullptr},
        {"sw_fill_band_dual", false, kSwBandDual, agx_sw_band_dual_launch, agx_sw_band_dual_preload, nullptr},
        {"sw_fill_band_dual_at", true, kSwBandDual, agx_sw_band_dual_launch, agx_sw_band_dual_preload, nullptr},
        {"sw_fill_band_trace", false, kSwBandTraced, agx_sw_band_trace_launch, agx_sw_band_trace_preload, agx_sw_band_walk_launch},
        {"sw_fill_band_trace_at", false, kSwBandTraced | kSwBandAt, agx_sw_band_trace_at_launch, agx_sw_band_trace_at_preload, agx_sw_band_walk_at_launch},
        {"sw_fill_band_trace_dual", false, kSwBandTraced | kSwBandDual, agx_sw_band_trace_dual_launch, agx_sw_band_trace_dual_preload,
         agx_sw_band_walk_dual_launch},
        // (a batch under a matrix is banded around a diagonal: its spans run the traced build with the start phase, and that walk)
        {"sw_fill_band_trace_mat", false, kSwBandTraced | kSwBandMatrix, agx_sw_band_trace_mat_launch, agx_sw_band_trace_mat_preload,
         agx_sw_band_walk_at_launch},
    };
    return rows;
}

const SwBandFill &band_fill(const agx_sw_batch *b, bool traced)
{
    if (traced) return band_fills()[b->dual ? kFillTraceDual : b->matrix ? kFillTraceMat : b->band_at ? kFillTraceAt : kFillTrace];
    // GLOBAL and EXTEND around a diagonal run the builds around the main one: their boundaries and captures are the same
    const bool at = b->band_at && b->mode != AGX_SW_MODE_GLOBAL && b->mode != AGX_SW_MODE_EXTEND;
    return band_fills()[b->dual         ? (at ? kFillDualAt : kFillDual)
                      : b->stats == 2 ? kFillStats
                      : b->zdrop_on   ? kFillZd
                      : b->matrix     ? kFillMat
                      : at            ? kFillAt
                                      : kFillPlain];
}

int band_fill_failed(const SwBandFill &f, int K, int mode)
{
    if (f.per_mode) agx_set_error("%s<%d, %d> launch failed: %s", f.name, K, mode, hipGetErrorString(hipGetLastError()));
    else agx_set_error("%s<%d> launch failed: %s", f.name, K, hipGetErrorString(hipGetLastError()));
    return AGX_E_HIP;
}

int band_launch(agx_sw_batch *b)
{
    b->cig_valid = false; // what agx_sw_batch_cigars kept belongs to the launch before
    if (b->launches.empty()) return AGX_OK;
    const SwBandFill &fill = band_fill(b, false);
    SwBandArgs a{};
    a.prm = b->prm;
    a.dual_gap = b->dual_gap;
    a.img = (const uint32_t *)b->img.p;
    a.groups = (const SwBandGroup *)b->groups.p;
    a.scores = (int32_t *)b->scores.p;
    a.pos = (uint32_t *)b->band_pos.p;
    a.zdrop = b->zdrop;
    a.stops = (int32_t *)b->band_stop.p;
    a.lstat = (uint32_t *)b->lstat.p;
    a.table = (const int16_t *)b->table.p;
    FanOut fan(b->ctx, (int)b->launches.size());
    int rc = fan.begin();
    if (rc) return rc;
    int k = 0;
    // widest class first: its waves have the longest steps
    for (auto it = b->launches.rbegin(); it != b->launches.rend(); ++it) {
        a.waves = (const SwWave *)b->waves.p + it->first_wave;
        a.n_waves = it->n_waves;
        if (fill.launch(it->C, b->mode, a, fan.stream(k++))) return band_fill_failed(fill, it->C, b->mode);
    }
    return fan.end();
}

// band_hits of a batch around a diagonal (include/agx.h, "Banded alignment around a diagonal"): the fill's rows are counted from
// the pair's first row; every reported cell is checked against the matrix and the band.  begins: run the begin pass of a SPANS
// batch in LOCAL and FIT (agx_sw_batch_scores does not need it) -- a second batch of the same kind over the reversed prefixes,
// whose band is the mirror image of the pair's: reversed, cell (i, j) of the span of cb rows and ca columns is (cb - i, ca - j),
// so diagonal d becomes ca - cb - d and the centre c becomes ca - cb - c, the half-width stays.
// L: also every pair's word matches << kSwBandStatBits | pairs -- from this batch's own fill (stats == 2), else from the begin pass,
// which then runs the stats builds; 0 for the pairs answered without a fill and for those whose alignment consumes nothing
int band_at_hits(agx_sw_batch *b, agx_sw_hit *hits, bool begins, std::vector<uint32_t> *L)
{
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    hipStream_t st = agx_enqueue_stream(b->ctx);
    const int64_t n = b->n_pairs;
    const int mode = b->mode;
    const bool cell = mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_EXTEND, column = mode == AGX_SW_MODE_FIT || mode == AGX_SW_MODE_EXTEND_QUERY;
    if (!b->launches.empty()) {
        AGX_HIP(hipMemcpyAsync(b->out_stage.p, b->scores.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (cell || column) AGX_HIP(hipMemcpyAsync(b->band_pos_stage.p, b->band_pos.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    const bool own_l = L && b->stats == 2 && !b->launches.empty();
    if (own_l) AGX_HIP(hipMemcpyAsync(b->lstat_stage.p, b->lstat.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    AGX_HIP(hipStreamSynchronize(st));
    if (own_l) L->assign((const uint32_t *)b->lstat_stage.p, (const uint32_t *)b->lstat_stage.p + n);
    else if (L) L->assign((size_t)n, 0u);
    const int32_t *sc = (const int32_t *)b->out_stage.p;
    const uint32_t *ps = (const uint32_t *)b->band_pos_stage.p;
    const bool spans = b->align == AGX_SW_ALIGN_SPANS;
    const agx_sw_hit nothing{0, -1, -1, -1, -1};
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t la = b->seq_len[(size_t)(2 * p)], lb = b->seq_len[(size_t)(2 * p + 1)];
        const uint32_t row0 = b->band_row0[(size_t)p];
        if (!la || !lb) {
            hits[p] = mode == AGX_SW_MODE_LOCAL ? nothing
                      : b->dual                 ? empty_side_hit_dual(mode, b->align, b->dual_sc, la, lb)
                                                : empty_side_hit(mode, b->align, b->scoring, la, lb);
            continue;
        }
        if (row0 == kNoBandRow) { // LOCAL: the band misses the matrix
            hits[p] = nothing;
            continue;
        }
        const int64_t dlo = (int64_t)b->band_diag[(size_t)p] - b->band, dhi = (int64_t)b->band_diag[(size_t)p] + b->band;
        agx_sw_hit h{sc[p], -1, (int32_t)la - 1, -1, (int32_t)lb - 1};
        int64_t i = lb, j = la;
        bool ok = true, consumed = true;
        if (cell) {
            if (h.score <= 0) {
                ok = h.score == 0;
                h = nothing;
                consumed = false;
            } else {
                i = (int64_t)(ps[p] >> 16) + row0;
                j = ps[p] & 0xffffu;
                // (0xffffffff, the word of a pair without a hit, is also cell (65535, 65535): with a score it is that cell, and the
                // test below holds it against the matrix and the band like any other)
                ok = i >= 1 && j >= 1;
            }
        } else if (column) {
            i = (int64_t)ps[p] + row0;
            ok = ps[p] <= 0xffffu;
        }
        if (consumed) {
            if (!ok || i > lb || j > la || j - i < dlo || j - i > dhi) {
                agx_set_error("agx_sw_batch_hits: pair %lld (mode %d, diag %d, band %d): score %d with end cell word 0x%08x is not an in-band cell of its "
                              "%u x %u matrix",
                              (long long)p, mode, b->band_diag[(size_t)p], b->band, sc[p], cell || column ? ps[p] : 0u, lb, la);
                return AGX_E_INTERNAL;
            }
            h.b_end = (int32_t)i - 1;
            h.a_end = (int32_t)j - 1;
            if (spans && mode != AGX_SW_MODE_LOCAL) h.a_begin = h.b_begin = 0; // (FIT: b_begin follows below)
        } else if (!ok) {
            agx_set_error("agx_sw_batch_hits: pair %lld (mode %d): the banded fill gives the negative score %d", (long long)p, mode, sc[p]);
            return AGX_E_INTERNAL;
        }
        hits[p] = h;
    }
    if (!begins || !spans || (mode != AGX_SW_MODE_LOCAL && mode != AGX_SW_MODE_FIT)) return AGX_OK;
    const bool fit = mode == AGX_SW_MODE_FIT;

    // ---- begin pass.  LOCAL: the pairs with a score; FIT: those that consume some of b.
    RevPrefixes rev;
    reversed_prefixes(b, hits, fit, 64, rev);
    const std::vector<int64_t> &pick = rev.pick;
    const int64_t m = (int64_t)pick.size();
    if (m == 0) return AGX_OK;
    std::vector<int32_t> rdiag((size_t)m);
    for (int64_t k = 0; k < m; ++k) {
        const agx_sw_hit &h = hits[pick[(size_t)k]];
        rdiag[(size_t)k] = (h.a_end + 1) - (h.b_end + 1) - b->band_diag[(size_t)pick[(size_t)k]];
    }
    agx_sw_batch *rb = nullptr;
    const BandAt rat{AGX_SW_ALIGN_ENDS, rdiag.data(), false, 0, L ? 2 : 0, b->dual ? &b->dual_sc : nullptr}; // (under the same two pieces)
    rc = create_band(b->ctx, &b->scoring, fit ? AGX_SW_MODE_EXTEND_QUERY : AGX_SW_MODE_LOCAL, b->band, rev.bytes.data(), rev.off.data(),
                     rev.len.data(), m, &rb, false, &rat, b->matrix ? &b->mat : nullptr);
    if (rc) return rc;
    struct Drop {
        agx_sw_batch *b;
        ~Drop()
        {
            (void)hipStreamSynchronize(b->ctx->stream); // an error exit may leave its fill running
            agx_sw_batch_destroy(b);
        }
    } drop{rb};
    std::vector<agx_sw_hit> rh((size_t)m);
    std::vector<uint32_t> rl;
    rc = agx_sw_batch_launch(rb);
    if (!rc) rc = band_at_hits(rb, rh.data(), false, L ? &rl : nullptr);
    if (rc) return rc;
    for (int64_t k = 0; k < m; ++k) {
        agx_sw_hit &h = hits[pick[(size_t)k]];
        const agx_sw_hit &r = rh[(size_t)k];
        // (FIT: the reverse fill may consume nothing of b -- all of a in one gap along row b_end + 1 -- which is b_begin = b_end + 1)
        if (r.score != h.score || r.a_end > h.a_end || r.b_end > h.b_end || (fit ? r.a_end != h.a_end || r.b_end < -1 : r.a_end < 0 || r.b_end < 0)) {
            agx_set_error("agx_sw_batch_hits: pair %lld: the reverse banded fill from its end cell (a %d, b %d) gives score %d at (a %d, b %d), the forward "
                          "fill %d",
                          (long long)pick[(size_t)k], h.a_end, h.b_end, r.score, r.a_end, r.b_end, h.score);
            return AGX_E_INTERNAL;
        }
        if (!fit) h.a_begin = h.a_end - r.a_end;
        h.b_begin = h.b_end - r.b_end;
        if (L) (*L)[(size_t)pick[(size_t)k]] = rl[(size_t)k];
    }
    return AGX_OK;
}

// the stops of a z-drop batch (include/agx.h, "Z-drop for banded extension"): waits like band_at_hits, -1 for the pairs answered
// without a fill; every stop is checked against its pair's rows and end cell
int band_zdrop_stops(agx_sw_batch *b, int32_t *stops)
{
    const int64_t n = b->n_pairs;
    std::vector<agx_sw_hit> hits((size_t)n);
    int rc = band_at_hits(b, hits.data(), false);
    if (rc) return rc;
    hipStream_t st = agx_enqueue_stream(b->ctx);
    if (!b->launches.empty()) {
        AGX_HIP(hipMemcpyAsync(b->band_stop_stage.p, b->band_stop.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AGX_HIP(hipStreamSynchronize(st));
    }
    const int32_t *sp = (const int32_t *)b->band_stop_stage.p;
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t lb = b->seq_len[(size_t)(2 * p + 1)];
        if (b->band_row0[(size_t)p] == kNoBandRow) { // an empty side: no fill
            stops[p] = -1;
            continue;
        }
        const int32_t s = sp[p];
        if (s < -1 || s >= (int64_t)lb || (s >= 0 && s < hits[(size_t)p].b_end)) {
            agx_set_error("agx_sw_batch_zdrop_stops: pair %lld (diag %d, band %d, zdrop %d): stop %d does not lie in -1 .. %u or lies before b_end = %d",
                          (long long)p, b->band_diag[(size_t)p], b->band, b->zdrop, s, lb, hits[(size_t)p].b_end);
            return AGX_E_INTERNAL;
        }
        stops[p] = s;
    }
    return AGX_OK;
}

// waits for the launched fill and builds the hits by the contract's rules, in the caller's pair order
int band_hits(agx_sw_batch *b, agx_sw_hit *hits)
{
    if (b->band_at) return band_at_hits(b, hits, true);
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    hipStream_t st = agx_enqueue_stream(b->ctx);
    const int64_t n = b->n_pairs;
    const bool filled = !b->launches.empty();
    if (filled) {
        AGX_HIP(hipMemcpyAsync(b->out_stage.p, b->scores.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (b->mode == AGX_SW_MODE_EXTEND)
            AGX_HIP(hipMemcpyAsync(b->band_pos_stage.p, b->band_pos.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    AGX_HIP(hipStreamSynchronize(st));
    const int32_t *sc = (const int32_t *)b->out_stage.p;
    const uint32_t *ps = (const uint32_t *)b->band_pos_stage.p;
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t la = b->seq_len[(size_t)(2 * p)], lb = b->seq_len[(size_t)(2 * p + 1)];
        if (!la || !lb) {
            hits[p] = empty_side_hit(b->mode, AGX_SW_ALIGN_SPANS, b->scoring, la, lb);
            continue;
        }
        agx_sw_hit h{sc[p], 0, (int32_t)la - 1, 0, (int32_t)lb - 1};
        if (b->mode == AGX_SW_MODE_EXTEND) {
            if (h.score <= 0)
                h = agx_sw_hit{0, -1, -1, -1, -1};
            else {
                const uint32_t i = ps[p] >> 16, j = ps[p] & 0xffffu;
                if (i < 1 || i > lb || j < 1 || j > la) {
                    agx_set_error("pair %lld: the banded fill reported the end cell (%u, %u) outside the %u x %u matrix", (long long)p, i, j, lb, la);
                    return AGX_E_INTERNAL;
                }
                h.b_end = (int32_t)i - 1;
                h.a_end = (int32_t)j - 1;
            }
        }
        hits[p] = h;
    }
    return AGX_OK;
}

} // namespace agx_sw_host

extern "C" {

int agx_sw_batch_create_align_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases,
                                   const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out);
    AGX_GUARD_END("agx_sw_batch_create_align_band")
}

int agx_sw_align_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                      const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band(ctx, scoring, mode, band, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_batch_create_align_band_diag(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag,
                                        const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    const BandAt at{what, diag};
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, false, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag")
}

int agx_sw_align_band_diag(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag, const uint8_t *bases,
                           const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag(ctx, scoring, mode, what, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_batch_create_align_band_diag_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                              const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    // LOCAL and FIT keep the plain forward fill (their begin pass carries L), the pinned modes' only fill carries it
    const BandAt at{AGX_SW_ALIGN_SPANS, diag, false, 0, mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_FIT ? 1 : 2};
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, false, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_stats")
}

int agx_sw_align_band_diag_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag, const uint8_t *bases,
                                 const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, agx_sw_stat *stats)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_stats(ctx, scoring, mode, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_stats(x, hits, stats); });
}

int agx_sw_batch_create_align_band_diag_dual(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int what, int32_t band,
                                             const int32_t *diag, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                             agx_sw_batch **out)
{
    if (!scoring) { // (there is no reference default for a second piece)
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_band_diag_dual: scoring is NULL");
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    const BandAt at{what, diag, false, 0, 0, scoring};
    const agx_sw_scoring piece1{scoring->match, scoring->mismatch, scoring->gap_open, scoring->gap_extend};
    return create_band(ctx, &piece1, mode, band, bases, off, len, n_pairs, out, false, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_dual")
}

int agx_sw_align_band_diag_dual(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int what, int32_t band, const int32_t *diag,
                                const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_dual(ctx, scoring, mode, what, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_batch_create_align_band_diag_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, int32_t band, const int32_t *diag,
                                               const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    if (!matrix) {
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_band_diag_matrix: matrix is NULL");
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    const BandAt at{what, diag};
    return create_band(ctx, nullptr, mode, band, bases, off, len, n_pairs, out, false, &at, matrix);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_matrix")
}

int agx_sw_align_band_diag_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, int32_t band, const int32_t *diag,
                                  const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_matrix(ctx, matrix, mode, what, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_batch_create_align_band_zdrop(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag,
                                         int32_t zdrop, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                         agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    const BandAt at{what, diag, true, zdrop};
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, false, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_zdrop")
}

int agx_sw_batch_zdrop_stops(agx_sw_batch *b, int32_t *stops)
{
    if (!b || (!stops && b->n_pairs)) {
        agx_set_error("agx_sw_batch_zdrop_stops: null argument");
        return AGX_E_ARG;
    }
    if (!b->zdrop_on) {
        agx_set_error("agx_sw_batch_zdrop_stops: not a z-drop batch (create it with agx_sw_batch_create_align_band_zdrop or "
                      "agx_sw_batch_create_align_band_zdrop_cigar)");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no stops");
        return AGX_E_NODEVICE;
    }
    AGX_GUARD_BEGIN
    return band_zdrop_stops(b, stops);
    AGX_GUARD_END("agx_sw_batch_zdrop_stops")
}

int agx_sw_align_band_zdrop(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, int32_t band, const int32_t *diag, int32_t zdrop,
                            const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, int32_t *stops)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_zdrop(ctx, scoring, mode, what, band, diag, zdrop, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) {
        const int r = agx_sw_batch_hits(x, hits);
        return r || !stops ? r : agx_sw_batch_zdrop_stops(x, stops);
    });
}

} // extern "C"
