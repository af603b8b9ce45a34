// ------------------------------------------------------------------ banded batches (include/agx.h, "Banded alignment")
// Their plan and create (around the main diagonal or a given one), launch and hits; the CIGARs of banded batches are in
// agx_sw_cigar.cpp.
#include "agx_sw_batch.h"

#include "agx_parallel.h"

using namespace agx_sw_host;

namespace {

// Lane tiling of a band of `width` diagonals over lb rows: K diagonals per lane, G = ceil(width / K) lanes per group, 64 / G
// groups per wave.  A wave step costs about kBandStepCells cells' worth of instructions besides its K cells (the exchanges, the
// cell mask, the window shift, the loop: counted in the K = 8 disassembly) and a group runs lb + G steps; the
// class with the least lane time per pair wins, ties go to the wider one (fewer steps).
constexpr int kBandStepCells = 5;
inline void band_tiling(int width, uint32_t lb, int &cls, int &G)
{
    double best = 0;
    cls = -1;
    for (int c = kSwNumBandClasses - 1; c >= 0; --c) {
        const int K = kSwBandClasses[c], g = (width + K - 1) / K;
        if (g > 64) continue;
        const double cost = ((double)lb + g) * (kBandStepCells + K) / (double)(64 / g);
        if (cls < 0 || cost < best) {
            best = cost;
            cls = c;
            G = g;
        }
    }
}

struct BandPlan { // one pair with work, as the sort moves it
    uint32_t pair, la, lb;
    int32_t dlo, dhi;
    uint8_t cls, G;
    uint32_t row0; // a band around a diagonal: the fill is given b[row0 .. row0 + lb) and the band shifted by row0; else 0
};

// What the band dlo .. dhi must hold in `mode` (include/agx.h, "Banded alignment around a diagonal"): nullptr if it does, else
// the words of the error message.
inline const char *band_at_condition(int mode, int64_t la, int64_t lb, int64_t dlo, int64_t dhi)
{
    const bool origin = dlo <= 0 && 0 <= dhi;
    switch (mode) {
    case AGX_SW_MODE_GLOBAL:
        if (!origin) return "does not hold the origin (diagonal 0)";
        return dlo <= la - lb && la - lb <= dhi ? nullptr : "does not hold the corner (diagonal la - lb)";
    case AGX_SW_MODE_EXTEND: return origin ? nullptr : "does not hold the origin (diagonal 0)";
    case AGX_SW_MODE_EXTEND_QUERY:
        if (!origin) return "does not hold the origin (diagonal 0)";
        return dhi >= la - lb ? nullptr : "holds no cell of column la (dhi < la - lb)";
    case AGX_SW_MODE_FIT:
        if (dlo > 0) return "holds no cell of column 0 (dlo > 0)";
        return dhi >= la - lb ? nullptr : "holds no cell of column la (dhi < la - lb)";
    default: return nullptr; // LOCAL: a band that misses the matrix scores 0
    }
}

} // namespace

namespace agx_sw_host {

int create_band(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool cigar, const BandAt *at, const agx_sw_matrix *matrix)
{
    const bool zd = at && at->zdrop_on;
    const char *who = matrix ? (cigar ? "agx_sw_batch_create_align_band_diag_matrix_cigar" : "agx_sw_batch_create_align_band_diag_matrix")
                      : zd   ? (cigar ? "agx_sw_batch_create_align_band_zdrop_cigar" : "agx_sw_batch_create_align_band_zdrop")
                      : at   ? (cigar ? "agx_sw_batch_create_align_band_diag_cigar" : "agx_sw_batch_create_align_band_diag")
                             : (cigar ? "agx_sw_batch_create_align_band_cigar" : "agx_sw_batch_create_align_band");
    if (!out) {
        agx_set_error("%s: out is NULL", who);
        return AGX_E_ARG;
    }
    *out = nullptr;
    // under a matrix (a batch around a diagonal without z-drop only: the entry points see to that) it is validated before anything
    // else that can fail; scoring is then its gaps around a match/mismatch pair that nothing reads
    agx_sw_scoring mat_sc{};
    SwParams mat_prm{};
    std::vector<int16_t> mat_table;
    if (matrix) {
        const int mrc = matrix_constants(matrix, mat_sc, mat_prm, mat_table);
        if (mrc) return mrc;
        scoring = &mat_sc;
    }
    if (mode < AGX_SW_MODE_LOCAL || mode > AGX_SW_MODE_EXTEND_QUERY) {
        agx_set_error("%s: mode = %d is not one of AGX_SW_MODE_LOCAL .. AGX_SW_MODE_EXTEND_QUERY (0..4)", who, mode);
        return AGX_E_ARG;
    }
    if (at && at->what != AGX_SW_ALIGN_ENDS && at->what != AGX_SW_ALIGN_SPANS) {
        agx_set_error("%s: what = %d is neither AGX_SW_ALIGN_ENDS nor AGX_SW_ALIGN_SPANS", who, at->what);
        return AGX_E_ARG;
    }
    if (!at && mode != AGX_SW_MODE_GLOBAL && mode != AGX_SW_MODE_EXTEND) {
        agx_set_error("%s: mode = %d has a free start or a column capture; a band around the main diagonal serves AGX_SW_MODE_GLOBAL and "
                      "AGX_SW_MODE_EXTEND only",
                      who, mode);
        return AGX_E_ARG;
    }
    if (zd && mode != AGX_SW_MODE_EXTEND) {
        agx_set_error("%s: mode = %d: a z-drop terminates an extension, AGX_SW_MODE_EXTEND only", who, mode);
        return AGX_E_ARG;
    }
    if (zd && (at->zdrop < 0 || at->zdrop > AGX_SW_ZDROP_MAX)) {
        agx_set_error("%s: zdrop = %d is outside 0 .. AGX_SW_ZDROP_MAX (%d)", who, at->zdrop, AGX_SW_ZDROP_MAX);
        return AGX_E_ARG;
    }
    if (band < 0) {
        agx_set_error("%s: band = %d is negative", who, band);
        return AGX_E_ARG;
    }
    if (at && 2 * (int64_t)band + 1 > AGX_SW_BAND_MAX_WIDTH) {
        agx_set_error("%s: band = %d needs %lld diagonals, supported %d", who, band, 2 * (long long)band + 1, AGX_SW_BAND_MAX_WIDTH);
        return AGX_E_LIMIT;
    }
    int rc = ctx ? agx_bind(ctx) : AGX_OK;
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !len))) {
        agx_set_error("%s: bad arguments (n_pairs=%lld)", who, (long long)n_pairs);
        return AGX_E_ARG;
    }
    if (n_pairs > 0x7fffffffLL / 2) {
        agx_set_error("%s: more than 2^30 pairs in one batch", who);
        return AGX_E_LIMIT;
    }
    const agx_sw_scoring ref_scoring = AGX_SW_SCORING_REFERENCE;
    const agx_sw_scoring sc = scoring ? *scoring : ref_scoring;
    if (sc.match < 1 || sc.match > 12 || sc.mismatch > 0 || sc.mismatch < sc.match - 128 || sc.gap_open > 0 || sc.gap_open < -1000 ||
        sc.gap_extend > 0 || sc.gap_extend < -1000) {
        agx_set_error("scoring {match %d, mismatch %d, open %d, extend %d} outside the supported range", sc.match, sc.mismatch, sc.gap_open,
                      sc.gap_extend);
        return AGX_E_LIMIT;
    }

    // ---- pass A: limits, band, lane tiling
    std::vector<BandPlan> plan;
    std::vector<uint32_t> row0s; // (at) per pair, for the batch
    if (at) row0s.assign((size_t)n_pairs, kNoBandRow);
    int64_t cells = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const uint32_t la = len[2 * p], lb = len[2 * p + 1];
        if (la > (uint32_t)AGX_SW_BAND_MAX_LEN || lb > (uint32_t)AGX_SW_BAND_MAX_LEN) {
            agx_set_error("pair %lld: lengths %u x %u exceed the supported %d on either side of a banded batch", (long long)p, la, lb,
                          AGX_SW_BAND_MAX_LEN);
            return AGX_E_LIMIT;
        }
        int64_t dlo, dhi, row0 = 0, rows = lb;
        if (at) {
            // exactly c - w .. c + w, never widened.  The band touches the rows max(0, -dhi) .. min(lb, la - dlo) only: the fill is
            // given those rows of b and the band shifted by the first.  The shifted problem has the same boundary values: the
            // pinned modes hold the origin, so their first row is 0; in FIT and LOCAL a first row > 0 means dhi < 0, the row above
            // it holds no in-band cell with j >= 0, and the only in-band cell of the first row is (row0, 0), whose value (0) is
            // what the fill gives the origin of its own matrix.
            const int64_t c = at->diag ? at->diag[p] : 0;
            if (c > (int64_t)AGX_SW_BAND_MAX_LEN + band || -c > (int64_t)AGX_SW_BAND_MAX_LEN + band) {
                agx_set_error("pair %lld: diag = %lld lies beyond the supported %d + band on either side", (long long)p, (long long)c, AGX_SW_BAND_MAX_LEN);
                return AGX_E_ARG;
            }
            dlo = c - band;
            dhi = c + band;
            if (const char *why = band_at_condition(mode, la, lb, dlo, dhi)) {
                agx_set_error("pair %lld: lengths %u x %u in mode %d: the band %lld .. %lld (diag %lld, band %d) %s", (long long)p, la, lb, mode,
                              (long long)dlo, (long long)dhi, (long long)c, band, why);
                return AGX_E_ARG;
            }
            if (mode == AGX_SW_MODE_LOCAL && (dlo > (int64_t)la - 1 || dhi < 1 - (int64_t)lb)) { // no in-band cell with i, j >= 1: scores 0
                cells += (int64_t)la * lb;
                continue;
            }
            row0 = std::max<int64_t>(0, -dhi);
            rows = std::min<int64_t>(lb, (int64_t)la - dlo) - row0;
            dlo += row0;
            dhi += row0;
        } else
            band_limits(mode, band, la, lb, dlo, dhi);
        if (dhi - dlo + 1 > AGX_SW_BAND_MAX_WIDTH) {
            agx_set_error("pair %lld: lengths %u x %u at band %d need %lld diagonals, supported %d", (long long)p, la, lb, band,
                          (long long)(dhi - dlo + 1), AGX_SW_BAND_MAX_WIDTH);
            return AGX_E_LIMIT;
        }
        cells += (int64_t)la * lb;
        if (!la || !lb) continue; // answered by the formulas
        if (!bases) {
            agx_set_error("%s: bases is NULL", who);
            return AGX_E_ARG;
        }
        BandPlan e{(uint32_t)p, la, (uint32_t)rows, (int32_t)dlo, (int32_t)dhi, 0, 0, (uint32_t)row0};
        if (at) row0s[(size_t)p] = (uint32_t)row0;
        int cls = 0, G = 1;
        band_tiling((int)(dhi - dlo + 1), e.lb, cls, G);
        e.cls = (uint8_t)cls;
        e.G = (uint8_t)G;
        plan.push_back(e);
    }
    // ---- sort: class, lanes per group, then rows falling -- the groups of a wave step alike (lb + G)
    std::sort(plan.begin(), plan.end(), [](const BandPlan &x, const BandPlan &y) {
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.G != y.G) return x.G < y.G;
        if (x.lb != y.lb) return x.lb > y.lb;
        return x.pair < y.pair;
    });
    // ---- waves, group records, image offsets
    const size_t n_fill = plan.size();
    std::vector<SwBandGroup> groups(n_fill);
    std::vector<SwWave> waves;
    std::vector<ClassLaunch> launches;
    uint64_t img_dw = 0;
    int64_t padded = 0;
    for (size_t k = 0; k < n_fill;) {
        const BandPlan &h = plan[k];
        const int K = kSwBandClasses[h.cls], G = h.G, per_wave = 64 / G;
        size_t end = k;
        while (end < n_fill && end - k < (size_t)per_wave && plan[end].cls == h.cls && plan[end].G == h.G) ++end;
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
        for (; k < end; ++k) {
            const BandPlan &e = plan[k];
            SwBandGroup &g = groups[k];
            const int q0 = e.dlo + G * K - G;
            g.fpad = (uint32_t)(((-q0) % 4 + 4) % 4);
            g.x_dw = (uint32_t)img_dw;
            img_dw += (g.fpad + e.la + 3) / 4 + 1;
            g.y_dw = (uint32_t)img_dw;
            img_dw += (e.lb + 4) / 4 + 1;
            g.la_lb = e.la | e.lb << 16;
            g.dlo = e.dlo;
            g.dhi = e.dhi;
            g.out = e.pair;
            g.reserved = e.row0; // (the kernels do not read it: the image build below does)
            if (img_dw > 0xffffffffull) {
                agx_set_error("pair %u: the batch's sequences exceed the 16 GiB a banded batch's image may take", e.pair);
                return AGX_E_LIMIT;
            }
        }
    }

    agx_sw_batch *b = new agx_sw_batch();
    DrainOnError done(ctx, [&] { agx_sw_batch_destroy(b); }); // (an error exit behind a queued copy drains the copy stream first)
    agx_ctx_retain(ctx);
    b->ctx = ctx;
    b->n_pairs = n_pairs;
    b->banded = true;
    b->band = band;
    b->cigar = cigar ? 1 : 0;
    b->family = 5;
    b->align = at ? at->what : AGX_SW_ALIGN_SPANS;
    b->band_at = at != nullptr;
    b->zdrop_on = zd;
    b->zdrop = zd ? at->zdrop : 0;
    b->mode = mode;
    b->scoring = sc;
    b->matrix = matrix != nullptr;
    if (matrix) b->mat = *matrix;
    b->prm.ge = sc.gap_extend;
    b->prm.gf = sc.gap_open + sc.gap_extend;
    b->prm.hd = sc.match - b->prm.gf;
    b->prm.delta = sc.match - sc.mismatch;
    b->prm.n_out = (uint32_t)n_pairs;
    b->launches = launches;
    b->info.n_pairs = n_pairs;
    b->info.cells = cells;
    b->info.padded_cells = padded;
    b->info.input_bytes = (int64_t)(img_dw * 4);
    b->info.n_launches = (int32_t)launches.size();
    b->info.n_waves = (int32_t)waves.size();
    if (!ctx) {
        *out = b;
        b = nullptr;
        done.ok = true;
        return AGX_OK;
    }
    agx_sw_band_preload();
    if (n_pairs > 0) b->seq_len.assign(len, len + 2 * n_pairs);
    if (matrix) agx_sw_band_mat_preload();
    if (at) {
        agx_sw_band_at_preload();
        if (zd) agx_sw_band_zdrop_preload();
        b->band_row0 = row0s;
        if (at->diag) b->band_diag.assign(at->diag, at->diag + n_pairs);
        else b->band_diag.assign((size_t)n_pairs, 0);
    }
    if (cigar || (at && at->what == AGX_SW_ALIGN_SPANS && (mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_FIT))) {
        // what the traced fills of the spans and the host's checks, or the begin pass, need long after this call
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
    if (cigar) {
        agx_sw_band_trace_preload();
        if (at) agx_sw_band_trace_at_preload();
        if (matrix) agx_sw_band_trace_mat_preload();
        agx_sw_walk_preload();
        b->band_groups = groups;
        b->band_rec.assign((size_t)n_pairs, kNoBandRec);
        b->band_cls.resize(n_fill);
        b->band_G.resize(n_fill);
        for (size_t k = 0; k < n_fill; ++k) {
            b->band_rec[plan[k].pair] = (uint32_t)k;
            b->band_cls[k] = plan[k].cls;
            b->band_G[k] = plan[k].G;
        }
    }
    PinBuf h_img, h_groups, h_waves;
    struct Temps {
        PinBuf *a, *b, *c;
        ~Temps()
        {
            a->release();
            b->release();
            c->release();
        }
    };
    if (n_fill) {
        // ---- the image, built on the host (it touches every byte once: the symbol check rides along).  Under a matrix the image
        // holds symbol numbers, code + 1, and 0 stays the padding; a byte outside the alphabet is written as padding and fails
        // the create below
        rc = h_img.alloc(ctx, (size_t)img_dw * 4);
        if (!rc) rc = h_groups.alloc(ctx, n_fill * sizeof(SwBandGroup));
        if (!rc) rc = h_waves.alloc(ctx, waves.size() * sizeof(SwWave));
        Temps temps{&h_img, &h_groups, &h_waves}; // released after `done` below has drained (it is declared later, so runs first)
        DrainOnError drain(ctx, [] {});
        if (rc) return rc;
        memcpy(h_groups.p, groups.data(), n_fill * sizeof(SwBandGroup));
        memcpy(h_waves.p, waves.data(), waves.size() * sizeof(SwWave));
        std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
        uint8_t *im = (uint8_t *)h_img.p;
        agx_parallel_for((int64_t)n_fill, 64, [&](int64_t lo, int64_t hi, int t) {
            int64_t first_bad = -1;
            for (int64_t k = lo; k < hi; ++k) {
                const SwBandGroup &g = groups[(size_t)k];
                const uint32_t la = g.la_lb & 0xffffu, lb = g.la_lb >> 16;
                const uint8_t *sa = bases + off[2 * (size_t)g.out], *sb = bases + off[2 * (size_t)g.out + 1] + g.reserved; // (row0)
                uint8_t *xa = im + (size_t)g.x_dw * 4, *ya = im + (size_t)g.y_dw * 4;
                const size_t xbytes = ((size_t)(g.fpad + la + 3) / 4 + 1) * 4, ybytes = ((size_t)(lb + 4) / 4 + 1) * 4;
                memset(xa, 0, g.fpad);
                memset(xa + g.fpad + la, 0, xbytes - g.fpad - la);
                ya[0] = 0;
                memset(ya + 1 + lb, 0, ybytes - 1 - lb);
                bool hit;
                if (matrix) {
                    const uint8_t *code = matrix->code, *b0 = sb - g.reserved;
                    const uint32_t lb_all = len[2 * (size_t)g.out + 1];
                    uint8_t miss = 0; // the OR of every code met: a valid one is below 32, so bit 7 says that some byte maps to 0xff
                    for (uint32_t k = 0; k < la; ++k) {
                        const uint8_t c = code[sa[k]];
                        miss |= c;
                        xa[g.fpad + k] = c == 0xff ? 0 : (uint8_t)(c + 1);
                    }
                    for (uint32_t k = 0; k < lb; ++k) {
                        const uint8_t c = code[sb[k]];
                        ya[1 + k] = c == 0xff ? 0 : (uint8_t)(c + 1);
                    }
                    for (uint32_t k = 0; k < lb_all; ++k) miss |= code[b0[k]]; // (all of b, as below)
                    hit = (miss & 0x80u) != 0;
                } else {
                    memcpy(xa + g.fpad, sa, la);
                    memcpy(ya + 1, sb, lb);
                    // (all of b, the rows a band around a diagonal leaves out included)
                    hit = memchr(sa, 0, la) || memchr(sb - g.reserved, 0, len[2 * (size_t)g.out + 1]);
                }
                if (hit && (first_bad < 0 || (int64_t)g.out < first_bad)) first_bad = g.out;
            }
            bad[(size_t)t] = first_bad;
        });
        int64_t first_bad = -1;
        for (int64_t v : bad)
            if (v >= 0 && (first_bad < 0 || v < first_bad)) first_bad = v;
        if (first_bad >= 0) {
            if (matrix) agx_set_error("pair %lld contains a byte outside the substitution matrix's alphabet", (long long)first_bad);
            else agx_set_error("pair %lld contains byte 0x00, which is reserved as the padding symbol", (long long)first_bad);
            return AGX_E_SYMBOL;
        }
        rc = b->img.alloc(ctx, (size_t)img_dw * 4);
        if (!rc && matrix) rc = b->table.alloc(ctx, mat_table.size() * sizeof(int16_t));
        if (!rc) rc = b->groups.alloc(ctx, n_fill * sizeof(SwBandGroup));
        if (!rc) rc = b->waves.alloc(ctx, waves.size() * sizeof(SwWave));
        if (!rc && launches.size() > 1) rc = agx_ctx_prepare_fanout(ctx);
        if (rc) return rc;
        hipStream_t cs = ctx->copy;
        AGX_HIP(hipMemcpyAsync(b->img.p, h_img.p, (size_t)img_dw * 4, hipMemcpyHostToDevice, cs));
        AGX_HIP(hipMemcpyAsync(b->groups.p, h_groups.p, n_fill * sizeof(SwBandGroup), hipMemcpyHostToDevice, cs));
        AGX_HIP(hipMemcpyAsync(b->waves.p, h_waves.p, waves.size() * sizeof(SwWave), hipMemcpyHostToDevice, cs));
        // (pageable: the runtime stages it before the call returns; mat_table outlives the wait below in any case)
        if (matrix) AGX_HIP(hipMemcpyAsync(b->table.p, mat_table.data(), mat_table.size() * sizeof(int16_t), hipMemcpyHostToDevice, cs));
        // results and their landing blocks (a later failure leaves behind the queued copies: `drain` waits for them)
        const size_t words = (size_t)n_pairs * sizeof(uint32_t);
        rc = b->scores.alloc(ctx, words);
        if (!rc) rc = b->band_pos.alloc(ctx, words);
        if (!rc) rc = b->out_stage.alloc(ctx, words);
        if (!rc) rc = b->band_pos_stage.alloc(ctx, words);
        if (!rc && zd) rc = b->band_stop.alloc(ctx, words);
        if (!rc && zd) rc = b->band_stop_stage.alloc(ctx, words);
        if (rc) return rc;
        AGX_HIP(hipStreamSynchronize(cs));
        drain.ok = true;
    }
    *out = b;
    b = nullptr;
    done.ok = true;
    return AGX_OK;
}

int band_launch(agx_sw_batch *b)
{
    b->cig_valid = false; // what agx_sw_batch_cigars kept belongs to the launch before
    if (b->launches.empty()) return AGX_OK;
    FanOut fan(b->ctx, (int)b->launches.size());
    int rc = fan.begin();
    if (rc) return rc;
    int k = 0;
    // widest class first: its waves have the longest steps
    for (auto it = b->launches.rbegin(); it != b->launches.rend(); ++it) {
        const ClassLaunch &cl = *it;
        if (b->zdrop_on) {
            if (agx_sw_band_zdrop_launch_class(cl.C, b->prm, (const uint32_t *)b->img.p, (const SwBandGroup *)b->groups.p,
                                               (const SwWave *)b->waves.p + cl.first_wave, cl.n_waves, (int32_t *)b->scores.p,
                                               (uint32_t *)b->band_pos.p, b->zdrop, (int32_t *)b->band_stop.p, fan.stream(k++))) {
                agx_set_error("sw_fill_band_zd<%d> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
            continue;
        }
        if (b->matrix) {
            if (agx_sw_band_mat_launch_class(cl.C, b->mode, b->prm, (const uint32_t *)b->img.p, (const SwBandGroup *)b->groups.p,
                                             (const SwWave *)b->waves.p + cl.first_wave, cl.n_waves, (int32_t *)b->scores.p,
                                             (uint32_t *)b->band_pos.p, (const int16_t *)b->table.p, fan.stream(k++))) {
                agx_set_error("sw_fill_band_mat<%d, %d> launch failed: %s", cl.C, b->mode, hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
            continue;
        }
        if (b->band_at && b->mode != AGX_SW_MODE_GLOBAL && b->mode != AGX_SW_MODE_EXTEND) {
            if (agx_sw_band_at_launch_class(cl.C, b->mode, b->prm, (const uint32_t *)b->img.p, (const SwBandGroup *)b->groups.p,
                                            (const SwWave *)b->waves.p + cl.first_wave, cl.n_waves, (int32_t *)b->scores.p,
                                            (uint32_t *)b->band_pos.p, fan.stream(k++))) {
                agx_set_error("sw_fill_band_at<%d, %d> launch failed: %s", cl.C, b->mode, hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
            continue;
        }
        if (agx_sw_band_launch_class(cl.C, b->mode == AGX_SW_MODE_EXTEND, b->prm, (const uint32_t *)b->img.p, (const SwBandGroup *)b->groups.p,
                                     (const SwWave *)b->waves.p + cl.first_wave, cl.n_waves, (int32_t *)b->scores.p, (uint32_t *)b->band_pos.p,
                                     fan.stream(k++))) {
            agx_set_error("sw_fill_band<%d> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
    }
    return fan.end();
}

// band_hits of a batch around a diagonal (include/agx.h, "Banded alignment around a diagonal"): the fill's rows are counted from
// the pair's first row; every reported cell is checked against the matrix and the band.  begins: run the begin pass of a SPANS
// batch in LOCAL and FIT (agx_sw_batch_scores does not need it) -- a second batch of the same kind over the reversed prefixes,
// whose band is the mirror image of the pair's: reversed, cell (i, j) of the span of cb rows and ca columns is (cb - i, ca - j),
// so diagonal d becomes ca - cb - d and the centre c becomes ca - cb - c, the half-width stays.
int band_at_hits(agx_sw_batch *b, agx_sw_hit *hits, bool begins)
{
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    hipStream_t st = b->ctx->stream;
    const int64_t n = b->n_pairs;
    const int mode = b->mode;
    const bool cell = mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_EXTEND, column = mode == AGX_SW_MODE_FIT || mode == AGX_SW_MODE_EXTEND_QUERY;
    if (!b->launches.empty()) {
        AGX_HIP(hipMemcpyAsync(b->out_stage.p, b->scores.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (cell || column) AGX_HIP(hipMemcpyAsync(b->band_pos_stage.p, b->band_pos.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    AGX_HIP(hipStreamSynchronize(st));
    const int32_t *sc = (const int32_t *)b->out_stage.p;
    const uint32_t *ps = (const uint32_t *)b->band_pos_stage.p;
    const bool spans = b->align == AGX_SW_ALIGN_SPANS;
    const agx_sw_hit nothing{0, -1, -1, -1, -1};
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t la = b->seq_len[(size_t)(2 * p)], lb = b->seq_len[(size_t)(2 * p + 1)];
        const uint32_t row0 = b->band_row0[(size_t)p];
        if (!la || !lb) {
            hits[p] = mode == AGX_SW_MODE_LOCAL ? nothing : empty_side_hit(mode, b->align, b->scoring, la, lb);
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
    const BandAt rat{AGX_SW_ALIGN_ENDS, rdiag.data()};
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
    rc = agx_sw_batch_launch(rb);
    if (!rc) rc = band_at_hits(rb, rh.data(), false);
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
    hipStream_t st = b->ctx->stream;
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
    hipStream_t st = b->ctx->stream;
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
