// CIGARs of the Smith-Waterman path (include/agx.h, "Alignment itself", "CIGARs for banded batches"):
// the bounds and the host's checks, one driver (cigars_impl) for every kind of cigar batch with a tracer per kind, and the entry
// points.  (The chunks of a banded cigar batch are laid out in waves by the banded planner's builder, layout_band_waves.)
#include "agx_sw_batch.h"

#include "agx_parallel.h"

using namespace agx_sw_host;

namespace {
// What one traced pair may take of the chunk budget: its directions in the class that needs the most dwords for its length (the
// plan is made per chunk and chooses later), plus its operation slot.  Independent of the plan, so the cut is the caller's.
uint64_t trace_bytes_bound(uint32_t ca, uint32_t cb)
{
    uint64_t worst = 0;
#define AGX_SW_BOUND(CC)                                                           \
    if ((ca + CC - 1u) / CC <= 64u) worst = std::max(worst, sw_trace_dwords((int)((ca + CC - 1u) / CC), cb, CC));
    AGX_SW_FOR_EACH_TRACE_CLASS(AGX_SW_BOUND)
#undef AGX_SW_BOUND
    return 4u * (worst + (uint64_t)ca + cb);
}

// The host's check of one CIGAR (include/agx.h, "Alignment itself"): runs well-formed and merged, exactly x and y consumed,
// every '=' / 'X' true of the symbols, and the operations rescored give `score`.  code: the matrix's byte map, or NULL.
// dual: the six numbers of a batch under two-piece gap costs, or NULL -- every run of I or D then costs the LITERAL
// max(gap_open + L gap_extend, gap_open2 + L gap_extend2) of its whole length, whatever pieces the walk joined into it.
bool cigar_checks(const uint32_t *ops, uint64_t n_ops, const uint8_t *x, int64_t ca, const uint8_t *y, int64_t cb, const agx_sw_scoring &s,
                  const agx_sw_matrix *m, int64_t score, const agx_sw_scoring_dual *dual = nullptr)
{
    const auto gap = [&](int64_t len) -> int64_t {
        const int64_t one = s.gap_open + len * s.gap_extend;
        return dual ? std::max<int64_t>(one, dual->gap_open2 + len * dual->gap_extend2) : one;
    };
    int64_t i = 0, j = 0, total = 0;
    uint32_t prev = 0;
    for (uint64_t k = 0; k < n_ops; ++k) {
        const uint32_t op = ops[k] & 15u;
        const int64_t len = ops[k] >> 4;
        if (len == 0 || op == prev) return false;
        prev = op;
        if (op == AGX_CIGAR_EQ || op == AGX_CIGAR_DIFF) {
            if (j + len > ca || i + len > cb) return false;
            for (int64_t t = 0; t < len; ++t, ++i, ++j) {
                const bool same = m ? m->code[x[j]] == m->code[y[i]] : x[j] == y[i];
                if (same != (op == AGX_CIGAR_EQ)) return false;
                total += m ? m->score[m->code[x[j]]][m->code[y[i]]] : same ? s.match : s.mismatch;
            }
        } else if (op == AGX_CIGAR_INS) {
            j += len;
            total += gap(len);
        } else if (op == AGX_CIGAR_DEL) {
            i += len;
            total += gap(len);
        } else
            return false;
    }
    return i == cb && j == ca && total == score;
}

// ---- CIGARs of banded batches (include/agx.h, "CIGARs for banded batches")

// What one traced pair of a banded cigar batch may take of the chunk budget: its directions in the class that needs the most
// dwords for its band width and its rows, plus its operation slot.  Independent of the plan, as trace_bytes_bound.
uint64_t band_trace_bytes_bound(uint32_t width, uint32_t ca, uint32_t cb)
{
    uint64_t worst = 0;
    for (int c = 0; c < kSwNumBandClasses; ++c) {
        const uint32_t K = (uint32_t)kSwBandClasses[c], G = (width + K - 1u) / K;
        if (G >= 1u && G <= 64u) worst = std::max(worst, sw_band_trace_dwords((int)G, cb, (int)K));
    }
    return 4u * (worst + (uint64_t)ca + cb);
}

// The same for a cigar batch under two-piece gap costs: eight bits a cell, sw_band_dual_trace_dwords.
uint64_t band_dual_trace_bytes_bound(uint32_t width, uint32_t ca, uint32_t cb)
{
    uint64_t worst = 0;
    for (int c = 0; c < kSwNumBandClasses; ++c) {
        const uint32_t K = (uint32_t)kSwBandClasses[c], G = (width + K - 1u) / K;
        if (G >= 1u && G <= 64u) worst = std::max(worst, sw_band_dual_trace_dwords((int)G, cb, (int)K));
    }
    return 4u * (worst + (uint64_t)ca + cb);
}

// The band-aware part of the host's check: from (0, 0), after every operation dlo <= j - i <= dhi (within a run j - i moves one
// way only, so the run's end decides).
bool cigar_in_band(const uint32_t *ops, uint64_t n_ops, int64_t dlo, int64_t dhi)
{
    int64_t d = 0;
    if (d < dlo || d > dhi) return false;
    for (uint64_t k = 0; k < n_ops; ++k) {
        const uint32_t op = ops[k] & 15u;
        const int64_t len = ops[k] >> 4;
        if (op == AGX_CIGAR_INS) d += len;
        else if (op == AGX_CIGAR_DEL) d -= len;
        else if (op != AGX_CIGAR_EQ && op != AGX_CIGAR_DIFF) return false;
        if (d < dlo || d > dhi) return false;
    }
    return true;
}

// in-band cells (1 <= i <= cb, 1 <= j <= ca, dlo <= j - i <= dhi) of a span
int64_t band_cells(int64_t ca, int64_t cb, int64_t dlo, int64_t dhi)
{
    int64_t cells = 0;
    for (int64_t i = 1; i <= cb; ++i) {
        const int64_t lo = std::max<int64_t>(1, i + dlo), hi = std::min<int64_t>(ca, i + dhi);
        if (hi >= lo) cells += hi - lo + 1;
    }
    return cells;
}

// Where the traced fill of a span starts inside a banded batch's resident image (include/agx.h, agx_sw_band_span_record; the
// head of agx_sw_band_diag_trace_kernel.hip has the argument).  false: the span does not lie in the image or in the band.
bool band_span_record(uint32_t la, uint32_t rows, uint32_t row0, uint32_t fpad, int64_t dlo, int64_t dhi, int lanes, const agx_sw_hit &h,
                      agx_sw_band_span &o)
{
    if (lanes < 1 || lanes > 64 || dhi < dlo) return false;
    if (h.a_begin < 0 || h.b_begin < 0 || h.a_end < h.a_begin || h.b_end < h.b_begin) return false;
    if ((uint32_t)h.a_end >= la || (uint32_t)h.b_begin < row0 || (uint64_t)h.b_end >= (uint64_t)row0 + rows) return false;
    const int64_t s = (int64_t)h.b_begin - row0, shift = s - h.a_begin;
    const int64_t ca = (int64_t)h.a_end - h.a_begin + 1, cb = (int64_t)h.b_end - h.b_begin + 1;
    const int64_t lo = dlo + shift, hi = dhi + shift;
    if (lo > 0 || hi < 0 || ca - cb < lo || ca - cb > hi) return false; // the begin and the end cell
    o.ca = (uint32_t)ca;
    o.cb = (uint32_t)cb;
    o.x_bytes = fpad + (uint32_t)h.a_begin;
    o.phase = (uint32_t)(s & 3);
    o.y_dwords = (uint32_t)((s - o.phase) / 4);
    o.dlo = (int32_t)lo;
    o.dhi = (int32_t)hi;
    o.steps = (uint32_t)cb + (uint32_t)lanes + o.phase;
    return true;
}

// ---- the driver of agx_sw_batch_cigars and its two tracers

inline void span_of(const agx_sw_hit &h, int64_t &ca, int64_t &cb)
{
    ca = h.a_begin >= 0 && h.a_end >= h.a_begin ? (int64_t)h.a_end - h.a_begin + 1 : 0;
    cb = h.b_begin >= 0 && h.b_end >= h.b_begin ? (int64_t)h.b_end - h.b_begin + 1 : 0;
}

// One chunk of traced spans on the device: every block it takes, and what its tracer hands the driver.  Every exit waits for the
// stream before the blocks go back to the pool: nothing may still run on them.
struct CigarChunk {
    agx_ctx *ctx;
    agx_sw_batch *tb = nullptr;                      // plain kind: the cigar == 2 batch of the copied spans, their arrays,
    std::vector<uint64_t> span_off;                  // ... and its hits (all kept for the chunk's time, as the blocks are)
    std::vector<uint32_t> span_len;
    std::vector<uint8_t> span_bytes;
    std::vector<agx_sw_hit> span_hits;
    DevBuf groups, waves, goff, walk, bwalk, scores; // banded kind: the chunk's own records over the batch's resident image,
    PinBuf h_scores;                                 // ... its scores, and the host's records until the stream has read them
    std::vector<SwBandGroup> plan_groups;
    std::vector<SwWave> plan_waves;
    std::vector<uint64_t> plan_goff;
    std::vector<SwWalkRec> plan_walk;
    std::vector<SwBandWalkRec> plan_bwalk;
    DevBuf trace, slots, runs, dst, dense; // both kinds (chunk_blocks; dense once the runs are counted)
    PinBuf h_runs, h_dense;
    // from the tracer: the walk records on the device, the extents of directions and slots, the traced scores in chunk order
    const SwWalkRec *walkrec = nullptr;
    uint64_t tr_dwords = 0, slot_words = 0;
    std::vector<int32_t> score;
    explicit CigarChunk(agx_ctx *c) : ctx(c) {}
    CigarChunk(const CigarChunk &) = delete;
    ~CigarChunk()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (DevBuf *v : {&groups, &waves, &goff, &walk, &bwalk, &scores, &trace, &slots, &runs, &dst, &dense}) v->release();
        for (PinBuf *v : {&h_runs, &h_scores, &h_dense}) v->release();
        if (tb) agx_sw_batch_destroy(tb);
    }
};

// What a tracer calls once it knows tr_dwords and slot_words: the blocks both kinds take, and the chunk's entry in cig_info.
int chunk_blocks(agx_sw_batch *b, CigarChunk &c, int64_t m, uint64_t min_trace_dwords)
{
    int rc = c.trace.alloc(c.ctx, std::max<uint64_t>(c.tr_dwords, min_trace_dwords) * 4);
    if (!rc) rc = c.slots.alloc(c.ctx, std::max<uint64_t>(c.slot_words, 1) * 4);
    if (!rc) rc = c.runs.alloc(c.ctx, (size_t)m * sizeof(uint32_t));
    if (!rc) rc = c.dst.alloc(c.ctx, (size_t)m * sizeof(uint64_t));
    if (!rc) rc = c.h_runs.alloc(c.ctx, (size_t)m * sizeof(uint32_t));
    if (rc) return rc;
    b->cig_info.trace_bytes_peak = std::max<int64_t>(b->cig_info.trace_bytes_peak, (int64_t)((c.tr_dwords + c.slot_words) * 4));
    ++b->cig_info.n_chunks;
    return AGX_OK;
}

// What differs between the kinds of cigar batch.  Every function reads the hits from b->cig_hits.
struct Tracer {
    int (*hits)(agx_sw_batch *b, agx_sw_hit *hits);
    // pair p has a span of ca x cb: may it be traced (else the error text is set), what may it take of the chunk budget, and
    // how many cells will be filled for it
    int (*admit)(const agx_sw_batch *b, int64_t p, int64_t ca, int64_t cb, uint64_t &bytes, int64_t &cells);
    // One chunk, the m pairs pairs[0 .. m): plan, allocate, and on the context's stream the traced fill and the walk (ev, when
    // not NULL: events 0, 1, 2 around them), the copy of the run counts into c.h_runs and the traced scores into c.score.
    // Returns when both have landed.
    int (*trace)(agx_sw_batch *b, const int64_t *pairs, int64_t m, CigarChunk &c, hipEvent_t *ev);
    // the kind's own check of a finished CIGAR besides cigar_checks (NULL: none)
    bool (*check)(const agx_sw_batch *b, int64_t p, const uint32_t *ops, uint64_t n_ops);
    // where the kinds' error messages differ (banded: the band's half-width goes into band_note)
    const char *band_note, *walk_failed_note, *leave_note;
};

// ---- plain cigar batches: the spans are copied into a GLOBAL batch of their own, whose fill is the traced build

int plain_hits(agx_sw_batch *b, agx_sw_hit *hits) { return hits_impl(b, hits, nullptr); }

int plain_admit(const agx_sw_batch *, int64_t, int64_t ca, int64_t cb, uint64_t &bytes, int64_t &cells)
{
    bytes = trace_bytes_bound((uint32_t)ca, (uint32_t)cb);
    cells = ca * cb;
    return AGX_OK;
}

int plain_trace(agx_sw_batch *b, const int64_t *pairs, int64_t m, CigarChunk &c, hipEvent_t *ev)
{
    agx_ctx *ctx = b->ctx;
    hipStream_t st = agx_enqueue_stream(ctx);
    const agx_sw_hit *hits = b->cig_hits.data();
    // the spans as a batch of their own, not reversed
    std::vector<uint64_t> &soff = c.span_off;
    std::vector<uint32_t> &slen = c.span_len;
    std::vector<uint8_t> &sub = c.span_bytes;
    soff.resize((size_t)m * 2);
    slen.resize((size_t)m * 2);
    uint64_t at = 0;
    for (int64_t k = 0; k < m; ++k) {
        int64_t ca, cb;
        span_of(hits[pairs[k]], ca, cb);
        soff[(size_t)(2 * k)] = at;
        slen[(size_t)(2 * k)] = (uint32_t)ca;
        at += (uint64_t)ca;
        soff[(size_t)(2 * k + 1)] = at;
        slen[(size_t)(2 * k + 1)] = (uint32_t)cb;
        at += (uint64_t)cb;
    }
    sub.resize((size_t)at);
    agx_parallel_for(m, 4096, [&](int64_t lo, int64_t hi, int) {
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t p = pairs[k];
            memcpy(sub.data() + soff[(size_t)(2 * k)], b->seq.data() + b->seq_off[(size_t)(2 * p)] + hits[p].a_begin, slen[(size_t)(2 * k)]);
            memcpy(sub.data() + soff[(size_t)(2 * k + 1)], b->seq.data() + b->seq_off[(size_t)(2 * p + 1)] + hits[p].b_begin, slen[(size_t)(2 * k + 1)]);
        }
    });
    int rc = create_batch(ctx, &b->scoring, b->matrix ? &b->mat : nullptr, sub.data(), soff.data(), slen.data(), m, &c.tb, false, AGX_SW_ALIGN_ENDS,
                          AGX_SW_MODE_GLOBAL, 0, 2);
    if (rc) return rc;
    agx_sw_batch *tb = c.tb;
    c.tr_dwords = tb->tr_dwords;
    c.slot_words = tb->tr_slot_words;
    c.walkrec = (const SwWalkRec *)tb->walkrec.p;
    rc = chunk_blocks(b, c, m, 1);
    if (rc) return rc;
    tb->trace_p = (uint32_t *)c.trace.p;
    if (ev) AGX_HIP(hipEventRecord(ev[0], st));
    rc = agx_sw_batch_launch(tb);
    if (rc) return rc;
    if (ev) AGX_HIP(hipEventRecord(ev[1], st));
    if (agx_sw_walk_launch(c.walkrec, (uint32_t)m, (const uint32_t *)tb->img.p, (const uint32_t *)c.trace.p, (uint32_t *)c.slots.p,
                           (uint32_t *)c.runs.p, st)) {
        agx_set_error("agx_sw_batch_cigars: walk kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        return AGX_E_HIP;
    }
    if (ev) AGX_HIP(hipEventRecord(ev[2], st));
    AGX_HIP(hipMemcpyAsync(c.h_runs.p, c.runs.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    std::vector<agx_sw_hit> &th = c.span_hits;
    th.resize((size_t)m);
    rc = hits_impl(tb, th.data(), nullptr); // (waits for the stream: the run counts have landed too)
    if (rc) return rc;
    c.score.resize((size_t)m);
    for (int64_t k = 0; k < m; ++k) c.score[(size_t)k] = th[(size_t)k].score;
    return AGX_OK;
}

constexpr Tracer kPlainTracer{plain_hits, plain_admit, plain_trace, nullptr, nullptr, "", ""};

// ---- banded cigar batches: per chunk one traced banded fill (corner capture, whatever the mode: the
// span's global alignment inside the pair's band), the band-aware walk and the gather.  The fills read the batch's resident image
// through copies of its group records that carry the span's lengths, in the tiling the batch planned.  A batch around a diagonal
// (band_at) has spans that begin anywhere: its records are those of band_span_record, its fill and walk the builds that start
// inside the image (agx_sw_band_diag_trace_kernel.hip); every span of the other batches begins at (0, 0).

// the band the score of pair p was computed in, counted from the begin cell (begins are 0 unless the batch is banded around a diagonal)
void band_limits_of(const agx_sw_batch *b, int64_t p, int64_t &dlo, int64_t &dhi)
{
    if (!b->band_at) {
        band_limits(b->mode, b->band, b->seq_len[(size_t)(2 * p)], b->seq_len[(size_t)(2 * p + 1)], dlo, dhi);
        return;
    }
    const agx_sw_hit &h = b->cig_hits[(size_t)p];
    const int64_t delta = h.a_begin >= 0 && h.b_begin >= 0 ? (int64_t)h.a_begin - h.b_begin : b->band_diag[(size_t)p]; // (no begin cell: no path)
    dlo = (int64_t)b->band_diag[(size_t)p] - b->band - delta;
    dhi = (int64_t)b->band_diag[(size_t)p] + b->band - delta;
}

int band_admit(const agx_sw_batch *b, int64_t p, int64_t ca, int64_t cb, uint64_t &bytes, int64_t &cells)
{
    if (b->band_rec[(size_t)p] == kNoBandRec) {
        agx_set_error("agx_sw_batch_cigars: pair %lld has a span of %lld x %lld and no fill", (long long)p, (long long)ca, (long long)cb);
        return AGX_E_INTERNAL;
    }
    int64_t dlo, dhi;
    band_limits_of(b, p, dlo, dhi);
    cells = band_cells(ca, cb, dlo, dhi);
    const SwBandGroup &g = b->band_groups[b->band_rec[(size_t)p]];
    bytes = (b->dual ? band_dual_trace_bytes_bound : band_trace_bytes_bound)((uint32_t)(g.dhi - g.dlo + 1), (uint32_t)ca, (uint32_t)cb);
    return AGX_OK;
}

int band_trace(agx_sw_batch *b, const int64_t *pairs, int64_t m, CigarChunk &c, hipEvent_t *ev)
{
    agx_ctx *ctx = b->ctx;
    hipStream_t st = agx_enqueue_stream(ctx);
    const agx_sw_hit *hits = b->cig_hits.data();
    const bool at = b->band_at;
    // ---- the chunk's plan: the batch's tiling per pair, longest span first, in waves by the wave builder of the batch's own plan
    struct Item {
        uint32_t k, rec, lb; // the pair's place in the chunk, its record, the span's rows
        uint8_t cls, G;
    };
    std::vector<Item> items((size_t)m);
    for (int64_t k = 0; k < m; ++k) {
        int64_t ca, cb;
        span_of(hits[pairs[k]], ca, cb);
        const uint32_t rec = b->band_rec[(size_t)pairs[k]];
        items[(size_t)k] = Item{(uint32_t)k, rec, (uint32_t)cb, b->band_cls[rec], b->band_G[rec]};
    }
    std::sort(items.begin(), items.end(), [](const Item &x, const Item &y) {
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.G != y.G) return x.G < y.G;
        if (x.lb != y.lb) return x.lb > y.lb;
        return x.k < y.k;
    });
    std::vector<SwBandGroup> &groups = c.plan_groups;
    std::vector<uint64_t> &goff = c.plan_goff;
    std::vector<SwWalkRec> &walk = c.plan_walk;
    std::vector<SwBandWalkRec> &bwalk = c.plan_bwalk;
    std::vector<SwWave> &waves = c.plan_waves;
    groups.resize((size_t)m);
    goff.resize((size_t)m);
    walk.resize((size_t)m);
    bwalk.resize((size_t)m);
    std::vector<ClassLaunch> launches;
    layout_band_waves(items, waves, launches);
    uint64_t tr_dwords = 0, slot_words = 0;
    for (SwWave &w : waves) {
        const int K = (int)w.reserved, G = w.G;
        for (size_t k = w.first_group, end = k + w.n_groups; k < end; ++k) {
            const Item &e = items[k];
            const int64_t p = pairs[e.k];
            int64_t ca, cb;
            span_of(hits[p], ca, cb);
            SwBandGroup g = b->band_groups[e.rec]; // image offsets, band and fpad as planned; the span's lengths
            uint32_t phase = 0;
            if (at) { // the span begins inside the image
                agx_sw_band_span sp;
                if (!band_span_record(g.la_lb & 0xffffu, g.la_lb >> 16, g.reserved, g.fpad, g.dlo, g.dhi, G, hits[p], sp) || sp.ca != (uint32_t)ca ||
                    sp.cb != (uint32_t)cb) {
                    agx_set_error("agx_sw_batch_cigars: pair %lld (mode %d, diag %d, band %d): its span a %d..%d, b %d..%d does not lie in the rows "
                                  "%u.. of its image or its begin or end cell is outside the band",
                                  (long long)p, b->mode, b->band_diag[(size_t)p], b->band, hits[p].a_begin, hits[p].a_end, hits[p].b_begin,
                                  hits[p].b_end, g.reserved);
                    return AGX_E_INTERNAL;
                }
                g.y_dw += sp.y_dwords;
                g.fpad = sp.x_bytes;
                g.dlo = sp.dlo;
                g.dhi = sp.dhi;
                g.reserved = phase = sp.phase;
                w.steps = std::max(w.steps, sp.steps);
            }
            g.la_lb = (uint32_t)ca | (uint32_t)cb << 16;
            g.out = e.k;
            groups[k] = g;
            goff[k] = tr_dwords;
            SwWalkRec &r = walk[e.k];
            r.goff = tr_dwords;
            r.slot = 0; // below, in the caller's order
            r.x_dw = g.x_dw;
            r.y_dw = g.y_dw;
            r.ca = (uint32_t)ca;
            r.cb = (uint32_t)cb;
            r.G = (uint16_t)G;
            r.C = (uint16_t)K;
            r.reserved = phase;
            int ks = 0;
            while ((1 << ks) < K) ++ks;
            bwalk[e.k] = SwBandWalkRec{g.dlo, g.dhi, g.fpad, (uint32_t)ks};
            tr_dwords += (b->dual ? sw_band_dual_trace_dwords : sw_band_trace_dwords)(G, (uint32_t)cb, K);
        }
    }
    for (int64_t k = 0; k < m; ++k) {
        walk[(size_t)k].slot = slot_words;
        slot_words += (uint64_t)walk[(size_t)k].ca + walk[(size_t)k].cb;
    }
    int rc = c.groups.alloc(ctx, (size_t)m * sizeof(SwBandGroup));
    if (!rc) rc = c.waves.alloc(ctx, waves.size() * sizeof(SwWave));
    if (!rc) rc = c.goff.alloc(ctx, (size_t)m * sizeof(uint64_t));
    if (!rc) rc = c.walk.alloc(ctx, (size_t)m * sizeof(SwWalkRec));
    if (!rc) rc = c.bwalk.alloc(ctx, (size_t)m * sizeof(SwBandWalkRec));
    if (!rc) rc = c.scores.alloc(ctx, (size_t)m * sizeof(int32_t));
    if (!rc) rc = c.h_scores.alloc(ctx, (size_t)m * sizeof(int32_t));
    if (rc) return rc;
    c.tr_dwords = tr_dwords;
    c.slot_words = slot_words;
    c.walkrec = (const SwWalkRec *)c.walk.p;
    rc = chunk_blocks(b, c, m, 4);
    if (rc) return rc;
    AGX_HIP(hipMemcpyAsync(c.groups.p, groups.data(), (size_t)m * sizeof(SwBandGroup), hipMemcpyHostToDevice, st));
    AGX_HIP(hipMemcpyAsync(c.waves.p, waves.data(), waves.size() * sizeof(SwWave), hipMemcpyHostToDevice, st));
    AGX_HIP(hipMemcpyAsync(c.goff.p, goff.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    AGX_HIP(hipMemcpyAsync(c.walk.p, walk.data(), (size_t)m * sizeof(SwWalkRec), hipMemcpyHostToDevice, st));
    AGX_HIP(hipMemcpyAsync(c.bwalk.p, bwalk.data(), (size_t)m * sizeof(SwBandWalkRec), hipMemcpyHostToDevice, st));
    if (ev) AGX_HIP(hipEventRecord(ev[0], st));
    const SwBandFill &fill = band_fill(b, true);
    SwBandArgs a{};
    a.prm = b->prm;
    a.dual_gap = b->dual_gap;
    a.img = (const uint32_t *)b->img.p;
    a.groups = (const SwBandGroup *)c.groups.p;
    a.scores = (int32_t *)c.scores.p;
    a.trace = (uint32_t *)c.trace.p;
    a.goff = (const uint64_t *)c.goff.p;
    a.table = (const int16_t *)b->table.p;
    for (auto it = launches.rbegin(); it != launches.rend(); ++it) { // widest class first, one after the other on the stream
        a.waves = (const SwWave *)c.waves.p + it->first_wave;
        a.n_waves = it->n_waves;
        if (fill.launch(it->C, b->mode, a, st)) return band_fill_failed(fill, it->C, b->mode);
    }
    if (ev) AGX_HIP(hipEventRecord(ev[1], st));
    const SwBandWalkArgs wa{c.walkrec, (const SwBandWalkRec *)c.bwalk.p, (uint32_t)m, a.img, a.trace, (uint32_t *)c.slots.p, (uint32_t *)c.runs.p};
    if (fill.walk(wa, st)) {
        agx_set_error("agx_sw_batch_cigars: walk kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        return AGX_E_HIP;
    }
    if (ev) AGX_HIP(hipEventRecord(ev[2], st));
    AGX_HIP(hipMemcpyAsync(c.h_runs.p, c.runs.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    AGX_HIP(hipMemcpyAsync(c.h_scores.p, c.scores.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AGX_HIP(hipStreamSynchronize(st));
    c.score.assign((const int32_t *)c.h_scores.p, (const int32_t *)c.h_scores.p + m);
    return AGX_OK;
}

bool band_check(const agx_sw_batch *b, int64_t p, const uint32_t *ops, uint64_t n_ops)
{
    int64_t dlo, dhi;
    band_limits_of(b, p, dlo, dhi);
    return !n_ops || cigar_in_band(ops, n_ops, dlo, dhi);
}

constexpr Tracer kBandTracer{band_hits, band_admit, band_trace, band_check, ", band %d", " (the walk left the band)", ", leave the band"};

// agx_sw_batch_cigars: hits (SPANS), then per chunk of spans one traced fill and walk -- the kind's tracer -- and the gather; every
// CIGAR is checked on the host; the answer goes into the batch (cig_hits, cig_off, cig_ops).
int cigars_impl(agx_sw_batch *b)
{
    const Tracer &t = b->banded ? kBandTracer : kPlainTracer;
    const int64_t n = b->n_pairs;
    b->cig_valid = false;
    b->cig_info = agx_sw_cigar_info{};
    b->cig_hits.assign((size_t)n, agx_sw_hit{});
    b->cig_off.assign((size_t)n + 1, 0);
    b->cig_ops.clear();
    int rc = t.hits(b, b->cig_hits.data());
    if (rc || n == 0) {
        b->cig_valid = !rc;
        return rc;
    }
    agx_ctx *ctx = b->ctx;
    const agx_sw_hit *hits = b->cig_hits.data();
    const agx_sw_matrix *mat = b->matrix ? &b->mat : nullptr;
    const agx_sw_scoring s = b->scoring; // (under a matrix: its gap_open and gap_extend, which is all that is read of it)
    const agx_sw_scoring_dual *dual = b->dual ? &b->dual_sc : nullptr; // (under two pieces s is the first)
    char band_note[32] = "";
    if (t.band_note) snprintf(band_note, sizeof band_note, t.band_note, b->band);
    // ---- pairs answered without a fill, and the list of the others
    std::vector<uint32_t> count((size_t)n, 0), lone((size_t)n, 0); // operations per pair; the only one of a pair with an empty side
    std::vector<int64_t> traced;
    std::vector<uint64_t> need; // what every traced pair may take of the budget
    int64_t cells = 0;
    for (int64_t p = 0; p < n; ++p) {
        int64_t ca, cb;
        span_of(hits[p], ca, cb);
        if (ca && cb) {
            uint64_t bytes = 0;
            int64_t filled = 0;
            rc = t.admit(b, p, ca, cb, bytes, filled);
            if (rc) return rc;
            traced.push_back(p);
            need.push_back(bytes);
            cells += filled;
        } else if (ca || cb) {
            count[(size_t)p] = 1;
            lone[(size_t)p] = (uint32_t)(ca ? ca : cb) << 4 | (uint32_t)(ca ? AGX_CIGAR_INS : AGX_CIGAR_DEL);
        }
    }
    b->cig_info.n_traced = (int64_t)traced.size();
    b->cig_info.trace_cells = cells;
    // ---- chunks of traced pairs, in the caller's order, by the budget
    const uint64_t budget = (uint64_t)ctx->opt_sw_trace_bytes;
    std::vector<std::vector<uint32_t>> chunk_ops;  // every chunk's runs, dense
    std::vector<uint64_t> where((size_t)n, 0);     // a traced pair's first run in its chunk's array
    std::vector<uint32_t> chunk_of((size_t)n, 0);
    hipStream_t st = agx_enqueue_stream(ctx);
    // tuning build, AGX_TRACE_CIGAR: kernel-only times of every chunk's traced fill, walk and gather (HIP events on the stream)
    const bool timed = agx_tune("AGX_TRACE_CIGAR") != nullptr;
    struct Events {
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events()
        {
            for (hipEvent_t v : e)
                if (v) (void)hipEventDestroy(v);
        }
    } ev;
    if (timed)
        for (hipEvent_t &v : ev.e) AGX_HIP(hipEventCreate(&v));
    for (size_t first = 0; first < traced.size();) {
        size_t last = first;
        uint64_t bytes = 0;
        while (last < traced.size()) {
            if (last > first && bytes + need[last] > budget) break;
            bytes += need[last];
            ++last;
        }
        const int64_t m = (int64_t)(last - first);
        std::vector<uint64_t> dst((size_t)m);
        CigarChunk c(ctx);
        rc = t.trace(b, traced.data() + first, m, c, timed ? ev.e : nullptr);
        if (rc) return rc;
        const uint32_t *runs = (const uint32_t *)c.h_runs.p;
        uint64_t total = 0;
        for (int64_t k = 0; k < m; ++k) {
            const int64_t p = traced[first + (size_t)k];
            int64_t ca, cb;
            span_of(hits[p], ca, cb);
            if (c.score[(size_t)k] != hits[p].score || runs[k] == 0 || runs[k] > (uint64_t)ca + (uint64_t)cb) { // (kSwWalkFailed: the walk left the band)
                agx_set_error("agx_sw_batch_cigars: pair %lld (mode %d%s): the traced fill of its span a %d..%d, b %d..%d gives score %d in %u runs%s, "
                              "the hit %d",
                              (long long)p, b->mode, band_note, hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end, c.score[(size_t)k], runs[k],
                              t.walk_failed_note && runs[k] == kSwWalkFailed ? t.walk_failed_note : "", hits[p].score);
                return AGX_E_INTERNAL;
            }
            dst[(size_t)k] = total;
            where[(size_t)p] = total;
            chunk_of[(size_t)p] = (uint32_t)chunk_ops.size();
            count[(size_t)p] = runs[k];
            total += runs[k];
        }
        rc = c.dense.alloc(ctx, (size_t)total * sizeof(uint32_t));
        if (!rc) rc = c.h_dense.alloc(ctx, (size_t)total * sizeof(uint32_t));
        if (rc) return rc;
        AGX_HIP(hipMemcpyAsync(c.dst.p, dst.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (timed) AGX_HIP(hipEventRecord(ev.e[3], st));
        if (agx_sw_gather_launch(c.walkrec, (uint32_t)m, (const uint32_t *)c.slots.p, (const uint32_t *)c.runs.p, (const uint64_t *)c.dst.p,
                                 (uint32_t *)c.dense.p, st)) {
            agx_set_error("agx_sw_batch_cigars: gather kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
        if (timed) AGX_HIP(hipEventRecord(ev.e[4], st));
        AGX_HIP(hipMemcpyAsync(c.h_dense.p, c.dense.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        AGX_HIP(hipStreamSynchronize(st));
        if (timed) {
            float fill = 0, walk = 0, gather = 0;
            AGX_HIP(hipEventElapsedTime(&gather, ev.e[3], ev.e[4]));
            AGX_HIP(hipEventElapsedTime(&fill, ev.e[0], ev.e[1]));
            AGX_HIP(hipEventElapsedTime(&walk, ev.e[1], ev.e[2]));
            fprintf(stderr, "[agx_sw_batch_cigars] chunk %d: %lld pairs, %.1f MB of directions, %.1f MB of slots: traced fill %.3f ms, walk %.3f ms, gather %.3f ms, %llu runs\n",
                    b->cig_info.n_chunks - 1, (long long)m, c.tr_dwords * 4 / 1e6, c.slot_words * 4 / 1e6, fill, walk, gather, (unsigned long long)total);
        }
        chunk_ops.emplace_back((const uint32_t *)c.h_dense.p, (const uint32_t *)c.h_dense.p + total);
        first = last;
    } // (the chunk returns its blocks before the next chunk takes its own)
    // ---- the caller's layout, and every CIGAR checked before it leaves
    for (int64_t p = 0; p < n; ++p) b->cig_off[(size_t)p + 1] = b->cig_off[(size_t)p] + count[(size_t)p];
    b->cig_ops.resize((size_t)b->cig_off[(size_t)n]);
    std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
    agx_parallel_for(n, 4096, [&](int64_t lo, int64_t hi, int tid) {
        for (int64_t p = lo; p < hi; ++p) {
            int64_t ca, cb;
            span_of(hits[p], ca, cb);
            uint32_t *out = b->cig_ops.data() + b->cig_off[(size_t)p];
            const uint32_t c = count[(size_t)p];
            if (ca && cb) memcpy(out, chunk_ops[chunk_of[(size_t)p]].data() + where[(size_t)p], (size_t)c * sizeof(uint32_t));
            else if (c) out[0] = lone[(size_t)p];
            const uint8_t *x = ca ? b->seq.data() + b->seq_off[(size_t)(2 * p)] + hits[p].a_begin : nullptr;
            const uint8_t *y = cb ? b->seq.data() + b->seq_off[(size_t)(2 * p + 1)] + hits[p].b_begin : nullptr;
            if ((!cigar_checks(out, c, x, ca, y, cb, s, mat, hits[p].score, dual) || (t.check && !t.check(b, p, out, c))) && bad[(size_t)tid] < 0)
                bad[(size_t)tid] = p;
        }
    });
    for (int64_t p : bad)
        if (p >= 0) {
            agx_set_error("agx_sw_batch_cigars: pair %lld (mode %d%s): its %u operations do not consume the span a %d..%d, b %d..%d, disagree with the "
                          "symbols%s or do not rescore to %d",
                          (long long)p, b->mode, band_note, count[(size_t)p], hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end, t.leave_note,
                          hits[p].score);
            return AGX_E_INTERNAL;
        }
    b->cig_valid = true;
    return AGX_OK;
}
} // namespace

extern "C" {

uint64_t agx_sw_band_cigar_bytes_bound(int32_t width, uint32_t ca, uint32_t cb)
{
    if (width < 1 || width > AGX_SW_BAND_MAX_WIDTH) return 0;
    return band_trace_bytes_bound((uint32_t)width, ca, cb);
}

uint64_t agx_sw_band_dual_cigar_bytes_bound(int32_t width, uint32_t ca, uint32_t cb)
{
    if (width < 1 || width > AGX_SW_BAND_MAX_WIDTH) return 0;
    return band_dual_trace_bytes_bound((uint32_t)width, ca, cb);
}

int agx_sw_cigar_rescore_dual(const agx_sw_scoring_dual *scoring, const uint32_t *ops, uint64_t n_ops, const uint8_t *x, uint32_t ca,
                              const uint8_t *y, uint32_t cb, int32_t score)
{
    if (!scoring || (!ops && n_ops) || (!x && ca) || (!y && cb)) return 0;
    const agx_sw_scoring piece1{scoring->match, scoring->mismatch, scoring->gap_open, scoring->gap_extend};
    return cigar_checks(ops, n_ops, x, ca, y, cb, piece1, nullptr, score, scoring) ? 1 : 0;
}

int agx_sw_batch_create_align_band_diag_dual_cigar(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int32_t band, const int32_t *diag,
                                                   const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                                   agx_sw_batch **out)
{
    if (!scoring) { // (there is no reference default for a second piece)
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_band_diag_dual_cigar: scoring is NULL");
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    const BandAt at{AGX_SW_ALIGN_SPANS, diag, false, 0, 0, scoring};
    const agx_sw_scoring piece1{scoring->match, scoring->mismatch, scoring->gap_open, scoring->gap_extend};
    return create_band(ctx, &piece1, mode, band, bases, off, len, n_pairs, out, true, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_dual_cigar")
}

int agx_sw_align_band_diag_dual_cigar(agx_ctx *ctx, const agx_sw_scoring_dual *scoring, int mode, int32_t band, const int32_t *diag,
                                      const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                      uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_dual_cigar(ctx, scoring, mode, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap); });
}

int agx_sw_band_span_record(uint32_t la, uint32_t rows, uint32_t row0, uint32_t fpad, int32_t dlo, int32_t dhi, int32_t lanes,
                            const agx_sw_hit *hit, agx_sw_band_span *out)
{
    agx_sw_band_span sp;
    if (!hit || !out || !band_span_record(la, rows, row0, fpad, dlo, dhi, lanes, *hit, sp)) {
        agx_set_error("agx_sw_band_span_record: null argument, an empty side, a span outside the image, lanes outside 1..64 or a begin or end cell "
                      "outside the band");
        return AGX_E_ARG;
    }
    *out = sp;
    return AGX_OK;
}

int agx_sw_batch_create_align_band_diag_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                              const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    const BandAt at{AGX_SW_ALIGN_SPANS, diag};
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, true, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_cigar")
}

int agx_sw_align_band_diag_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag, const uint8_t *bases,
                                 const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, uint64_t *op_off, uint32_t *ops,
                                 uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_cigar(ctx, scoring, mode, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap); });
}

int agx_sw_batch_create_align_band_diag_matrix_cigar(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int32_t band, const int32_t *diag,
                                                     const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                                     agx_sw_batch **out)
{
    if (!matrix) {
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_band_diag_matrix_cigar: matrix is NULL");
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    const BandAt at{AGX_SW_ALIGN_SPANS, diag};
    return create_band(ctx, nullptr, mode, band, bases, off, len, n_pairs, out, true, &at, matrix);
    AGX_GUARD_END("agx_sw_batch_create_align_band_diag_matrix_cigar")
}

int agx_sw_align_band_diag_matrix_cigar(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int32_t band, const int32_t *diag,
                                        const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                        uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_diag_matrix_cigar(ctx, matrix, mode, band, diag, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap); });
}

int agx_sw_batch_create_align_band_zdrop_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag,
                                               int32_t zdrop, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                                               agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    const BandAt at{AGX_SW_ALIGN_SPANS, diag, true, zdrop};
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, true, &at);
    AGX_GUARD_END("agx_sw_batch_create_align_band_zdrop_cigar")
}

int agx_sw_align_band_zdrop_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const int32_t *diag, int32_t zdrop,
                                  const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits,
                                  int32_t *stops, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_zdrop_cigar(ctx, scoring, mode, band, diag, zdrop, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) {
        const int r = agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap);
        return r || !stops ? r : agx_sw_batch_zdrop_stops(x, stops);
    });
}

int agx_sw_cigar_in_band(const uint32_t *ops, uint64_t n_ops, int32_t dlo, int32_t dhi)
{
    if (!ops && n_ops) return 0;
    return cigar_in_band(ops, n_ops, dlo, dhi) ? 1 : 0;
}

int agx_sw_batch_create_align_band_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases,
                                         const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    return create_band(ctx, scoring, mode, band, bases, off, len, n_pairs, out, true);
    AGX_GUARD_END("agx_sw_batch_create_align_band_cigar")
}

int agx_sw_align_band_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int32_t band, const uint8_t *bases, const uint64_t *off,
                            const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_band_cigar(ctx, scoring, mode, band, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap); });
}

int agx_sw_batch_cigars(agx_sw_batch *b, agx_sw_hit *hits, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    if (!b || !op_off) {
        agx_set_error("agx_sw_batch_cigars: null argument");
        return AGX_E_ARG;
    }
    if (b->cigar != 1 || b->align != AGX_SW_ALIGN_SPANS) {
        agx_set_error("agx_sw_batch_cigars: not a cigar batch (create it with agx_sw_batch_create_align_cigar, agx_sw_batch_create_align_band_cigar, "
                      "agx_sw_batch_create_align_band_diag_cigar, agx_sw_batch_create_align_band_diag_matrix_cigar or "
                      "agx_sw_batch_create_align_band_diag_dual_cigar)");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no CIGARs");
        return AGX_E_NODEVICE;
    }
    AGX_GUARD_BEGIN
    if (!b->cig_valid) {
        const int rc = cigars_impl(b);
        if (rc) return rc;
    }
    const int64_t n = b->n_pairs;
    memcpy(op_off, b->cig_off.data(), ((size_t)n + 1) * sizeof(uint64_t));
    if (hits && n) memcpy(hits, b->cig_hits.data(), (size_t)n * sizeof(agx_sw_hit));
    const uint64_t total = b->cig_off[(size_t)n];
    if (!ops) return AGX_OK; // the sizing call
    if (ops_cap < total) {
        agx_set_error("agx_sw_batch_cigars: ops_cap = %llu, the batch has %llu operations", (unsigned long long)ops_cap, (unsigned long long)total);
        return AGX_E_ARG;
    }
    if (total) memcpy(ops, b->cig_ops.data(), (size_t)total * sizeof(uint32_t));
    return AGX_OK;
    AGX_GUARD_END("agx_sw_batch_cigars")
}

int agx_sw_batch_cigar_info(const agx_sw_batch *b, agx_sw_cigar_info *info)
{
    if (!b || !info) {
        agx_set_error("agx_sw_batch_cigar_info: null argument");
        return AGX_E_ARG;
    }
    if (b->cigar != 1) {
        agx_set_error("agx_sw_batch_cigar_info: not a cigar batch (create it with agx_sw_batch_create_align_cigar)");
        return AGX_E_ARG;
    }
    *info = b->cig_info;
    return AGX_OK;
}

int agx_sw_batch_create_align_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                                    const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    if (scoring && matrix) {
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_cigar: both scoring and matrix given; exactly one way of scoring");
        return AGX_E_ARG;
    }
    return create_align("agx_sw_batch_create_align_cigar", ctx, scoring, matrix, mode, AGX_SW_ALIGN_SPANS, bases, off, len, n_pairs, out, false, true);
}

int agx_sw_align_cigar(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                       const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, uint64_t *op_off, uint32_t *ops, uint64_t ops_cap)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_cigar(ctx, scoring, matrix, mode, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_cigars(x, hits, op_off, ops, ops_cap); });
}

} // extern "C"
