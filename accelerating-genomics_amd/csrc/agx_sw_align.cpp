// Align batches of the Smith-Waterman path (include/agx.h, "Where the alignment lies" to "Matches and aligned pairs"): their
// create on top of create_batch, the hits with their begin pass, the statistics, and the one-shot calls.
#include "agx_sw_batch.h"

#include "agx_parallel.h"

using namespace agx_sw_host;

extern "C" {

int agx_sw_batch_create_align(agx_ctx *ctx, const agx_sw_scoring *scoring, int what, const uint8_t *bases, const uint64_t *off,
                              const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    return agx_sw_batch_create_align_mode(ctx, scoring, AGX_SW_MODE_LOCAL, what, bases, off, len, n_pairs, out);
}

} // extern "C"

namespace agx_sw_host {
// What a pair with an empty side answers in the modes other than LOCAL (include/agx.h, "Alignment modes"): no cell is
// filled, the boundary formulas are the answer.  D[0][la] = all of a in one gap; GLOBAL with la = 0 the same for b.
agx_sw_hit empty_side_hit(int mode, int what, const agx_sw_scoring &sc, uint32_t la, uint32_t lb)
{
    agx_sw_hit h{0, -1, -1, -1, -1};
    const int gap_a = la ? sc.gap_open + (int)la * sc.gap_extend : 0;
    const int gap_b = lb ? sc.gap_open + (int)lb * sc.gap_extend : 0;
    if (mode == AGX_SW_MODE_EXTEND) return h; // D[0][0] = 0 is the maximum: nothing consumed, all four stay -1
    h.a_end = (int32_t)la - 1;
    if (mode == AGX_SW_MODE_GLOBAL) {
        h.score = gap_a + gap_b; // (one of them is 0)
        h.b_end = (int32_t)lb - 1;
    } else
        h.score = gap_a; // FIT, EXTEND_QUERY: max_i D[i][la] stands at i = 0 (la = 0: D[i][0] <= 0 = D[0][0]; lb = 0: i = 0 only)
    if (what == AGX_SW_ALIGN_SPANS) h.a_begin = h.b_begin = 0;
    return h;
}

// The same under two-piece gap costs (include/agx.h, "Banded alignment around a diagonal under two-piece gap costs"): every formula
// holds one gap, whose cost is the larger of the two pieces' -- the hit of the piece that scores higher; the ends are the same.
agx_sw_hit empty_side_hit_dual(int mode, int what, const agx_sw_scoring_dual &sc, uint32_t la, uint32_t lb)
{
    const agx_sw_hit h1 = empty_side_hit(mode, what, agx_sw_scoring{sc.match, sc.mismatch, sc.gap_open, sc.gap_extend}, la, lb);
    const agx_sw_hit h2 = empty_side_hit(mode, what, agx_sw_scoring{sc.match, sc.mismatch, sc.gap_open2, sc.gap_extend2}, la, lb);
    return h2.score > h1.score ? h2 : h1;
}

// an align batch under match/mismatch scoring (matrix == NULL) or under a substitution matrix (scoring unused)
int create_align(const char *who, agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, int what,
                 const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool stats, bool cigar)
{
    if (mode < AGX_SW_MODE_LOCAL || mode > AGX_SW_MODE_EXTEND_QUERY) {
        if (out) *out = nullptr;
        agx_set_error("%s%s: mode = %d is not one of AGX_SW_MODE_LOCAL .. AGX_SW_MODE_EXTEND_QUERY (0..4)", who, matrix || stats || cigar ? "" : "_mode", mode);
        return AGX_E_ARG;
    }
    if (what != AGX_SW_ALIGN_ENDS && what != AGX_SW_ALIGN_SPANS) {
        if (out) *out = nullptr;
        agx_set_error("%s: what = %d is neither AGX_SW_ALIGN_ENDS nor AGX_SW_ALIGN_SPANS", who, what);
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    agx_sw_batch *b = nullptr;
    // a stats batch: LOCAL and FIT keep the plain forward fill (their begin pass carries L), the pinned modes' only fill carries it
    const int stats_kind = !stats ? 0 : (mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_FIT) ? 1 : 2;
    const int max_query = stats ? AGX_SW_STATS_MAX_QUERY_LEN : cigar ? AGX_SW_CIGAR_MAX_QUERY_LEN : AGX_SW_ALIGN_MAX_QUERY_LEN;
    int rc = create_batch(ctx, scoring, matrix, bases, off, len, n_pairs, &b, false, what, mode, stats_kind, cigar ? 1 : 0);
    if (rc) return rc;
    struct Drop {
        agx_sw_batch *b;
        ~Drop() { agx_sw_batch_destroy(b); } // (create_batch has waited for everything it queued)
    } drop{b};
    if (mode != AGX_SW_MODE_LOCAL)
        for (int64_t p = 0; p < n_pairs; ++p) { // the planner skips pairs with an empty side: their answers come from the formulas
            const uint32_t la = len[2 * p], lb = len[2 * p + 1];
            if (la && lb) continue;
            if (la > (uint32_t)max_query || lb > (uint32_t)AGX_SW_ALIGN_MAX_TARGET_LEN) {
                agx_set_error("pair %lld: lengths %u x %u exceed the supported %d x %d (query x target of an align batch)", (long long)p, la, lb,
                              max_query, AGX_SW_ALIGN_MAX_TARGET_LEN);
                return AGX_E_LIMIT;
            }
            const int32_t v = empty_side_hit(mode, what, b->scoring, la, lb).score;
            if (ctx && v) {
                b->fix_pair.push_back(p);
                b->fix_score.push_back(v);
            }
        }
    if (ctx && n_pairs > 0) b->seq_len.assign(len, len + 2 * n_pairs); // agx_sw_batch_hits checks every end cell against them
    if (ctx && what == AGX_SW_ALIGN_SPANS && n_pairs > 0 && (mode == AGX_SW_MODE_LOCAL || mode == AGX_SW_MODE_FIT || cigar)) {
        // the begin pass (and a cigar batch's traced fill of the spans) reads the sequences again, long after this call: a dense
        // copy of the batch's own
        b->seq_off.resize((size_t)n_pairs * 2);
        uint64_t at = 0;
        for (int64_t k = 0; k < 2 * n_pairs; ++k) {
            b->seq_off[(size_t)k] = at;
            at += len[k];
        }
        b->seq.resize((size_t)at);
        agx_parallel_for(2 * n_pairs, 8192, [&](int64_t lo, int64_t hi, int) {
            for (int64_t k = lo; k < hi; ++k)
                if (len[k]) memcpy(b->seq.data() + b->seq_off[(size_t)k], bases + off[k], len[k]);
        });
    }
    drop.b = nullptr;
    *out = b;
    return AGX_OK;
    AGX_GUARD_END(who)
}
} // namespace agx_sw_host

extern "C" {

int agx_sw_batch_create_align_mode(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, const uint8_t *bases,
                                   const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    return create_align("agx_sw_batch_create_align", ctx, scoring, nullptr, mode, what, bases, off, len, n_pairs, out);
}

int agx_sw_batch_create_align_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, const uint8_t *bases,
                                     const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    if (!matrix) {
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_matrix: matrix is NULL");
        return AGX_E_ARG;
    }
    return create_align("agx_sw_batch_create_align_matrix", ctx, nullptr, matrix, mode, what, bases, off, len, n_pairs, out);
}

} // extern "C"

namespace agx_sw_host {
void reversed_prefixes(const agx_sw_batch *b, const agx_sw_hit *hits, bool fit, int64_t grain, RevPrefixes &r)
{
    r.pick.reserve((size_t)b->n_pairs);
    for (int64_t p = 0; p < b->n_pairs; ++p)
        if (fit ? hits[p].b_end >= 0 : hits[p].score > 0) r.pick.push_back(p);
    const int64_t m = (int64_t)r.pick.size();
    r.off.resize((size_t)m * 2);
    r.len.resize((size_t)m * 2);
    uint64_t at = 0;
    for (int64_t k = 0; k < m; ++k) {
        const agx_sw_hit &h = hits[r.pick[(size_t)k]];
        r.off[(size_t)(2 * k)] = at;
        r.len[(size_t)(2 * k)] = (uint32_t)h.a_end + 1u;
        at += (uint64_t)h.a_end + 1u;
        r.off[(size_t)(2 * k + 1)] = at;
        r.len[(size_t)(2 * k + 1)] = (uint32_t)h.b_end + 1u;
        at += (uint64_t)h.b_end + 1u;
    }
    r.bytes.resize((size_t)at);
    agx_parallel_for(m, grain, [&](int64_t lo, int64_t hi, int) {
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t p = r.pick[(size_t)k];
            for (int side = 0; side < 2; ++side) {
                const uint8_t *src = b->seq.data() + b->seq_off[(size_t)(2 * p + side)];
                uint8_t *dst = r.bytes.data() + r.off[(size_t)(2 * k + side)];
                const uint32_t l = r.len[(size_t)(2 * k + side)];
                for (uint32_t i = 0; i < l; ++i) dst[i] = src[l - 1u - i];
            }
        }
    });
}

// agx_sw_batch_hits; with L (agx_sw_batch_stats) also the word matches << 12 | pairs of every pair, 0 where no fill says
// otherwise: from this batch's own fill (stats == 2), else from the begin pass, which then runs the stats build
int hits_impl(agx_sw_batch *b, agx_sw_hit *hits, std::vector<uint32_t> *L)
{
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    hipStream_t st = agx_enqueue_stream(b->ctx);
    const int64_t n = b->n_pairs;
    if (n == 0) {
        AGX_HIP(hipStreamSynchronize(st));
        return AGX_OK;
    }
    const int32_t *sc = (const int32_t *)b->out_stage.p;
    const uint32_t *en = (const uint32_t *)b->ends_stage.p;
    const bool own_l = L && b->stats == 2;
    AGX_HIP(hipMemcpyAsync(b->out_stage.p, b->scores.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AGX_HIP(hipMemcpyAsync(b->ends_stage.p, b->ends.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (own_l) AGX_HIP(hipMemcpyAsync(b->lstat_stage.p, b->lstat.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    AGX_HIP(hipStreamSynchronize(st));
    if (own_l) L->assign((const uint32_t *)b->lstat_stage.p, (const uint32_t *)b->lstat_stage.p + n);
    else if (L) L->assign((size_t)n, 0u);
    // end cells, checked against the caller's lengths: a padding cell must never be reported
    const uint32_t *len = b->seq_len.empty() ? nullptr : b->seq_len.data(); // (the begin passes' own batches have none: checked against the end cell below)
    const int mode = b->mode;
    const bool spans = b->align == AGX_SW_ALIGN_SPANS;
    std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
    agx_parallel_for(n, 16384, [&](int64_t lo, int64_t hi, int tid) {
        for (int64_t p = lo; p < hi; ++p) {
            agx_sw_hit h{sc[p], -1, -1, -1, -1};
            bool ok;
            if (mode == AGX_SW_MODE_LOCAL) {
                if (en[p] != 0xffffffffu) {
                    h.a_end = (int32_t)(en[p] & ((1u << kSwLocColBits) - 1u));
                    h.b_end = (int32_t)(en[p] >> kSwLocColBits);
                }
                const bool located = en[p] != 0xffffffffu;
                ok = sc[p] >= 0 && located == (sc[p] > 0);
                if (ok && located && len) ok = (uint32_t)h.a_end < len[2 * p] && (uint32_t)h.b_end < len[2 * p + 1];
            } else if (len && (len[2 * p] == 0 || len[2 * p + 1] == 0)) {
                h = empty_side_hit(mode, b->align, b->scoring, len[2 * p], len[2 * p + 1]);
                ok = sc[p] == 0 && en[p] == 0xffffffffu; // no kernel wrote there
            } else {
                // the anchored fill's word: (row + 1) << 12 | (column + 1); 0xffffffff = no kernel wrote the slot
                h.a_end = (int32_t)(en[p] & ((1u << kSwLocColBits) - 1u)) - 1;
                h.b_end = (int32_t)(en[p] >> kSwLocColBits) - 1;
                ok = en[p] != 0xffffffffu;
                const int64_t la = len ? (int64_t)len[2 * p] : -1, lb = len ? (int64_t)len[2 * p + 1] : -1;
                if (mode == AGX_SW_MODE_EXTEND) {
                    ok = ok && sc[p] >= 0 && (sc[p] > 0 ? h.a_end >= 0 && h.b_end >= 0 : h.a_end == -1 && h.b_end == -1);
                    if (ok && len) ok = h.a_end < la && h.b_end < lb;
                } else {
                    ok = ok && h.a_end >= 0 && h.b_end >= -1; // all of a, whatever of b
                    if (ok && len) ok = h.a_end == la - 1 && (mode == AGX_SW_MODE_GLOBAL ? h.b_end == lb - 1 : h.b_end < lb);
                }
                if (ok && spans && !(mode == AGX_SW_MODE_EXTEND && sc[p] == 0)) h.a_begin = h.b_begin = 0; // (FIT: b_begin follows below)
            }
            if (!ok && bad[(size_t)tid] < 0) bad[(size_t)tid] = p;
            hits[p] = h;
        }
    });
    for (int64_t p : bad)
        if (p >= 0) {
            agx_set_error("agx_sw_batch_hits: pair %lld (mode %d): score %d with end cell word 0x%08x is not a cell of its matrix", (long long)p, mode, sc[p], en[p]);
            return AGX_E_INTERNAL;
        }
    if (!spans || (mode != AGX_SW_MODE_LOCAL && mode != AGX_SW_MODE_FIT)) return AGX_OK;
    const bool fit = mode == AGX_SW_MODE_FIT;

    // ---- begin pass.  LOCAL: the same fill over the reversed prefixes a[a_end..0], b[b_end..0] of the pairs with a score.
    // Its end cell, by the same rule, is the latest begin in b, then in a, of an alignment of that score ending in the end
    // cell.  FIT: all of a reversed against b[b_end..0] in mode EXTEND_QUERY -- the smallest reversed end is the latest
    // begin in b (DESIGN.md has both arguments).
    RevPrefixes rev;
    reversed_prefixes(b, hits, fit, 4096, rev);
    const std::vector<int64_t> &pick = rev.pick;
    const int64_t m = (int64_t)pick.size();
    if (m == 0) return AGX_OK;
    agx_sw_batch *rb = nullptr;
    // (a substitution matrix is symmetric and a stays across the lanes: the reversed problem runs under the same matrix)
    rc = create_batch(b->ctx, &b->scoring, b->matrix ? &b->mat : nullptr, rev.bytes.data(), rev.off.data(), rev.len.data(), m, &rb, false, AGX_SW_ALIGN_ENDS,
                      fit ? AGX_SW_MODE_EXTEND_QUERY : AGX_SW_MODE_LOCAL, L ? 2 : 0);
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
    if (!rc) rc = hits_impl(rb, rh.data(), L ? &rl : nullptr);
    if (rc) return rc;
    for (int64_t k = 0; k < m; ++k) {
        agx_sw_hit &h = hits[pick[(size_t)k]];
        const agx_sw_hit &r = rh[(size_t)k];
        if (r.score != h.score || r.a_end < 0 || r.a_end > h.a_end || r.b_end < 0 || r.b_end > h.b_end || (fit && r.a_end != h.a_end)) {
            agx_set_error("agx_sw_batch_hits: pair %lld: the reverse fill from its end cell (a %d, b %d) gives score %d at (a %d, b %d), the forward fill %d",
                          (long long)pick[(size_t)k], h.a_end, h.b_end, r.score, r.a_end, r.b_end, h.score);
            return AGX_E_INTERNAL;
        }
        if (!fit) h.a_begin = h.a_end - r.a_end;
        h.b_begin = h.b_end - r.b_end;
        if (L) (*L)[(size_t)pick[(size_t)k]] = rl[(size_t)k];
    }
    return AGX_OK;
}
} // namespace agx_sw_host

extern "C" {

int agx_sw_batch_hits(agx_sw_batch *b, agx_sw_hit *hits)
{
    if (!b || (!hits && b->n_pairs)) {
        agx_set_error("agx_sw_batch_hits: null argument");
        return AGX_E_ARG;
    }
    if (!b->align) {
        agx_set_error("agx_sw_batch_hits: a score-only batch has no hits (create it with agx_sw_batch_create_align)");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no hits");
        return AGX_E_NODEVICE;
    }
    AGX_GUARD_BEGIN
    if (b->banded) return band_hits(b, hits);
    return hits_impl(b, hits, nullptr);
    AGX_GUARD_END("agx_sw_batch_hits")
}

int agx_sw_batch_stats(agx_sw_batch *b, agx_sw_hit *hits, agx_sw_stat *stats)
{
    if (!b || (!stats && b->n_pairs)) {
        agx_set_error("agx_sw_batch_stats: null argument");
        return AGX_E_ARG;
    }
    if (!b->stats || b->align != AGX_SW_ALIGN_SPANS) {
        agx_set_error("agx_sw_batch_stats: not a stats batch (create it with agx_sw_batch_create_align_stats or "
                      "agx_sw_batch_create_align_band_diag_stats)");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no stats");
        return AGX_E_NODEVICE;
    }
    AGX_GUARD_BEGIN
    const int64_t n = b->n_pairs;
    std::vector<agx_sw_hit> own;
    if (!hits && n) {
        own.resize((size_t)n);
        hits = own.data();
    }
    std::vector<uint32_t> L;
    // (a batch banded around a diagonal: DESIGN.md 4.1m -- its L has wider fields, both lengths reach 65 535)
    const int rc = b->banded ? band_at_hits(b, hits, true, &L) : hits_impl(b, hits, &L);
    if (rc || n == 0) return rc;
    const int bits = b->banded ? kSwBandStatBits : kSwStatColBits;
    // Every stat is checked before it leaves: 0 <= matches <= pairs <= min(columns of a, of b); under match/mismatch scoring
    // what the score leaves after matches, mismatches and gap cells must be a whole number of gap opens, between "one if
    // there is a gap cell" and "one per gap cell".
    const agx_sw_scoring s = b->scoring;
    const bool mm = !b->matrix;
    std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
    agx_parallel_for(n, 16384, [&](int64_t lo, int64_t hi, int tid) {
        for (int64_t p = lo; p < hi; ++p) {
            const agx_sw_hit &h = hits[p];
            const int64_t ca = h.a_begin >= 0 && h.a_end >= h.a_begin ? (int64_t)h.a_end - h.a_begin + 1 : 0;
            const int64_t cb = h.b_begin >= 0 && h.b_end >= h.b_begin ? (int64_t)h.b_end - h.b_begin + 1 : 0;
            const int64_t matches = L[(size_t)p] >> bits, pairs = L[(size_t)p] & ((1u << bits) - 1u);
            bool ok = matches <= pairs && pairs <= std::min(ca, cb);
            if (ok && mm && ca + cb > 0) {
                const int64_t gaps = ca + cb - 2 * pairs;
                const int64_t r = (int64_t)h.score - matches * s.match - (pairs - matches) * s.mismatch - gaps * s.gap_extend;
                if (s.gap_open == 0) ok = r == 0;
                else {
                    const int64_t opens = r / s.gap_open;
                    ok = r % s.gap_open == 0 && opens >= (gaps ? 1 : 0) && opens <= gaps;
                }
            }
            if (!ok && bad[(size_t)tid] < 0) bad[(size_t)tid] = p;
            stats[p] = agx_sw_stat{(int32_t)matches, (int32_t)pairs};
        }
    });
    for (int64_t p : bad)
        if (p >= 0) {
            agx_set_error("agx_sw_batch_stats: pair %lld (mode %d): matches %u, pairs %u do not fit its score %d over the span a %d..%d, b %d..%d",
                          (long long)p, b->mode, L[(size_t)p] >> bits, L[(size_t)p] & ((1u << bits) - 1u), hits[p].score,
                          hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end);
            return AGX_E_INTERNAL;
        }
    return AGX_OK;
    AGX_GUARD_END("agx_sw_batch_stats")
}

int agx_sw_align(agx_ctx *ctx, const agx_sw_scoring *scoring, int what, const uint8_t *bases, const uint64_t *off,
                 const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    return agx_sw_align_mode(ctx, scoring, AGX_SW_MODE_LOCAL, what, bases, off, len, n_pairs, hits);
}

int agx_sw_align_mode(agx_ctx *ctx, const agx_sw_scoring *scoring, int mode, int what, const uint8_t *bases, const uint64_t *off,
                      const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_mode(ctx, scoring, mode, what, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_align_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, int mode, int what, const uint8_t *bases, const uint64_t *off,
                        const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_matrix(ctx, matrix, mode, what, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_hits(x, hits); });
}

int agx_sw_batch_create_align_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                                    const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    if (scoring && matrix) {
        if (out) *out = nullptr;
        agx_set_error("agx_sw_batch_create_align_stats: both scoring and matrix given; exactly one way of scoring");
        return AGX_E_ARG;
    }
    return create_align("agx_sw_batch_create_align_stats", ctx, scoring, matrix, mode, AGX_SW_ALIGN_SPANS, bases, off, len, n_pairs, out, true);
}

int agx_sw_align_stats(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, int mode, const uint8_t *bases,
                       const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_hit *hits, agx_sw_stat *stats)
{
    agx_sw_batch *b = nullptr;
    const int rc = agx_sw_batch_create_align_stats(ctx, scoring, matrix, mode, bases, off, len, n_pairs, &b);
    return rc ? rc : align_once(b, [&](agx_sw_batch *x) { return agx_sw_batch_stats(x, hits, stats); });
}

} // extern "C"
