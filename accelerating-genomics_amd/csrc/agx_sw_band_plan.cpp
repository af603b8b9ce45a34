// ------------------------------------------------------------------ the planner of banded batches ("create pipeline")
// The stages of agx_sw_host::create_band (agx_sw_band.cpp) that touch no device, in the order it calls them: each reads what it
// is given and fills a result of its own.  (The wave builder between the sort and the group records, layout_band_waves, is a
// template and so lives in agx_sw_batch.h: it also lays out the chunks of a banded cigar batch, agx_sw_cigar.cpp.)
#include "agx_sw_batch.h"

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

// ---- the arguments, in the order every banded create has checked them (create_band binds the context between the first two)
int check_band_kind(const BandKind &kind)
{
    const char *who = kind.who;
    const BandAt *at = kind.at;
    const int mode = kind.mode;
    const int32_t band = kind.band;
    const bool zd = at && at->zdrop_on;
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
    return AGX_OK;
}

// ... the arrays of the pairs, then the scoring (sc: what the batch is scored with)
int check_band_arrays(const BandKind &kind, const agx_sw_scoring *scoring, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                      agx_sw_scoring &sc)
{
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !len))) {
        agx_set_error("%s: bad arguments (n_pairs=%lld)", kind.who, (long long)n_pairs);
        return AGX_E_ARG;
    }
    if (n_pairs > 0x7fffffffLL / 2) {
        agx_set_error("%s: more than 2^30 pairs in one batch", kind.who);
        return AGX_E_LIMIT;
    }
    const agx_sw_scoring ref_scoring = AGX_SW_SCORING_REFERENCE;
    sc = scoring ? *scoring : ref_scoring;
    if (sc.match < 1 || sc.match > 12 || sc.mismatch > 0 || sc.mismatch < sc.match - 128 || sc.gap_open > 0 || sc.gap_open < -1000 ||
        sc.gap_extend > 0 || sc.gap_extend < -1000) {
        agx_set_error("scoring {match %d, mismatch %d, open %d, extend %d} outside the supported range", sc.match, sc.mismatch, sc.gap_open,
                      sc.gap_extend);
        return AGX_E_LIMIT;
    }
    if (const agx_sw_scoring_dual *d = kind.at ? kind.at->dual : nullptr) // the second piece: the limits of the first
        if (d->gap_open2 > 0 || d->gap_open2 < -1000 || d->gap_extend2 > 0 || d->gap_extend2 < -1000) {
            agx_set_error("scoring {match %d, mismatch %d, open %d, extend %d, open2 %d, extend2 %d} outside the supported range", d->match, d->mismatch,
                          d->gap_open, d->gap_extend, d->gap_open2, d->gap_extend2);
            return AGX_E_LIMIT;
        }
    return AGX_OK;
}

// ---- pass A: limits, band, lane tiling
int plan_band_pairs(const BandKind &kind, const uint8_t *bases, const uint32_t *len, int64_t n_pairs, BandPairs &out)
{
    const BandAt *at = kind.at;
    const int mode = kind.mode;
    const int32_t band = kind.band;
    std::vector<BandPlan> &plan = out.plan;
    if (at) out.row0s.assign((size_t)n_pairs, kNoBandRow);
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
            agx_set_error("%s: bases is NULL", kind.who);
            return AGX_E_ARG;
        }
        BandPlan e{(uint32_t)p, la, (uint32_t)rows, (int32_t)dlo, (int32_t)dhi, 0, 0, (uint32_t)row0};
        if (at) out.row0s[(size_t)p] = (uint32_t)row0;
        int cls = 0, G = 1;
        band_tiling((int)(dhi - dlo + 1), e.lb, cls, G);
        e.cls = (uint8_t)cls;
        e.G = (uint8_t)G;
        plan.push_back(e);
    }
    out.cells = cells;
    return AGX_OK;
}

// ---- sort: class, lanes per group, then rows falling -- the groups of a wave step alike (lb + G).  A total order: the pair
// number breaks the ties, so the plan does not depend on the sort's algorithm
void sort_band_plan(std::vector<BandPlan> &plan)
{
    std::sort(plan.begin(), plan.end(), [](const BandPlan &x, const BandPlan &y) {
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.G != y.G) return x.G < y.G;
        if (x.lb != y.lb) return x.lb > y.lb;
        return x.pair < y.pair;
    });
}

// ---- the group records in plan order, and where the image holds every group's a and b
int write_band_groups(const std::vector<BandPlan> &plan, std::vector<SwBandGroup> &groups, uint64_t &img_dw)
{
    groups.resize(plan.size());
    img_dw = 0;
    for (size_t k = 0; k < plan.size(); ++k) {
        const BandPlan &e = plan[k];
        SwBandGroup &g = groups[k];
        const int K = kSwBandClasses[e.cls], G = e.G;
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
        g.reserved = e.row0; // (the kernels do not read it: build_band_image does)
        if (img_dw > 0xffffffffull) {
            agx_set_error("pair %u: the batch's sequences exceed the 16 GiB a banded batch's image may take", e.pair);
            return AGX_E_LIMIT;
        }
    }
    return AGX_OK;
}

// ---- the image of the groups [lo, hi) into dst, which has img_dw dwords (it touches every byte once: the symbol check rides
// along).  code: under a matrix its byte map -- the image then holds symbol numbers, code + 1, and 0 stays the padding; a byte
// outside the alphabet is written as padding.  -> the first pair of the range, in the caller's order, that breaks the symbol
// rule (a byte 0x00, or under a matrix a byte outside the alphabet, anywhere in a or in b, the rows a band around a diagonal
// leaves out included), or -1
int64_t build_band_image(const std::vector<SwBandGroup> &groups, int64_t lo, int64_t hi, const uint8_t *bases, const uint64_t *off,
                         const uint32_t *len, const uint8_t *code, uint8_t *dst)
{
    int64_t first_bad = -1;
    for (int64_t k = lo; k < hi; ++k) {
        const SwBandGroup &g = groups[(size_t)k];
        const uint32_t la = g.la_lb & 0xffffu, lb = g.la_lb >> 16, lb_all = len[2 * (size_t)g.out + 1];
        const uint8_t *sa = bases + off[2 * (size_t)g.out], *b0 = bases + off[2 * (size_t)g.out + 1], *sb = b0 + g.reserved; // (row0)
        uint8_t *xa = dst + (size_t)g.x_dw * 4, *ya = dst + (size_t)g.y_dw * 4;
        const size_t xbytes = ((size_t)(g.fpad + la + 3) / 4 + 1) * 4, ybytes = ((size_t)(lb + 4) / 4 + 1) * 4;
        memset(xa, 0, g.fpad);
        memset(xa + g.fpad + la, 0, xbytes - g.fpad - la);
        ya[0] = 0;
        memset(ya + 1 + lb, 0, ybytes - 1 - lb);
        bool hit;
        if (code) {
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
            for (uint32_t k = 0; k < lb_all; ++k) miss |= code[b0[k]];
            hit = (miss & 0x80u) != 0;
        } else {
            memcpy(xa + g.fpad, sa, la);
            memcpy(ya + 1, sb, lb);
            hit = memchr(sa, 0, la) || memchr(b0, 0, lb_all);
        }
        if (hit && (first_bad < 0 || (int64_t)g.out < first_bad)) first_bad = g.out;
    }
    return first_bad;
}

} // namespace agx_sw_host
