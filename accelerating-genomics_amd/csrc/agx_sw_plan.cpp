// The host planner of the Smith-Waterman path: the tiling tables, the plan of a uniform batch and of a mixed one (passes B and C of
// agx_sw.cpp's head comment), the layout of waves, launches and image offsets (pass D) and the record writers.  create_batch
// (agx_sw.cpp) calls these stage by stage; every stage reads what it is given and returns what it made.
#include "agx_sw_batch.h"

#include <cmath>
#include <mutex>

#include "agx_parallel.h"

namespace agx_sw_host {

namespace {

// Tuning build only (see agx_tune): AGX_SW_TAIL_BETA, AGX_SW_MAX_C, AGX_SW_FORCE_C, AGX_SW_MAX_CLASSES,
// AGX_SW_WAVES_PER_CLASS, AGX_SW_SORT_WAVES, AGX_SW_KERNEL.  The shipped library runs on the defaults.
bool positive(long n) { return n > 0; }
bool at_least_4(long n) { return n >= 4; }
int max_cols_per_lane() { static const int v = (int)agx_knob_int(agx_tune("AGX_SW_MAX_C"), AGX_SW_MAX_COLS_PER_LANE, at_least_4); return v; }
int force_cols_per_lane() { static const int v = (int)agx_knob_int(agx_tune("AGX_SW_FORCE_C"), 0); return v; }

// Lane time a pair costs under tiling (class ci, G): steps * C * 64 / floor(64 / G) padded cells (the
// lanes of a wave that cannot host another group are charged to the pair), weighted by the measured
// per-cell cost of the class.  beta: lanes' worth of extra weight on a wave's own duration (steps * C),
// which favours spreading long pairs over more lanes; 0 in the throughput regime.
inline double tiling_slope(const double *costs, int ci, int G, double beta)
{
    return kSwClasses[ci] * ((64.0 / (double)(64 / G)) * costs[ci] + beta);
}

// present[lx] != 0: some pair of the batch has that shorter length (only those rows are built)
void build_tiling_table(TilingTable &tt, const std::vector<uint8_t> &present, const double *costs, uint32_t allowed, double beta)
{
    const uint32_t n_lx = (uint32_t)present.size();
    std::vector<std::vector<TilingSeg>> rows(n_lx);
    agx_parallel_for((int64_t)n_lx, 64, [&](int64_t lo, int64_t hi, int) {
        for (int64_t lx = std::max<int64_t>(lo, 1); lx < hi; ++lx) {
            if (!present[(size_t)lx]) continue;
            struct Line {
                int ci, G;
                double w;
            } ln[kSwNumClasses];
            int n = 0;
            for (int ci = 0; ci < kSwNumClasses; ++ci) {
                if (!((allowed >> ci) & 1u)) continue;
                const int C = kSwClasses[ci];
                const int G = ((int)lx + C - 1) / C;
                if (G > 64) continue;
                if (C > max_cols_per_lane() && n > 0) continue;
                if (force_cols_per_lane() && C != force_cols_per_lane()) continue;
                if (costs[ci] == 0) continue; // class not built for this kernel
                ln[n++] = Line{ci, G, tiling_slope(costs, ci, G, beta)};
            }
            if (n == 0) continue;
            auto cost_at = [&](int k, double ly) { return (ly + ln[k].G - 1) * ln[k].w; };
            // start at ly = lx (the longer side is never shorter); ties go to the wider class
            int cur = 0;
            for (int k = 1; k < n; ++k)
                if (cost_at(k, (double)lx) <= cost_at(cur, (double)lx)) cur = k;
            uint32_t from = (uint32_t)lx;
            std::vector<TilingSeg> &row = rows[(size_t)lx];
            for (;;) {
                row.push_back(TilingSeg{from, (uint8_t)ln[cur].ci, (uint8_t)ln[cur].G, ln[cur].w});
                // the next line to undercut the current one: smaller slope, first ly where it is strictly cheaper
                int nxt = -1;
                double nxt_at = 0;
                for (int k = 0; k < n; ++k) {
                    if (!(ln[k].w < ln[cur].w)) continue;
                    const double x = ((ln[k].G - 1) * ln[k].w - (ln[cur].G - 1) * ln[cur].w) / (ln[cur].w - ln[k].w);
                    double at = std::floor(x) + 1;
                    if (at <= (double)from) at = (double)from + 1;
                    if (nxt < 0 || at < nxt_at || (at == nxt_at && ln[k].w < ln[nxt].w)) {
                        nxt = k;
                        nxt_at = at;
                    }
                }
                if (nxt < 0 || nxt_at > 65535.0) break;
                cur = nxt;
                from = (uint32_t)nxt_at;
            }
        }
    });
    tt.first.assign((size_t)n_lx + 1, 0);
    tt.segs.clear();
    for (uint32_t lx = 0; lx < n_lx; ++lx) {
        tt.first[lx] = (uint32_t)tt.segs.size();
        tt.segs.insert(tt.segs.end(), rows[lx].begin(), rows[lx].end());
    }
    tt.first[n_lx] = (uint32_t)tt.segs.size();
}

// Uniform batches (most pairs share one shape, e.g. fixed-length reads): every wave of that shape
// costs the same, so the launch lasts ceil(waves / SIMDs) wave-times -- the tiling is chosen for the
// whole shape with that quantisation instead of pair by pair.
Tiling choose_tiling_uniform(const double *costs, int slots, int lx, int ly, int64_t count, int n_simd)
{
    Tiling best{-1, 0};
    double best_cost = 0;
    for (int ci = 0; ci < kSwNumClasses; ++ci) {
        const int C = kSwClasses[ci];
        const int G = (lx + C - 1) / C;
        if (G > 64) continue;
        if (C > max_cols_per_lane() && best.cls >= 0) continue;
        if (force_cols_per_lane() && C != force_cols_per_lane()) continue;
        const int64_t per_wave = (int64_t)(64 / G) * slots;
        const int64_t waves = (count + per_wave - 1) / per_wave;
        const int64_t rounds = (waves + n_simd - 1) / n_simd;
        const double wgt = costs[ci];
        if (wgt == 0) continue;
        const double c = (double)rounds * (ly + G - 1) * C * wgt;
        if (best.cls < 0 || c < best_cost) {
            best = Tiling{ci, G};
            best_cost = c;
        }
    }
    return best;
}

// a tiling the kernels of this batch can run (the matrix kernels have no class beyond 40 columns per lane)
inline bool runnable(const Tiling &tl, bool matrix) { return tl.cls >= 0 && !(matrix && kSwClasses[tl.cls] > 40); }

inline uint32_t shape_of(const PairPlan &pp) { return pp.lx() << 16 | (pp.ly & 0xffffu); }

// every pair of shape `want` (all of them: want = none) gets tiling tl
void retile_shape(std::vector<PairPlan> &all, int64_t grain, const uint32_t *want, Tiling tl)
{
    agx_parallel_for((int64_t)all.size(), grain, [&](int64_t lo, int64_t hi, int) {
        for (int64_t p = lo; p < hi; ++p) {
            PairPlan &pp = all[(size_t)p];
            if (want && !(pp.cls != kClsEmpty && shape_of(pp) == *want)) continue;
            pp.cls = (uint8_t)tl.cls;
            pp.G = (uint8_t)tl.G;
        }
    });
}

// ---- pass B.  What one tiling of the whole batch reads, and what it leaves per thread for the batch-level rules
struct alignas(128) TileSums { // a cache line pair of its own: every thread adds to its part per pair
    int rc = AGX_OK;
    int64_t bad_pair = -1;
    double waves = 0;
    double class_work[kSwNumClasses] = {};
};
struct TilePass {
    std::vector<PairPlan> &all;
    const std::vector<uint8_t> &present;
    const KernelChoice &kc;
    bool matrix;
    TilingTable tt;
    std::vector<TileSums> sums; // one per pool thread, added up in thread order
    double waves_est() const
    {
        double w = 0;
        for (const TileSums &s : sums) w += s.waves;
        return w;
    }
};

// Tiles every pair among the `allowed` classes with tail term beta.  only_outside: a pair whose class is allowed keeps it.
void tile_all(TilePass &t, uint32_t allowed, double beta, bool only_outside)
{
    build_tiling_table(t.tt, t.present, t.kc.costs, allowed, beta);
    t.sums.assign((size_t)agx_host_threads(), TileSums{});
    const double *costs = t.kc.costs;
    const int slots = t.kc.slots;
    const bool matrix = t.matrix;
    const TilingTable &tt = t.tt;
    std::vector<PairPlan> &all = t.all;
    agx_parallel_for((int64_t)all.size(), 8192, [&](int64_t lo, int64_t hi, int tid) {
        TileSums &me = t.sums[(size_t)tid];
        for (int64_t p = lo; p < hi; ++p) {
            PairPlan &pp = all[(size_t)p];
            if (pp.cls == kClsEmpty) continue;
            Tiling tl;
            double cost = 0;
            const bool keep_own = only_outside && pp.cls < kSwNumClasses && ((allowed >> pp.cls) & 1u);
            if (!keep_own && tt.pick(pp.lx(), pp.ly, &tl, &cost) && !(matrix && kSwClasses[tl.cls] > 40)) {
                pp.cls = (uint8_t)tl.cls;
                pp.G = (uint8_t)tl.G;
            } else if (pp.cls == kClsUntiled) { // no class spans this pair (cannot happen within the limits)
                if (me.rc == AGX_OK) {
                    me.rc = AGX_E_LIMIT;
                    me.bad_pair = p;
                }
                continue;
            } else // keeps the class it has
                cost = (double)(pp.ly + pp.G - 1) * tiling_slope(costs, pp.cls, pp.G, beta);
            me.class_work[pp.cls] += cost;
            me.waves += (double)pp.G / 64.0 / slots;
        }
    });
}

// Tail regime: when the planned waves fill the chip's resident capacity (about 5 per SIMD for this
// kernel) less than 1.6 times, a launch lasts as long as its longest waves -- alone on their SIMDs
// in a small batch, or stranded in a mostly empty second filling.  Such a batch is re-tiled with a
// term on a wave's own duration (3 lanes' worth; more the emptier the chip): long pairs spread over
// more lanes, waves get shorter and more numerous (tools/sw_tail_beta_sweep.py, sw_tail_rule_check.py:
// mixed 32..512 pairs, 8192 pairs 1.24 -> 2.6 TCUPS, 16 384 2.46 -> 2.9, 131 072 4.15 -> 4.61).  Beyond
// 1.6 fillings the term costs 1-3 % and is left out.  (Uniform batches are re-tiled below with their
// own wave-count model.)
void tail_rule(TilePass &t, int n_cu, double *beta_used)
{
    if (!(tail_beta_override() < 0 && n_cu > 0)) return;
    const double fill = t.waves_est() / (5.0 * 4.0 * n_cu);
    // (the biased packed fill runs two waves per SIMD, and with its round-2b cell the term pays up to 1.2 of ITS
    // fillings = 0.48 of these: 45 056 mixed pairs 6.5 -> 7.2 TCUPS, 49 152 7.15 -> 7.26, but 57 344 7.74 -> 7.55 and
    // 65 536 8.07 -> 7.71 -- tools/sw_tail_rule_check.py)
    if (fill < (t.kc.coded_plan ? 0.48 : 1.6)) {
        *beta_used = fill < 0.1 ? 10.0 : fill < 0.4 ? 6.0 : 3.0;
        tile_all(t, ~0u, *beta_used, false);
    }
}

// Every class is its own launch and the measured cost curve is flat over many widths: a mixed batch
// keeps the classes that carry most of the work -- about one per 4096 wavefronts, at most 6
// (tools/sw_mixed_sweep.py: 16384 pairs of 32..512 went from 0.63 to 2.5 TCUPS, 65536 from 2.1 to 3.9) --
// and re-tiles the other pairs among them (a pair no kept class can span keeps its own).
void consolidate_classes(TilePass &t, double beta_used)
{
    double work[kSwNumClasses] = {};
    double waves_est = 0;
    for (const TileSums &s : t.sums) {
        waves_est += s.waves;
        for (int c = 0; c < kSwNumClasses; ++c) work[c] += s.class_work[c];
    }
    static const double per_class = agx_knob_real(agx_tune("AGX_SW_WAVES_PER_CLASS"), 4096.0, [](double v) { return v > 0; });
    // The biased packed kernel runs every class in ONE launch (sw_fill_pk2_any), so from about two wavefronts
    // per SIMD on it keeps them all: padding shrinks (useful cells 0.908 -> 0.932 on config 4's per-GPU shard)
    // and nothing is forked or joined: 131 072 mixed pairs 5.62 -> 6.02 TCUPS, 262 144 6.05 -> 6.39, 65 536
    // 5.48 -> 5.81.  Smaller batches are in the tail regime, where the launch lasts as long as its longest
    // waves and the few-classes rule still wins (16 384 pairs: 3.58 against 3.02 TCUPS; tools/sw_mixed_check.py).
    const int k_max = max_classes_override()                      ? std::min(max_classes_override(), 1 + (int)(waves_est / per_class))
                      : t.kc.coded_plan && waves_est >= 2048.0 ? kSwNumClasses
                                                                  : std::min(6, 1 + (int)(waves_est / per_class));
    int used = 0;
    for (int c = 0; c < kSwNumClasses; ++c) used += work[c] > 0;
    if (used > k_max) {
        int order[kSwNumClasses];
        for (int c = 0; c < kSwNumClasses; ++c) order[c] = c;
        std::sort(order, order + kSwNumClasses, [&](int x, int y) { return work[x] > work[y]; });
        uint32_t keep = 0;
        for (int k = 0; k < k_max; ++k) keep |= 1u << order[k];
        tile_all(t, keep, beta_used, true);
    }
}

// dominant shape?  (sampled first, counted only if the sample says so): at least half of the pairs share one shape, which is
// then tiled as a uniform batch of that many pairs would be
void dominant_shape_rule(std::vector<PairPlan> &all, int n_cu, const KernelChoice &kc, bool matrix)
{
    const int64_t n_pairs = (int64_t)all.size();
    if (!(n_pairs >= 1024 && n_cu > 0)) return;
    uint32_t cand = 0;
    const int votes = sampled_majority_shape((size_t)n_pairs, (size_t)n_pairs / 512, [&](size_t p, uint32_t *sh) {
        *sh = shape_of(all[p]);
        return all[p].cls != kClsEmpty;
    }, &cand);
    if (votes <= 0) return;
    std::vector<int64_t> part((size_t)agx_host_threads(), 0);
    agx_parallel_for(n_pairs, 16384, [&](int64_t lo, int64_t hi, int tid) {
        int64_t c = 0;
        for (int64_t p = lo; p < hi; ++p) c += all[(size_t)p].cls != kClsEmpty && shape_of(all[(size_t)p]) == cand;
        part[(size_t)tid] = c;
    });
    int64_t count = 0;
    for (int64_t c : part) count += c;
    if (count * 2 < n_pairs) return;
    const Tiling tl = choose_tiling_uniform(kc.costs, kc.slots, (int)(cand >> 16), (int)(cand & 0xffffu), count, 4 * n_cu);
    if (runnable(tl, matrix)) retile_shape(all, 16384, &cand, tl);
}

// ---- pass C: order = class, then lanes per group (wide first), then long rows first, then file
// order; waves end up homogeneous and the longest waves of a launch are dispatched first.
// Two stable counting passes (LSD): by ly descending, then by (class, G descending); pairs with an
// empty side sort into a trailing bucket and are dropped.
void sort_plan(std::vector<PairPlan> &all, uint32_t longest_long, std::vector<PairPlan> &plan)
{
    std::vector<PairPlan> tmp;
    counting_sort(all, tmp, (size_t)longest_long + 2, [&](const PairPlan &pp) { return (size_t)(longest_long + 1 - pp.ly); });
    std::vector<PairPlan>().swap(all);
    const size_t n_buckets = (size_t)kSwNumClasses * 64;
    counting_sort(tmp, plan, n_buckets + 1, [&](const PairPlan &pp) {
        return pp.cls == kClsEmpty ? n_buckets : (size_t)pp.cls * 64 + (size_t)(64 - pp.G);
    });
    while (!plan.empty() && plan.back().cls == kClsEmpty) plan.pop_back();
}

// a (class, G) bucket behind the groups and waves counted so far: entry j is slot j % slots of group j / slots, a wave
// takes 64 / G groups
inline void place_bucket(Bucket &q, int slots, size_t &n_groups, size_t &n_waves)
{
    q.group0 = n_groups;
    q.n_groups = (q.count + slots - 1) / slots;
    n_groups += q.n_groups;
    q.wave0 = n_waves;
    const size_t per_wave = (size_t)(64 / q.G);
    q.n_waves = (q.n_groups + per_wave - 1) / per_wave;
    n_waves += q.n_waves;
}

// image offsets: [x block][y block] per entry in plan order, after the zero block vacant slots point at
int image_offsets(const std::vector<PairPlan> &plan, size_t img0, PlanLayout &lay)
{
    lay.x_dw.resize(plan.size());
    lay.y_dw.resize(plan.size());
    std::vector<uint32_t> &x_dw = lay.x_dw, &y_dw = lay.y_dw;
    const int parts = (int)std::min<int64_t>(agx_host_threads(), std::max<int64_t>(1, (int64_t)plan.size() / 16384));
    std::vector<size_t> part_sum((size_t)parts + 1, 0);
    const size_t chunk = (plan.size() + parts - 1) / (size_t)parts;
    auto words = [&](const PairPlan &pp, size_t *xw) {
        *xw = ((size_t)pp.G * kSwClasses[pp.cls] + 3) / 4 + 1;
        return *xw + ((size_t)pp.ly + 3) / 4;
    };
    agx_pool_run(parts, [&](int t) {
        const size_t lo = std::min(plan.size(), (size_t)t * chunk), hi = std::min(plan.size(), lo + chunk);
        size_t s = 0, xw;
        for (size_t i = lo; i < hi; ++i) s += words(plan[i], &xw);
        part_sum[(size_t)t + 1] = s;
    });
    for (int t = 0; t < parts; ++t) part_sum[(size_t)t + 1] += part_sum[(size_t)t];
    lay.img_dw = img0 + part_sum[(size_t)parts];
    if (lay.img_dw > 0xffffffffull) {
        agx_set_error("packed image exceeds 16 GiB; split the batch");
        return AGX_E_LIMIT;
    }
    agx_pool_run(parts, [&](int t) {
        const size_t lo = std::min(plan.size(), (size_t)t * chunk), hi = std::min(plan.size(), lo + chunk);
        size_t at = img0 + part_sum[(size_t)t], xw;
        for (size_t i = lo; i < hi; ++i) {
            const size_t tot = words(plan[i], &xw);
            x_dw[i] = (uint32_t)at;
            y_dw[i] = (uint32_t)(at + xw);
            at += tot;
        }
    });
    return AGX_OK;
}

} // namespace

double tail_beta_override() { static const double v = agx_knob_real(agx_tune("AGX_SW_TAIL_BETA"), -1.0); return v; }
int max_classes_override() { static const int v = (int)agx_knob_int(agx_tune("AGX_SW_MAX_CLASSES"), 0, positive); return v; }

const double *class_costs(int family) // 0 int32, 1 packed signed, 2 packed biased, 3 int32 on the packed plan's coded image, 4 locating int32, 5 anchored int32
{
    // (the locating fill is the int32 cell plus a per-step scan: the int32 kernel's relative costs, no wide classes)
    return family == 0 ? kSwClassCost : family == 1 ? kSwPkClassCost : family >= 3 ? kSwI32dClassCost : kSwPk2ClassCost;
}

const TilingTable &full_tiling_table(int family)
{
    static TilingTable tabs[4];
    static std::once_flag once[4];
    std::call_once(once[family], [family] {
        const std::vector<uint8_t> present((size_t)(family == 0 ? AGX_SW_MAX_SHORT_LEN : kSwPackedMaxShort) + 1, 1);
        build_tiling_table(tabs[family], present, class_costs(family), ~0u, 0.0);
    });
    return tabs[family];
}

// ---- uniform batches (fixed-length reads: BASELINE config 2): one shape, so one tiling -- chosen with the
// wave-count quantisation above -- and nothing to sort: file order is already the order passes B and C
// would produce.
bool plan_uniform(std::vector<PairPlan> &all, uint32_t shape, int n_cu, const KernelChoice &kc, bool matrix, std::vector<PairPlan> &plan)
{
    const Tiling tl = choose_tiling_uniform(kc.costs, kc.slots, (int)(shape >> 16), (int)(shape & 0xffffu), (int64_t)all.size(), 4 * n_cu);
    if (!runnable(tl, matrix)) return false;
    retile_shape(all, 32768, nullptr, tl);
    plan.swap(all);
    return true;
}

// ---- pass B: lane tiling per pair, then the batch-level rules; pass C: the sorts
int plan_host(std::vector<PairPlan> &all, const std::vector<uint8_t> &present, uint32_t longest_long, int n_cu, const KernelChoice &kc, bool matrix,
              std::vector<PairPlan> &plan, double *t_plan)
{
    TilePass t{all, present, kc, matrix, {}, {}};
    double beta_used = tail_beta_override() >= 0 ? tail_beta_override() : 0.0;
    tile_all(t, ~0u, beta_used, false);
    for (const TileSums &s : t.sums)
        if (s.rc != AGX_OK) {
            agx_set_error("pair %lld: no lane tiling fits its %u columns", (long long)s.bad_pair, all[(size_t)s.bad_pair].lx());
            return s.rc;
        }
    tail_rule(t, n_cu, &beta_used);
    consolidate_classes(t, beta_used);
    dominant_shape_rule(all, n_cu, kc, matrix);
    *t_plan = agx_now_ms();
    sort_plan(all, longest_long, plan);
    return AGX_OK;
}

PlanLayout layout_from_buckets(const std::vector<uint32_t> &hist, int slots, uint32_t *bt, size_t *entries)
{
    PlanLayout lay;
    size_t n_entries = 0;
    for (int k = 0; k < kSwPlanBuckets; ++k) { // ascending bucket id = the sort order
        Bucket q;
        q.first = n_entries;
        q.count = hist[(size_t)k];
        q.cls = k >> 6;
        q.G = 64 - (k & 63);
        place_bucket(q, slots, lay.n_groups, lay.n_waves_total);
        bt[5 * k + 0] = (uint32_t)q.first;
        bt[5 * k + 1] = (uint32_t)q.count;
        bt[5 * k + 2] = (uint32_t)q.group0;
        bt[5 * k + 3] = (uint32_t)q.n_groups;
        bt[5 * k + 4] = (uint32_t)q.wave0;
        n_entries += q.count;
        if (q.count) lay.launched_classes |= 1u << q.cls;
    }
    *entries = n_entries;
    lay.groups_bytes = lay.n_groups * sizeof(SwGroup2);
    lay.waves_bytes = lay.n_waves_total * sizeof(SwWave);
    const uint32_t class_mask = lay.launched_classes;
    ClassLaunch cl; // several classes: ONE launch, the class read per wave (sw_fill_pk2_any); else that class's own fill
    cl.C = (class_mask & (class_mask - 1)) ? 0 : kSwClasses[__builtin_ctz(class_mask)];
    cl.first_wave = 0;
    cl.n_waves = (uint32_t)lay.n_waves_total;
    lay.launches.assign(1, cl);
    return lay;
}

// ---- pass D: every (class, G) bucket is regular, so waves, records and offsets need no scan but the
// prefix sum of the image words.
int layout_from_plan(const std::vector<PairPlan> &plan, const KernelChoice &kc, size_t img0, PlanLayout &lay)
{
    const int slots = kc.slots;
    std::vector<Bucket> &bk = lay.buckets;
    for (size_t i = 0; i < plan.size();) {
        Bucket q;
        q.first = i;
        q.cls = plan[i].cls;
        q.G = plan[i].G;
        size_t lo = i, hi = plan.size(); // the run's end by bisection (equal keys are contiguous)
        while (lo + 1 < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (plan[mid].cls == q.cls && plan[mid].G == q.G) lo = mid;
            else hi = mid;
        }
        q.count = lo + 1 - i;
        i = lo + 1;
        bk.push_back(q);
    }
    size_t n_waves = 0;
    for (Bucket &q : bk) place_bucket(q, slots, lay.n_groups, n_waves);
    std::vector<SwWave> &waves = lay.waves;
    std::vector<ClassLaunch> &launches = lay.launches;
    waves.assign(n_waves, SwWave{});
    for (const Bucket &q : bk) {
        if (launches.empty() || launches.back().C != kSwClasses[q.cls]) {
            ClassLaunch cl;
            cl.C = kSwClasses[q.cls];
            cl.first_wave = (uint32_t)q.wave0;
            launches.push_back(cl);
            lay.launched_classes |= 1u << q.cls;
        }
        launches.back().n_waves += (uint32_t)q.n_waves;
        const size_t per_wave = (size_t)(64 / q.G);
        for (size_t wl = 0; wl < q.n_waves; ++wl) {
            SwWave w{};
            w.first_group = (uint32_t)(q.group0 + wl * per_wave);
            w.n_groups = (uint16_t)std::min(per_wave, q.n_groups - wl * per_wave);
            w.G = (uint16_t)q.G;
            w.steps = plan[q.first + wl * per_wave * slots].ly + (uint32_t)q.G - 1u; // rows are sorted long first
            w.reserved = (uint32_t)kSwClasses[q.cls];
            waves[q.wave0 + wl] = w;
            lay.padded += (int64_t)w.steps * 64 * kSwClasses[q.cls] * slots;
        }
    }
    // dispatch order = longest waves first (a wave lasts steps x C; C is the class's): the buckets were
    // filled widest group first, which leaves narrow groups with long rows for the end of the launch
    static const bool sort_waves = [] {
        const char *e = agx_tune("AGX_SW_SORT_WAVES");
        return !(e && e[0] == '0');
    }();
    // A mixed batch of the biased packed kernel is ONE launch (sw_fill_pk2_any): all its waves in one list,
    // longest first across the classes.
    static const bool one_launch_ok = [] {
        const char *e = agx_tune("AGX_SW_ONE_LAUNCH");
        return !(e && e[0] == '0');
    }();
    if (kc.coded_plan && launches.size() > 1 && one_launch_ok) {
        if (sort_waves)
            std::stable_sort(waves.begin(), waves.end(), [](const SwWave &a, const SwWave &b) {
                return (uint64_t)a.steps * a.reserved > (uint64_t)b.steps * b.reserved;
            });
        ClassLaunch all_classes;
        all_classes.C = 0; // 0 = every class, read per wave
        all_classes.first_wave = 0;
        all_classes.n_waves = (uint32_t)waves.size();
        launches.assign(1, all_classes);
    } else if (sort_waves && !launches.empty())
        agx_pool_run((int)launches.size(), [&](int k) {
            const ClassLaunch &cl = launches[(size_t)k];
            std::stable_sort(waves.begin() + cl.first_wave, waves.begin() + cl.first_wave + cl.n_waves,
                             [](const SwWave &a, const SwWave &b) { return a.steps > b.steps; });
        });
    const int rc = image_offsets(plan, img0, lay);
    if (rc) return rc;
    lay.groups_bytes = lay.n_groups * (kc.packed ? sizeof(SwGroup2) : sizeof(SwGroup));
    lay.waves_bytes = waves.size() * sizeof(SwWave);
    lay.n_waves_total = waves.size();
    return AGX_OK;
}

// ---- group records (straight into pinned staging when there is a device)
void write_group_records(const PlanLayout &lay, const std::vector<PairPlan> &plan, const KernelChoice &kc, int64_t n_pairs, void *groups_data)
{
    const int slots = kc.slots;
    const bool packed = kc.packed;
    const std::vector<uint32_t> &x_dw = lay.x_dw, &y_dw = lay.y_dw;
    for (const Bucket &q : lay.buckets)
        agx_parallel_for((int64_t)q.n_groups, 8192, [&](int64_t a, int64_t z, int) {
            for (int64_t g = a; g < z; ++g)
                for (int h = 0; h < slots; ++h) {
                    const size_t j = (size_t)g * slots + h;
                    uint32_t xd = 0, yd = 0, ll = 0, outi = (uint32_t)n_pairs; // vacant slot: zero block, spare score
                    if (j < q.count) {
                        const PairPlan &pp = plan[q.first + j];
                        xd = x_dw[q.first + j];
                        yd = y_dw[q.first + j];
                        ll = (uint32_t)pp.lxo | (pp.ly << 16);
                        outi = pp.pair;
                    }
                    if (packed) {
                        SwGroup2 &r = reinterpret_cast<SwGroup2 *>(groups_data)[q.group0 + (size_t)g];
                        r.x_dw[h] = xd;
                        r.y_dw[h] = yd;
                        r.lx_ly[h] = ll;
                        r.out[h] = outi;
                    } else
                        reinterpret_cast<SwGroup *>(groups_data)[q.group0 + (size_t)g] = SwGroup{xd, yd, ll, outi};
                }
        });
}

// the traced fill (cigar == 2): every group's directions behind one another, in group order (one pair per group)
void write_trace_records(const PlanLayout &lay, const std::vector<PairPlan> &plan, int64_t n_pairs, agx_sw_batch *b)
{
    b->tr_goff.assign(lay.n_groups, 0);
    b->tr_walk.assign((size_t)n_pairs, SwWalkRec{});
    uint64_t at = 0;
    for (const Bucket &q : lay.buckets)
        for (size_t g = 0; g < q.n_groups; ++g) {
            const PairPlan &pp = plan[q.first + g];
            const int C = kSwClasses[q.cls];
            b->tr_goff[q.group0 + g] = at;
            SwWalkRec &r = b->tr_walk[pp.pair];
            r.goff = at;
            r.x_dw = lay.x_dw[q.first + g];
            r.y_dw = lay.y_dw[q.first + g];
            r.ca = pp.lx();
            r.cb = pp.ly;
            r.G = (uint16_t)q.G;
            r.C = (uint16_t)C;
            at += sw_trace_dwords(q.G, pp.ly, C);
        }
    b->tr_dwords = at;
    uint64_t words = 0;
    for (SwWalkRec &r : b->tr_walk) {
        r.slot = words;
        words += (uint64_t)r.ca + r.cb;
    }
    b->tr_slot_words = words;
}

} // namespace agx_sw_host
