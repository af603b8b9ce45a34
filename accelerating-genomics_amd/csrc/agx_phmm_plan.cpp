// The PairHMM planner: from the pairs of a batch to lane tilings, waves and records for one kernel family.  make_plan, at the
// end of this file, is a driver over the stages above it, in the order it calls them; each stage reads what it is given and
// fills a result of its own.
#include "agx_phmm_host.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <unordered_map>

#include "agx_parallel.h"

// (hidden here too: a definition takes its visibility from the namespace block it stands in)
namespace agx_phmm_host __attribute__((visibility("hidden"))) {

ClassTable class_table(int kind)
{
    if (kind == 3) return ClassTable{kPhPkClasses, kPhPkClassCost, kPhPkNumClasses};
    return ClassTable{kPhClasses, kPhClassCost[kind], kPhNumClasses};
}

PhGroup make_group(uint32_t hap_dw, const Plan &p, uint32_t tab)
{
    PhGroup g{};
    g.hap_dw = hap_dw;
    g.H = p.H;
    g.R_tab = p.R | (tab << 16);
    g.out = p.out;
    g.init64 = DBL_MAX / 16 / (double)p.H;
    g.init32 = FLT_MAX / 16 / (float)p.H;
    return g;
}

int check_lds(size_t largest, size_t named)
{
    if (largest <= 160 * 1024) return AGX_OK;
    agx_set_error("a read table of %zu bytes does not fit the 160 KiB LDS", named);
    return AGX_E_LIMIT;
}

Fnv1a plan_hash(int kind, int slots, const PlanOut &po, const std::vector<ClassLaunch> &launches)
{
    Fnv1a f;
    f.field((int32_t)kind), f.field((int32_t)slots), f.field((uint8_t)po.trains), f.field((uint8_t)po.file_order);
    f.field(po.padded);
    for (const ClassLaunch &cl : launches)
        f.field((int32_t)cl.C), f.field((uint8_t)cl.all_g16), f.field(cl.first_wave), f.field(cl.n_waves), f.field((uint64_t)cl.lds), f.field((uint64_t)cl.lds_rescue);
    for (const PhWave &w : po.waves) f.field(w.first_group), f.field(w.first_tab), f.field(w.n_groups), f.field(w.n_tabs), f.field(w.G), f.field(w.reserved), f.field(w.steps);
    for (const PhTab &t : po.tabs) f.field(t.read_dw), f.field(t.R);
    for (const PhGroup &g : po.groups1) f.field(g.hap_dw), f.field(g.H), f.field(g.R_tab), f.field(g.out), f.field(g.init64), f.field(g.init32), f.field(g.reserved);
    for (const PhGroup2 &g : po.groups2) {
        for (int k = 0; k < 2; ++k) f.field(g.hap_dw[k]), f.field(g.H[k]), f.field(g.out[k]), f.field(g.init32[k]), f.field(g.out2[k]);
        f.field(g.R_tab), f.field(g.R2);
    }
    return f;
}

namespace {

// LDS bytes a wave may spend on several read tables (8 waves/CU fit 160 KiB); AGX_PHMM_TAB_BUDGET overrides (experiments)
bool positive(long n) { return n > 0; }
size_t tab_budget() { static const size_t v = (size_t)agx_knob_int(agx_tune("AGX_PHMM_TAB_BUDGET"), 20 * 1024, positive); return v; }

// Tuning knob for experiments (not part of the ABI): AGX_PHMM_MAX_C caps the columns per lane.
int max_cols_per_lane()
{
    static const int v = (int)agx_knob_int(agx_tune("AGX_PHMM_MAX_C"), kPhClasses[kPhNumClasses - 1], [](long n) { return n >= 4; });
    return v;
}

// AGX_PHMM_FORCE_C pins the class (calibration runs only); a class table without that width
// ignores it (e.g. the double rescue plan of a packed float batch forced to an odd width).
int force_cols_per_lane_raw() { static const int v = (int)agx_knob_int(agx_tune("AGX_PHMM_FORCE_C"), 0); return v; }

int force_cols_per_lane(const ClassTable &ct)
{
    const int f = force_cols_per_lane_raw();
    for (int ci = 0; f && ci < ct.n; ++ci)
        if (ct.C[ci] == f && ct.cost[ci] != 0) return f;
    return 0;
}

// AGX_PHMM_TAIL_BETA overrides the planner's tail term (experiments); negative = unset
double tail_beta_override() { static const double v = agx_knob_real(agx_tune("AGX_PHMM_TAIL_BETA"), -1.0); return v; }

// AGX_PHMM_MAX_CLASSES: upper bound on the kernel classes a mixed batch may spread over (default 6)
int max_classes() { static const int v = (int)agx_knob_int(agx_tune("AGX_PHMM_MAX_CLASSES"), 6, positive); return v; }

// What both tiling rules share: which classes may tile a haplotype of H columns, and the cheapest one offered so far.
struct TilingSearch {
    ClassTable ct;
    uint32_t H;
    int best = -1, bestG = 0;
    double best_cost = 0;
    // the lanes class ci needs, or 0: more than 64, wider than AGX_PHMM_MAX_C when a class has been found already, not the
    // forced width, or not built for this arithmetic (cost 0)
    int lanes(int ci) const
    {
        const int C = ct.C[ci];
        const int G = (int)((H + C - 1) / C);
        if (G > 64) return 0;
        if (C > max_cols_per_lane() && best >= 0) return 0;
        if (force_cols_per_lane(ct) && C != force_cols_per_lane(ct)) return 0;
        return ct.cost[ci] == 0 ? 0 : G;
    }
    void offer(int ci, int G, double cost)
    {
        if (best >= 0 && !(cost < best_cost)) return;
        best = ci, bestG = G, best_cost = cost;
    }
    // cls << 8 | G, as ShapeTable::slot_tile holds it; class 255: no tiling fits
    uint16_t tile() const { return (uint16_t)((best < 0 ? 255 : best) << 8 | bestG); }
};

// allowed: bit ci set = class ci may be used; *cost_out: the lane time estimate of the choice;
// beta: lanes' worth of extra weight on a wave's own duration (steps * C), see tile_with_tail_term
uint16_t choose_tiling(int kind, uint32_t R, uint32_t H, uint64_t allowed, double *cost_out, double beta)
{
    TilingSearch s{class_table(kind), H};
    for (int ci = 0; ci < s.ct.n; ++ci) {
        if (!((allowed >> ci) & 1u)) continue;
        const int G = s.lanes(ci);
        if (!G) continue;
        const int C = s.ct.C[ci];
        s.offer(ci, G, (double)(R + G - 1) * C * ((64.0 / (double)(64 / G)) * s.ct.cost[ci] + beta));
    }
    if (cost_out) *cost_out = s.best_cost;
    return s.tile();
}

// Uniform batches (most pairs share one (R, H) shape): the launch lasts ceil(waves / SIMDs)
// wave-times, so the tiling of that shape is chosen with that quantisation.
// pair_reads: the plan will pair reads into trains (packed float fill): a wave then lasts 2 (R + 1) + G - 2 steps and there are
// half as many -- the quantisation is that of the paired waves (H = 270: 9 lanes x 30 columns are 2341 paired waves, three
// rounds of which the last is a seventh full, 0.363 ms; 16 x 17 are 4096, four full rounds, 0.286 ms)
uint16_t choose_tiling_uniform(int kind, uint32_t R, uint32_t H, int64_t count, int n_simd, bool pair_reads)
{
    TilingSearch s{class_table(kind), H};
    for (int ci = 0; ci < s.ct.n; ++ci) {
        const int G = s.lanes(ci);
        if (!G) continue;
        const int C = s.ct.C[ci];
        const int64_t per_wave = 64 / G;
        int64_t waves = (count + per_wave - 1) / per_wave;
        uint32_t steps = R + (uint32_t)G - 1u;
        if (pair_reads && C <= 30) { // (widths 31 and 32 do not pair: see WaveFiller::partner_of)
            waves = (waves + 1) / 2;
            steps = 2u * (R + 1u) + (uint32_t)G - 2u;
        }
        const int64_t rounds = (waves + n_simd - 1) / n_simd;
        s.offer(ci, G, (double)rounds * steps * C * s.ct.cost[ci]);
    }
    return s.tile();
}

// Cuts [0, n) into at most `parts` pieces of about equal size whose inner boundaries satisfy is_cut(i) (i starts a new
// run): every O(pairs) pass of the planner that works run by run is threaded over such pieces.
template <typename F>
std::vector<size_t> cut_at_runs(size_t n, int parts, F is_cut)
{
    std::vector<size_t> cut{0};
    for (int k = 1; k < parts; ++k) {
        size_t i = std::max(cut.back(), n * (size_t)k / (size_t)parts);
        while (i < n && (i == 0 || !is_cut(i))) ++i;
        if (i > cut.back() && i < n) cut.push_back(i);
    }
    cut.push_back(n);
    return cut;
}

inline uint32_t key_of(const Plan &p) { return p.R << 16 | p.th; }

// ---- stage: shape statistics -- the window of read and haplotype lengths; every pair starts out tiled for its own haplotype
struct Lengths {
    uint32_t r_min = 0xffffffffu, r_max = 0, h_min = 0xffffffffu, h_max = 0;
    bool one_shape = false;
    void add(const Lengths &r)
    {
        r_min = std::min(r_min, r.r_min), r_max = std::max(r_max, r.r_max);
        h_min = std::min(h_min, r.h_min), h_max = std::max(h_max, r.h_max);
    }
};
Lengths shape_stats(std::vector<Plan> &gen)
{
    struct alignas(64) PerThread { // one cache line per part
        Lengths l;
    };
    std::vector<PerThread> ranges((size_t)agx_host_threads());
    agx_parallel_for((int64_t)gen.size(), 16384, [&](int64_t lo, int64_t hi, int t) {
        Lengths r;
        for (int64_t k = lo; k < hi; ++k) {
            Plan &p = gen[(size_t)k];
            p.th = p.H;
            r.r_min = std::min(r.r_min, p.R), r.r_max = std::max(r.r_max, p.R);
            r.h_min = std::min(r.h_min, p.H), r.h_max = std::max(r.h_max, p.H);
        }
        ranges[(size_t)t].l = r;
    });
    Lengths all;
    for (const PerThread &r : ranges) all.add(r.l);
    all.one_shape = !gen.empty() && all.r_min == all.r_max && all.h_min == all.h_max;
    return all;
}

// ---- stage: haplotype pairing.  Two haplotypes share a lane group in the packed kernel: within every read's run, order the
// haplotypes by length and tile neighbours for the longer of the two, so that partners get the
// same class (mixed-length regions would otherwise leave most second slots vacant).
// (fixed-length input -- BASELINE configs 3 and 5 -- needs neither this pairing nor the sorts below: every
// key is equal, the enumeration order already is the order they would produce)
void pair_haplotypes(std::vector<Plan> &gen, int run_parts)
{
    const std::vector<size_t> cut = cut_at_runs(gen.size(), run_parts, [&](size_t i) { return gen[i].read != gen[i - 1].read; });
    agx_pool_run((int)cut.size() - 1, [&](int t) {
        size_t a = cut[(size_t)t];
        const size_t end = cut[(size_t)t + 1];
        while (a < end) {
            size_t z = a;
            while (z < end && gen[z].read == gen[a].read) ++z;
            std::stable_sort(gen.begin() + (ptrdiff_t)a, gen.begin() + (ptrdiff_t)z, [](const Plan &x, const Plan &y) { return x.H > y.H; });
            for (size_t k = a; k < z; ++k) gen[k].th = gen[a + ((k - a) & ~(size_t)1)].H; // the pair's longer one
            a = z;
        }
    });
}

// ---- stage: the distinct (R, th) shapes of the batch and how many pairs have each.
// The shapes of a batch live in a window of read and haplotype lengths: they are counted in a dense table over
// that window (threads add to it directly) when it has at most 2^20 cells, else through a hash map.
struct ShapeTable {
    bool one_shape = false, dense = false;
    uint32_t r_min = 0, h_min = 0;
    uint64_t win_h = 0;
    std::unordered_map<uint32_t, uint32_t> sparse_slot; // key -> slot (batches whose window is too wide)
    std::vector<uint32_t> slot_count;                   // pairs per slot
    std::vector<uint16_t> slot_tile;                    // cls << 8 | G
    std::vector<uint32_t> shape_key, shape_slot;        // the distinct shapes
    size_t slot_of(uint32_t key) const
    {
        if (one_shape) return 0;
        if (dense) return (size_t)((key >> 16) - r_min) * (size_t)win_h + ((key & 0xffffu) - h_min);
        return sparse_slot.find(key)->second;
    }
    int64_t n_shapes() const { return (int64_t)shape_key.size(); }
    ShapeTable(const std::vector<Plan> &gen, const Lengths &all);
};
ShapeTable::ShapeTable(const std::vector<Plan> &gen, const Lengths &all) : one_shape(all.one_shape), r_min(all.r_min), h_min(all.h_min)
{
    const int64_t n = (int64_t)gen.size();
    const uint64_t win_r = n ? (uint64_t)all.r_max - all.r_min + 1 : 0;
    win_h = n ? (uint64_t)all.h_max - all.h_min + 1 : 0;
    // (... and no more than eight cells per pair beyond 65 536: a small batch with a wide window goes through the map)
    dense = win_r * win_h <= std::min<uint64_t>((uint64_t)1 << 20, std::max<uint64_t>(65536, 8 * (uint64_t)n));
    if (one_shape) {
        slot_count.assign(1, (uint32_t)n);
        shape_key.push_back(key_of(gen[0]));
        shape_slot.push_back(0);
    } else if (dense) {
        slot_count.assign((size_t)(win_r * win_h), 0);
        agx_parallel_for(n, 16384, [&](int64_t lo, int64_t hi, int) {
            uint32_t last = 0, run = 0; // consecutive pairs often share their shape
            for (int64_t k = lo; k < hi; ++k) {
                const uint32_t key = key_of(gen[(size_t)k]);
                if (run && key == last) {
                    ++run;
                    continue;
                }
                if (run) __atomic_fetch_add(&slot_count[slot_of(last)], run, __ATOMIC_RELAXED);
                last = key;
                run = 1;
            }
            if (run) __atomic_fetch_add(&slot_count[slot_of(last)], run, __ATOMIC_RELAXED);
        });
        for (size_t sl = 0; sl < slot_count.size(); ++sl)
            if (slot_count[sl]) {
                shape_key.push_back((uint32_t)(all.r_min + sl / win_h) << 16 | (uint32_t)(all.h_min + sl % win_h));
                shape_slot.push_back((uint32_t)sl);
            }
    } else {
        for (const Plan &p : gen) {
            const auto it = sparse_slot.emplace(key_of(p), (uint32_t)slot_count.size());
            if (it.second) {
                slot_count.push_back(0);
                shape_key.push_back(key_of(p));
                shape_slot.push_back(it.first->second);
            }
            ++slot_count[it.first->second];
        }
    }
    slot_tile.assign(slot_count.size(), (uint16_t)0xff00);
}

// ---- stage: tiling per (R, H) shape.  The per-class cost curve is flat over many widths, and every class
// is its own launch: a mixed batch first chooses freely, then keeps the few classes that carry
// most of the work and re-tiles the rest among them (a shape no kept class can span keeps its own).
struct Tiling {
    std::vector<double> class_work; // per class: the lane time of the pairs tiled for it
    double waves_est = 0;
    double beta = 0;
};
void tile_all(const PlanKind &pk, ShapeTable &st, Tiling &tl)
{
    const ClassTable ct = class_table(pk.kind);
    const uint64_t all_classes = ~0ull;
    std::vector<std::vector<double>> work((size_t)agx_host_threads(), std::vector<double>((size_t)ct.n + 1, 0.0)); // [ct.n]: waves
    agx_parallel_for(st.n_shapes(), 512, [&](int64_t lo, int64_t hi, int t) {
        std::vector<double> &wk = work[(size_t)t];
        for (int64_t k = lo; k < hi; ++k) {
            const uint32_t key = st.shape_key[(size_t)k], cnt = st.slot_count[st.shape_slot[(size_t)k]];
            double cost = 0;
            const uint16_t v = choose_tiling(pk.kind, key >> 16, key & 0xffffu, all_classes, &cost, tl.beta);
            st.slot_tile[st.shape_slot[(size_t)k]] = v;
            const int c = v >> 8, G = v & 0xff;
            if (c < ct.n) {
                wk[(size_t)c] += cost * cnt;
                wk[(size_t)ct.n] += (double)cnt * G / 64.0 / pk.slots;
            }
        }
    });
    tl.class_work.assign((size_t)ct.n, 0.0);
    tl.waves_est = 0;
    for (const auto &wk : work) {
        for (int c = 0; c < ct.n; ++c) tl.class_work[(size_t)c] += wk[(size_t)c];
        tl.waves_est += wk[(size_t)ct.n];
    }
}
Tiling tile_with_tail_term(const PlanKind &pk, int n_cu, ShapeTable &st)
{
    Tiling tl;
    tl.beta = tail_beta_override() >= 0 ? tail_beta_override() : 0.0;
    tile_all(pk, st, tl);
    // Tail regime (as in the SW planner): a batch whose waves fill the chip's resident capacity (3 waves
    // per SIMD for the packed kernel, 2 for the others) less than 1.6 times lasts as long as its longest
    // waves; it is re-tiled with 2 lanes' worth of extra cost on a wave's own duration, which spreads
    // pairs over more lanes.  Mixed regions (tools/phmm_tail_beta_sweep.py): 2048 pairs +27 % packed /
    // +35 % double, 16 384 pairs +30 % / +3 %; beyond 1.6 fillings the term costs a few percent.
    if (tail_beta_override() < 0 && n_cu > 0 && tl.waves_est / ((pk.slots == 2 ? 3.0 : 2.0) * 4.0 * n_cu) < 1.6) {
        tl.beta = 2.0;
        tile_all(pk, st, tl);
    }
    return tl;
}

// ---- stage: consolidation.  small batches afford fewer launches: about one class per 16384 wavefronts of work
// (tools/phmm_classes_sweep.py: the count matters little, fewer is never worse by more than 3 %)
void consolidate(const PlanKind &pk, const Tiling &tl, ShapeTable &st)
{
    const ClassTable ct = class_table(pk.kind);
    const int k_max = std::min(max_classes(), 1 + (int)(tl.waves_est / 16384.0));
    int used = 0;
    for (double wk : tl.class_work) used += wk > 0;
    if (used <= k_max) return;
    std::vector<int> order((size_t)ct.n);
    for (int k = 0; k < ct.n; ++k) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return tl.class_work[(size_t)x] > tl.class_work[(size_t)y]; });
    uint64_t keep = 0;
    for (int k = 0; k < k_max; ++k) keep |= 1ull << order[(size_t)k];
    agx_parallel_for(st.n_shapes(), 512, [&](int64_t lo, int64_t hi, int) {
        for (int64_t k = lo; k < hi; ++k) {
            uint16_t &v = st.slot_tile[st.shape_slot[(size_t)k]];
            if ((v >> 8) < 64 && ((keep >> (v >> 8)) & 1u)) continue;
            const uint16_t w = choose_tiling(pk.kind, st.shape_key[(size_t)k] >> 16, st.shape_key[(size_t)k] & 0xffffu, keep, nullptr, tl.beta);
            if ((w >> 8) < ct.n) v = w;
        }
    });
}

// ---- stage: assignment -- every pair takes its shape's class and lane count
int assign_tiles(const PlanKind &pk, const ShapeTable &st, std::vector<Plan> &gen)
{
    const ClassTable ct = class_table(pk.kind);
    std::atomic<int64_t> unfit{-1};
    agx_parallel_for((int64_t)gen.size(), 16384, [&](int64_t lo, int64_t hi, int) {
        uint32_t last_key = 0;
        uint16_t last_v = 0;
        bool have = false;
        for (int64_t gi = lo; gi < hi; ++gi) {
            Plan &p = gen[(size_t)gi];
            const uint32_t key = key_of(p);
            if (!have || key != last_key) {
                last_v = st.slot_tile[st.slot_of(key)];
                last_key = key;
                have = true;
            }
            p.cls = (uint8_t)(last_v >> 8);
            p.G = (uint8_t)(last_v & 0xff);
            if (p.cls >= ct.n) {
                int64_t none = -1;
                unfit.compare_exchange_strong(none, gi);
            }
        }
    });
    if (unfit.load() < 0) return AGX_OK;
    const Plan &p = gen[(size_t)unfit.load()];
    agx_set_error("pair (read %u, hap %u): no lane tiling fits %u columns", p.read, p.hap, p.H);
    return AGX_E_LIMIT;
}

// a packed plan pairs reads into trains unless told not to: wherever it can (forced), or from two waves per SIMD after pairing
bool wants_trains(const PlanKind &pk, int n_cu, double waves_est)
{
    return pk.slots == 2 && pk.trains != 1 && (pk.trains == 2 || waves_est >= 16.0 * n_cu);
}

// ---- stage: dominant (R, H) shape?  A shape that half the pairs have is tiled by the uniform rule.
void retile_dominant_shape(const PlanKind &pk, int n_cu, bool one_shape, double waves_est, std::vector<Plan> &gen)
{
    const int64_t n = (int64_t)gen.size();
    if (n < 1024 || n_cu <= 0) return;
    const size_t stride = (size_t)n / 512;
    uint32_t cand = 0;
    int votes = 0;
    for (size_t k = 0; k < 512; ++k) {
        const uint32_t key = key_of(gen[k * stride]);
        if (votes == 0) {
            cand = key;
            votes = 1;
        } else
            votes += key == cand ? 1 : -1;
    }
    std::atomic<int64_t> count{0};
    if (one_shape)
        count = n;
    else
        agx_parallel_for(n, 16384, [&](int64_t lo, int64_t hi, int) {
            int64_t c = 0;
            for (int64_t k = lo; k < hi; ++k) c += key_of(gen[(size_t)k]) == cand;
            count.fetch_add(c, std::memory_order_relaxed);
        });
    if (votes <= 0 || count.load() * 2 < n) return;
    const uint16_t v = choose_tiling_uniform(pk.kind, cand >> 16, cand & 0xffffu, (count.load() + pk.slots - 1) / pk.slots, 4 * n_cu,
                                             wants_trains(pk, n_cu, waves_est));
    const uint8_t c = (uint8_t)(v >> 8), G = (uint8_t)(v & 0xff);
    if (c >= class_table(pk.kind).n) return;
    agx_parallel_for(n, 16384, [&](int64_t lo, int64_t hi, int) {
        for (int64_t k = lo; k < hi; ++k)
            if (key_of(gen[(size_t)k]) == cand) {
                gen[(size_t)k].cls = c;
                gen[(size_t)k].G = G;
            }
    });
}

// ---- stage: the two-pass sort.  order: class, lanes per group (wide first), then long reads first, read, haplotype -- a wave's
// groups then have similar row counts, and haplotypes of one read stay adjacent (one LDS table).
// `gen` is (read, haplotype)-ordered: two stable counting passes, by read length, then by class.
std::vector<Plan> sort_for_waves(const PlanKind &pk, const Lengths &all, std::vector<Plan> &gen)
{
    std::vector<Plan> plan;
    if (all.one_shape)
        plan.swap(gen); // one (R, H) shape: one class, one G, equal keys throughout
    else {
        const uint32_t max_r = all.r_max;
        std::vector<Plan> tmp;
        counting_sort(gen, tmp, (size_t)max_r + 1, [&](const Plan &p) { return (size_t)(max_r - p.R); });
        counting_sort(tmp, plan, (size_t)class_table(pk.kind).n * 64 + 1, [](const Plan &p) { return (size_t)p.cls * 64 + (size_t)(64 - p.G); });
    }
    std::vector<Plan>().swap(gen);
    return plan;
}

// ---- stage: waves and records.  The greedy filling below runs on pieces of `plan` that start where the read, the class or
// the group width changes (a wave never spans such a piece's end; a packed group's partner is the next haplotype of
// the SAME read, so no group does either); the pieces' records are then laid end to end.
// Read trains (packed float fill, fast cell): two consecutive reads of the sorted order whose runs in this bucket hold
// the same haplotypes -- reads of one region -- share their lane groups: the second enters as the first leaves, the skew
// is paid once (K (R + 1) + G - 1 steps for K = 2 reads instead of K (R + G - 1)).  Measured envelope, tools/train_emulation.py:
// +5.4 % on config 3, +5.8 % at four times its size; trains of four +4 %, of eight a loss (their tables outgrow the LDS
// share of a wave).  Only where the paired waves still fill the chip: from two waves per SIMD after pairing.
struct WaveFiller {
    const PlanKind &pk;
    const PlanSeed &seed;
    const std::vector<Plan> &plan;
    const ClassTable ct;
    bool use_trains; // the driver makes a plan with, and perhaps one without

    size_t tab_bytes(bool f64, uint32_t rows) const
    {
        return pk.slots == 2 ? ph_pk_tab_bytes(rows) : pk.lut_rows ? ph_lut_tab_bytes(rows) : ph_tab_bytes(f64, seed.gatk_prior, rows);
    }
    size_t partner_of(size_t a, size_t end, size_t &run_end) const;
    PhGroup2 packed_group(size_t &i, size_t end, size_t tr, uint32_t R2, uint32_t tab) const;
    void count_waste(const PhWave &w, const ClassLaunch &cl, PlanOut &o) const;
    void fill(size_t i, size_t end, PlanOut &o) const;
};

// the run of entries of plan[a]'s read in its (class, G) bucket ends at run_end; returns how many entries on its partner
// run -- the next read, same bucket, same haplotypes -- starts (0: none)
size_t WaveFiller::partner_of(size_t a, const size_t end, size_t &run_end) const
{
    const uint32_t rd = plan[a].read;
    const int cls = plan[a].cls, G = plan[a].G;
    size_t a_end = a;
    while (a_end < end && plan[a_end].read == rd && plan[a_end].cls == cls && plan[a_end].G == G) ++a_end;
    run_end = a_end;
    if (a_end >= end || plan[a_end].cls != cls || plan[a_end].G != G) return 0;
    // (widths 31 and 32 sit at their 256-register cap: the train build spills 15-25 values and gains nothing --
    // config 5's packed float shard -1.5 %, four times its size +1.6 %, tools/trains_shapes.py)
    if (pk.trains != 2 && ct.C[cls] > 30) return 0;
    const uint32_t rd2 = plan[a_end].read;
    size_t b_end = a_end;
    while (b_end < end && plan[b_end].read == rd2 && plan[b_end].cls == cls && plan[b_end].G == G) ++b_end;
    if (b_end - a_end != a_end - a) return 0;
    for (size_t k = 0; k < a_end - a; ++k)
        if (plan[a + k].hap != plan[a_end + k].hap) return 0;
    // the tables a wave of such groups needs must fit its LDS share: a run that does not fill a wave shares it with
    // its neighbours' tables (mixed regions), and a train's table is twice a read's
    const size_t run_groups = (a_end - a + 1) / 2, per_wave = (size_t)(64 / G);
    const size_t tables = pk.trains == 2 ? 1 : (per_wave + run_groups - 1) / run_groups + (run_groups % per_wave ? 1 : 0); // (forced: one table must fit)
    if (tables * ph_pk_tab_bytes(plan[a].R + 1u + plan[a_end].R + 2u * ((uint32_t)G - 1u)) > tab_budget()) return 0;
    return a_end - a;
}

// the packed record of plan[i] and, where the next entry is another haplotype of the same read in the same bucket, of that
// one too (i then moves on to it); tr: the entries' second reads sit tr entries on (0: no train)
PhGroup2 WaveFiller::packed_group(size_t &i, const size_t end, const size_t tr, const uint32_t R2, const uint32_t tab) const
{
    const Plan &p = plan[i];
    const uint32_t vacant_out = (uint32_t)seed.n_pairs;
    PhGroup2 g{};
    g.R_tab = p.R | (tab << 16);
    g.hap_dw[0] = seed.hap_dw[p.hap];
    g.H[0] = p.H;
    g.out[0] = p.out;
    g.init32[0] = FLT_MAX / 16 / (float)p.H;
    // second slot: the next haplotype of the same read in this class, else vacant
    g.hap_dw[1] = 0;
    g.H[1] = 0;
    g.out[1] = vacant_out;
    g.init32[1] = 0;
    g.R2 = R2;
    g.out2[0] = tr ? plan[i + tr].out : vacant_out;
    g.out2[1] = vacant_out;
    if (i + 1 < end && plan[i + 1].cls == p.cls && plan[i + 1].G == p.G && plan[i + 1].read == p.read) {
        const Plan &q = plan[i + 1];
        g.hap_dw[1] = seed.hap_dw[q.hap];
        g.H[1] = q.H;
        g.out[1] = q.out;
        g.init32[1] = FLT_MAX / 16 / (float)q.H;
        if (tr) g.out2[1] = plan[i + 1 + tr].out;
        ++i;
    }
    return g;
}

// AGX_TRACE_CREATE: where the padded cells of wave w (the last one of o, its groups behind it) go
void WaveFiller::count_waste(const PhWave &w, const ClassLaunch &cl, PlanOut &o) const
{
    const int G = w.G, cnt = w.n_groups, slots = pk.slots;
    const uint32_t steps = w.steps;
    const int64_t cols = (int64_t)G * cl.C;
    for (int k = 0; k < cnt; ++k) {
        uint32_t R = 0, H[2] = {0, 0}, extra = 0; // extra: a train's reset row
        if (slots == 2) {
            const PhGroup2 &g = o.groups2[w.first_group + (size_t)k];
            R = (g.R_tab & 0xffffu) + g.R2, H[0] = g.H[0], H[1] = g.H[1], extra = g.R2 ? 1u : 0u;
        } else {
            const PhGroup &g = o.groups1[w.first_group + (size_t)k];
            R = g.R_tab & 0xffffu, H[0] = g.H;
        }
        for (int h = 0; h < slots; ++h) {
            o.waste[0] += (int64_t)R * H[h];
            o.waste[1] += (int64_t)R * (cols - H[h]);
            o.waste[2] += (int64_t)(G - 1 + (int)extra) * cols;
            o.waste[3] += (int64_t)(steps - (R + extra + (uint32_t)G - 1u)) * cols;
        }
    }
    o.waste[4] += (int64_t)steps * (64 - (int64_t)cnt * G) * cl.C * slots;
}

void WaveFiller::fill(size_t i, const size_t end, PlanOut &o) const
{
    const int slots = pk.slots;
    const bool lut_rows = pk.lut_rows;
    size_t run_end = i, run_delta = 0; // the read run i is in ends at run_end; its partner run starts run_delta entries on (0: none)
    while (i < end) {
        const int cls = plan[i].cls;
        ClassLaunch cl;
        cl.C = ct.C[cls];
        cl.first_wave = (uint32_t)o.waves.size();
        while (i < end && plan[i].cls == cls) {
            const int G = plan[i].G;
            const int per_wave = 64 / G;
            PhWave w{};
            w.first_group = (uint32_t)(slots == 2 ? o.groups2.size() : o.groups1.size());
            w.first_tab = (uint32_t)o.tabs.size();
            w.G = (uint16_t)G;
            int cnt = 0;
            uint32_t steps = 0, ntabs = 0, last_read = 0xffffffffu;
            size_t lut_bytes = 0; // lut_rows: every table is as long as its own read (+ a neutral row at either end)
            while (i < end && plan[i].cls == cls && plan[i].G == G && cnt < per_wave) {
                const Plan &p = plan[i];
                if (use_trains && i >= run_end) run_delta = partner_of(i, end, run_end);
                const size_t tr = use_trains ? run_delta : 0; // this entry's second read sits tr entries on
                const uint32_t R2 = tr ? plan[i + tr].R : 0u;
                const uint32_t nsteps = std::max(steps, p.R + (tr ? R2 + 1u : 0u) + (uint32_t)G - 1u);
                const uint32_t ntabs_new = ntabs + (p.read != last_read ? 1u : 0u);
                if (lut_rows) {
                    if (cnt > 0 && p.read != last_read && lut_bytes + ph_lut_lds_bytes(p.R + 2u) > tab_budget()) break;
                } else if (cnt > 0 && ntabs_new > 1 && tab_bytes(pk.rows_f64, nsteps + G - 1) * ntabs_new > tab_budget())
                    break;
                if (p.read != last_read) {
                    // (lut_rows: the table's offset / 16 rides in the upper half of R, agx_phmm_lut_kernel.hip)
                    o.tabs.push_back(PhTab{seed.read_dw[p.read], lut_rows ? p.R | (uint32_t)(lut_bytes / 16) << 16 : p.R});
                    if (use_trains) o.tabs.push_back(tr ? PhTab{seed.read_dw[plan[i + tr].read], R2} : PhTab{0u, 0u});
                    if (lut_rows) lut_bytes += ph_lut_lds_bytes(p.R + 2u);
                    last_read = p.read;
                }
                ntabs = ntabs_new;
                steps = nsteps;
                if (slots == 2)
                    o.groups2.push_back(packed_group(i, end, tr, R2, ntabs - 1));
                else
                    o.groups1.push_back(make_group(seed.hap_dw[p.hap], p, ntabs - 1));
                ++cnt;
                ++i;
                if (use_trains && run_delta && i == run_end) { // the partner run rode along: step over it
                    i += run_delta;
                    run_end = i;
                    run_delta = 0;
                }
            }
            w.n_groups = (uint16_t)cnt;
            w.n_tabs = (uint16_t)ntabs;
            w.steps = steps;
            if (pk.trace) count_waste(w, cl, o);
            if (G != 16) cl.all_g16 = false;
            cl.lds = std::max(cl.lds, lut_rows ? lut_bytes : tab_bytes(pk.rows_f64, steps + G - 1) * ntabs);
            if (pk.kind == 2) cl.lds_rescue = std::max(cl.lds_rescue, ph_tab_bytes(true, seed.gatk_prior, steps + G - 1) * ntabs); // (only the float fill's records are reused for a double pass)
            o.padded += (int64_t)steps * 64 * cl.C * slots;
            o.waves.push_back(w);
        }
        cl.n_waves = (uint32_t)o.waves.size() - cl.first_wave;
        o.launches.push_back(cl);
    }
}

// lays the records of the pieces end to end: offsets first, then the copies by threads
void stitch(const std::vector<PlanOut> &part, int slots, PlanOut &po)
{
    const int pieces = (int)part.size();
    size_t n_groups = 0, n_tabs = 0, n_waves = 0;
    for (const PlanOut &o : part) n_groups += o.groups1.size() + o.groups2.size(), n_tabs += o.tabs.size(), n_waves += o.waves.size();
    (slots == 2 ? po.groups2.resize(n_groups) : po.groups1.resize(n_groups));
    po.tabs.resize(n_tabs);
    po.waves.resize(n_waves);
    std::vector<size_t> g0((size_t)pieces), t0((size_t)pieces), w0((size_t)pieces);
    size_t ga = 0, ta = 0, wa = 0;
    for (int t = 0; t < pieces; ++t) {
        const PlanOut &o = part[(size_t)t];
        g0[(size_t)t] = ga, t0[(size_t)t] = ta, w0[(size_t)t] = wa;
        ga += o.groups1.size() + o.groups2.size(), ta += o.tabs.size(), wa += o.waves.size();
        po.padded += o.padded;
        for (int k = 0; k < 5; ++k) po.waste[k] += o.waste[k];
        for (ClassLaunch cl : o.launches) { // a class that runs on into the next piece is one launch
            cl.first_wave += (uint32_t)w0[(size_t)t];
            if (!po.launches.empty() && po.launches.back().C == cl.C) {
                ClassLaunch &m = po.launches.back();
                m.n_waves += cl.n_waves;
                m.all_g16 = m.all_g16 && cl.all_g16;
                m.lds = std::max(m.lds, cl.lds);
                m.lds_rescue = std::max(m.lds_rescue, cl.lds_rescue);
            } else
                po.launches.push_back(cl);
        }
    }
    agx_pool_run(pieces, [&](int t) {
        const PlanOut &o = part[(size_t)t];
        if (slots == 2)
            std::copy(o.groups2.begin(), o.groups2.end(), po.groups2.begin() + (ptrdiff_t)g0[(size_t)t]);
        else
            std::copy(o.groups1.begin(), o.groups1.end(), po.groups1.begin() + (ptrdiff_t)g0[(size_t)t]);
        std::copy(o.tabs.begin(), o.tabs.end(), po.tabs.begin() + (ptrdiff_t)t0[(size_t)t]);
        for (size_t k = 0; k < o.waves.size(); ++k) {
            PhWave w = o.waves[k];
            w.first_group += (uint32_t)g0[(size_t)t];
            w.first_tab += (uint32_t)t0[(size_t)t];
            po.waves[w0[(size_t)t] + k] = w;
        }
    });
}

// one plan over all of `plan`: the pieces between cut[] filled by threads, then stitched
void build(const WaveFiller &wf, const std::vector<size_t> &cut, PlanOut &po)
{
    const int pieces = (int)cut.size() - 1, slots = wf.pk.slots;
    if (pieces <= 1) {
        wf.fill(0, wf.plan.size(), po);
        return;
    }
    std::vector<PlanOut> part((size_t)pieces);
    agx_pool_run(pieces, [&](int t) {
        PlanOut &o = part[(size_t)t];
        const size_t span = cut[(size_t)t + 1] - cut[(size_t)t];
        (slots == 2 ? o.groups2.reserve(span / 2 + 64) : o.groups1.reserve(span));
        o.waves.reserve(span / 4 + 16);
        o.tabs.reserve(span / 8 + 16);
        wf.fill(cut[(size_t)t], cut[(size_t)t + 1], o);
    });
    stitch(part, slots, po);
}

// ---- stage: the trains decision -- one plan, or the plans with and without trains compared by their padded cells
void build_with_or_without_trains(WaveFiller &wf, const std::vector<size_t> &cut, bool one_shape, PlanOut &po)
{
    const int trains = wf.pk.trains;
    // (one shape throughout: every run pairs like the first, and pairing only removes steps -- one plan is made, whichever)
    size_t probe_end = 0;
    const bool sure = wf.use_trains && one_shape && !wf.plan.empty() && wf.partner_of(0, wf.plan.size(), probe_end) != 0;
    if (wf.use_trains && one_shape && !sure && trains != 2) wf.use_trains = false;
    if (!wf.use_trains) {
        build(wf, cut, po);
        return;
    }
    // Trains double a table: where a wave's groups come from several reads (mixed regions: a read's haplotype pairs do
    // not fill a wave) fewer tables fit the wave's LDS share and lanes stay empty -- on the reference's corpus shape
    // useful cells 0.85 -> 0.77.  Both plans are made (the wave filling is a tenth of the planner) and the one with
    // fewer padded cells stays; forced trains (AGX_PHMM_TRAINS_ON) skip the comparison.
    PlanOut with;
    build(wf, cut, with);
    with.trains = true;
    bool keep = trains == 2 || sure;
    if (!keep) {
        wf.use_trains = false;
        build(wf, cut, po);
        keep = (double)with.padded < 0.985 * (double)po.padded;
        if (wf.pk.trace)
            fprintf(stderr, "[phmm make_plan kind %d] read trains: %zu waves / %.4g padded cells with, %zu / %.4g without -> %s\n", wf.pk.kind, with.waves.size(),
                    (double)with.padded, po.waves.size(), (double)po.padded, keep ? "with" : "without");
    }
    if (keep) {
        with.file_order = po.file_order;
        po = std::move(with);
    }
}

// ---- stage: dispatch order within every launch, and the LDS check
int order_and_check(bool one_shape, PlanOut &po)
{
    for (const ClassLaunch &cl : po.launches) {
        // dispatch order = longest waves first (a wave lasts steps x C): the buckets were filled widest
        // group first, which leaves narrow groups with long reads for the end of the launch
        if (!one_shape)
            std::stable_sort(po.waves.begin() + cl.first_wave, po.waves.begin() + cl.first_wave + cl.n_waves,
                             [](const PhWave &a, const PhWave &b) { return a.steps > b.steps; });
        if (int rc = check_lds(std::max(cl.lds, cl.lds_rescue), cl.lds)) return rc;
    }
    return AGX_OK;
}

void trace_plan(int kind, const PlanOut &po)
{
    const double t = (double)po.padded;
    fprintf(stderr, "[phmm make_plan kind %d] %zu waves, padded cells %.4g: useful %.3f, columns beyond H %.3f, skew %.3f, steps beyond the group's read %.3f, "
                    "lanes without a group %.3f; read trains %d; classes",
            kind, po.waves.size(), t, po.waste[0] / t, po.waste[1] / t, po.waste[2] / t, po.waste[3] / t, po.waste[4] / t, (int)po.trains);
    for (const ClassLaunch &cl : po.launches) fprintf(stderr, " %dx%u", cl.C, cl.n_waves);
    fprintf(stderr, "\n");
}

} // namespace

int make_plan(const PlanSeed &seed, std::vector<Plan> gen, const PlanKind &pk, PlanOut &po)
{
    const double tm0 = agx_now_ms();
    const int n_cu = seed.n_cu;
    const int64_t n = (int64_t)gen.size();
    const Lengths all = shape_stats(gen);
    const int run_parts = (int)std::min<int64_t>(agx_host_threads(), std::max<int64_t>(1, n / 8192));
    if (pk.slots == 2 && !all.one_shape) pair_haplotypes(gen, run_parts);
    ShapeTable shapes(gen, all);
    const double tm1 = agx_now_ms();
    const Tiling tiling = tile_with_tail_term(pk, n_cu, shapes);
    consolidate(pk, tiling, shapes);
    const double tm2 = agx_now_ms();
    if (int rc = assign_tiles(pk, shapes, gen)) return rc;
    retile_dominant_shape(pk, n_cu, all.one_shape, tiling.waves_est, gen);
    const double tm3 = agx_now_ms();
    const std::vector<Plan> plan = sort_for_waves(pk, all, gen);
    po.file_order = all.one_shape;
    const double tm4 = agx_now_ms();
    const std::vector<size_t> cut = cut_at_runs(plan.size(), run_parts, [&](size_t i) {
        return plan[i].read != plan[i - 1].read || plan[i].cls != plan[i - 1].cls || plan[i].G != plan[i - 1].G;
    });
    WaveFiller wf{pk, seed, plan, class_table(pk.kind), wants_trains(pk, n_cu, tiling.waves_est)};
    build_with_or_without_trains(wf, cut, all.one_shape, po);
    if (int rc = order_and_check(all.one_shape, po)) return rc;
    if (pk.trace)
        fprintf(stderr, "[phmm make_plan kind %d] pairing+shapes %.2f, tiling %.2f, assign %.2f, sort %.2f, waves+records %.2f ms (%d pieces)\n",
                pk.kind, tm1 - tm0, tm2 - tm1, tm3 - tm2, tm4 - tm3, agx_now_ms() - tm4, (int)cut.size() - 1);
    if (pk.trace && po.padded > 0) trace_plan(pk.kind, po);
    return AGX_OK;
}

} // namespace agx_phmm_host
