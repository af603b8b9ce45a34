// Private to the host side of the PairHMM path -- agx_phmm.cpp (create, launch, results) and agx_phmm_plan.cpp (the planner) --
// and included by nothing else: what those two files need of each other.  No kernel includes it.
#pragma once
#include "agx_phmm.h"

#include <vector>

#include "agx_internal.h"

// (hidden: what crosses a file boundary is still no export of the library)
namespace agx_phmm_host __attribute__((visibility("hidden"))) {

// one pair with work, from its enumeration to its record
struct Plan {
    uint32_t out;
    uint32_t read, hap;
    uint32_t R, H;
    uint32_t th; // the haplotype length the pair is tiled for (packed kernel: the longer one of its lane group)
    uint8_t cls;
    uint8_t G;
};

struct ClassLaunch {
    int C = 0;
    bool all_g16 = true; // every wave of the class has groups of exactly 16 lanes
    uint32_t first_wave = 0, n_waves = 0;
    size_t lds = 0;        // dynamic LDS of the fill in the batch's precision
    size_t lds_rescue = 0; // same tables with double rows (F32 rescue pass)
};

// kind 0..2 = rows of kPhClassCost over kPhClasses; kind 3 = the packed float kernel's own class table
struct ClassTable {
    const int *C;
    const double *cost;
    int n;
};
ClassTable class_table(int kind);

// ---- a plan: lane tilings, waves and records for one kernel family
struct PlanOut {
    std::vector<PhGroup> groups1;
    std::vector<PhGroup2> groups2;
    std::vector<PhTab> tabs;
    std::vector<PhWave> waves;
    std::vector<ClassLaunch> launches;
    int64_t padded = 0;
    // where the padded cells go (AGX_TRACE_CREATE): [0] useful R x H, [1] columns beyond H (vacant halves included), [2] the G - 1
    // steps of skew, [3] steps beyond a group's own R + G - 1 (the wave steps its longest read), [4] lanes without a group
    int64_t waste[5] = {0, 0, 0, 0, 0};
    bool trains = false; // packed plan: groups may carry a second read, every table has two PhTab entries (agx_phmm.h)
    bool file_order = false; // one (R, H) shape: the records are in output order (agx_phmm_batch_bind_results)
};

// What a plan is made from: the pairs with work in output order (region, read, haplotype) and where the image holds
// every read and haplotype.  A packed float batch keeps it: its double rescue plan is made when a fill first counts a
// pair below the float range (config 3: never), not at creation.
struct PlanSeed {
    std::vector<Plan> gen0;
    std::vector<uint32_t> read_dw, hap_dw;
    int64_t n_pairs = 0;
    int n_cu = 256;
    bool gatk_prior = false;
};

// What kind of plan make_plan makes.  kind = row of kPhClassCost (0 f64, 1 f64 FMA, 2 f32, 3 packed f32 FMA); slots = pairs
// per group; lut_rows: the read tables have the rows of agx_phmm_lut_kernel.hip;
// trains: 0 = read trains where they pay (packed plans of enough waves), 1 = never, 2 = wherever two reads can share a group
struct PlanKind {
    int kind, slots;
    bool rows_f64, lut_rows, trace;
    int trains;
};
// `gen` (a copy of seed.gen0, or seed.gen0 itself when nobody needs it afterwards) is consumed.
int make_plan(const PlanSeed &seed, std::vector<Plan> gen, const PlanKind &pk, PlanOut &po);

// the record of a pair that has a lane group to itself, its read in table `tab` of its wave
PhGroup make_group(uint32_t hap_dw, const Plan &p, uint32_t tab);
// AGX_E_LIMIT with the message naming `named` when a launch's tables of `largest` bytes are beyond the LDS of a CU
int check_lds(size_t largest, size_t named);

// AGX_TRACE_CREATE (Fnv1a, agx_internal.h; tests/test_phmm_plan_digest_cpu.py pins the digests per kind of batch): kind and slots as make_plan takes them, the flags, the padded cells, the launches and every record as it goes to the device
Fnv1a plan_hash(int kind, int slots, const PlanOut &po, const std::vector<ClassLaunch> &launches);

} // namespace agx_phmm_host
