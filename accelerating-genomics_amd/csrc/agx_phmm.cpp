// Host side of the PairHMM path: validation, packing, launches, the final
// log10 (host libm, as the reference does), multi-device sharding, and the pairHMM() seam
// (include/agx.h, "PairHMM" section).  The lane-tiling choice and the waves are made in agx_phmm_plan.cpp.
#include "agx_phmm_host.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <memory>
#include <mutex>
#include <thread>

#include "agx_parallel.h"

using namespace agx_phmm_host;

namespace {

constexpr uint32_t kHapSlack = 44;       // zero bytes after every haplotype: any tiling reads in bounds

constexpr int stripe_cols() { return AGX_PH_STRIPE_COLS; }

// the float modes: a fill in float and a double pass over the pairs below the float range, the logarithms on the device
bool f32_family(int precision) { return precision == AGX_PHMM_F32 || precision == AGX_PHMM_F32_FMA; }

// The quality tables of a batch as they lie on the device, one after the other: the launch code takes the four from lut_ptrs.
struct Lut {
    double d[256];
    float f[256];
    double mis_d[256];
    float mis_f[256];
};
struct LutPtrs {
    const void *d, *f, *mis_d, *mis_f;
};
LutPtrs lut_ptrs(const void *base)
{
    const char *p = (const char *)base;
    return LutPtrs{p + offsetof(Lut, d), p + offsetof(Lut, f), p + offsetof(Lut, mis_d), p + offsetof(Lut, mis_f)};
}

// 256-entry quality LUT exactly as partition_read() computes it (antidiagsPairHMM.c:104-107)
// mis: the mismatch prior per quality byte -- Qr (reference) or Qr/3 (AGX_PHMM_GATK_PRIOR)
void build_lut(bool gatk_prior, Lut &lut)
{
    for (int c = 0; c < 256; ++c) {
        // the reference holds the quality bytes in plain `char`, signed on x86-64 (:100-107): a byte of 0x80 and above
        // is a negative number there (200 -> -56), and so it is here
        lut.d[c] = pow(10.0, -((c < 128 ? c : c - 256) - 33.0) * 0.1);
        lut.f[c] = (float)lut.d[c];
        lut.mis_d[c] = gatk_prior ? lut.d[c] / 3.0 : lut.d[c];
        lut.mis_f[c] = gatk_prior ? lut.f[c] / 3.0f : lut.f[c];
    }
}

// Arrays on their way to the device through one pinned staging block and one stream: one DMA per array.
struct Piece {
    DevBuf *dst;
    const void *src; // NULL: the array lies in page-locked memory of its own (the image), given to queue()
    size_t bytes;
};
struct StagedUpload {
    std::vector<Piece> pieces;
    static size_t slot(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    // the staging block and every destination
    int alloc(agx_ctx *ctx, PinBuf &stage) const
    {
        size_t stage_bytes = 0;
        for (const Piece &pc : pieces)
            if (pc.src) stage_bytes += slot(pc.bytes);
        int rc = stage.alloc(ctx, stage_bytes);
        for (const Piece &pc : pieces)
            if (!rc) rc = pc.dst->alloc(ctx, pc.bytes);
        return rc;
    }
    // copies every array into the block and queues its DMA on cs; the first error stops the queuing and is returned
    hipError_t queue(const PinBuf &stage, const void *own_pinned, hipStream_t cs) const
    {
        hipError_t e = hipSuccess;
        size_t at = 0;
        for (const Piece &pc : pieces) {
            if (!pc.src) {
                if (e == hipSuccess && pc.bytes) e = hipMemcpyAsync(pc.dst->p, own_pinned, pc.bytes, hipMemcpyHostToDevice, cs);
                continue;
            }
            if (pc.bytes) memcpy((char *)stage.p + at, pc.src, pc.bytes);
            if (e == hipSuccess && pc.bytes) e = hipMemcpyAsync(pc.dst->p, (char *)stage.p + at, pc.bytes, hipMemcpyHostToDevice, cs);
            at += slot(pc.bytes);
        }
        return e;
    }
};

} // namespace

// accuracy guard of the packed float fill (PhUnderflow, agx_phmm.h): |log10 L| below this times sqrt(R) -> double.
// 1.24 x the worst error found over 3.6 million pairs (reads of 10 ... 2000 bases, three error rates; tools/phmm_f32_guard_cal.py)
constexpr double kGuardRef = 0.18, kGuardGatk = 0.40;

// agx_phmm_forward sends a batch of more than two of these through in pieces of whole regions (see there)
constexpr double kPhmmPieceCells = 4.0e9;

struct agx_phmm_batch {
    agx_ctx *ctx = nullptr; // retained
    int precision = AGX_PHMM_F64;
    bool probs = false; // read tracks are probabilities (pairHMM() seam), not Phred characters
    bool gatk_prior = false;
    int64_t n_pairs = 0;
    bool packed = false;          // main plan uses PhGroup2 records (AGX_PHMM_F32_FMA)
    bool rescue_pending = false;  // packed batches: the rescue plan has not run for the last launch (it runs from
                                  // agx_phmm_batch_results, and only when the fill counted a pair below the float range)
    bool trains = false;          // ... with read trains (PlanOut::trains)
    bool fast = false;            // ... and its fill runs the fast cell (plain DNA, no Phred-0 gap-continuation quality in the batch)
    bool lut_ring = false;        // ... and some read's table is a ring (ph_lut_is_ring): the STREAM builds
    bool lut_prior = false;       // double modes on plain DNA: priors looked up in the read tables (agx_phmm_lut_kernel.hip)
    bool separate_rescue = false; // the double rescue pass has its own plan (packed batches), made on first use from:
    std::unique_ptr<PlanSeed> rescue_seed;
    bool rescue_broken = false; // making that plan failed (out of memory): the batch's float results cannot be completed
    DevBuf img, sums, lut, counter;
    bool counters_dirty = false; // a launch has counted into `counter` and nobody has taken (and reset) the counts yet
    PinBuf out_stage; // page-locked landing block of the results, taken at create (agx_phmm_batch_results allocates nothing)
    struct DevPlan {
        DevBuf groups, tabs, waves;
        std::vector<ClassLaunch> launches;
    } main, rescue, stripe; // stripe: pairs whose haplotype no class spans, one per wavefront
    DevBuf stripe_scratch;    // 6 * stripe_rows doubles per workgroup of the striped launch
    uint32_t stripe_rows = 0, stripe_grid = 0;
    bool stripe_mis_div = false; // the striped launch derives the GATK mismatch prior itself (see create)
    agx_phmm_info info{};
    // agx_phmm_batch_bind_results: a page-locked array of the caller's that a packed float fill in output order writes its
    // log10 likelihoods into itself; bound_flag (in out_stage) says whether a pair went to the rescue plan instead
    bool file_order = false;
    double *bound = nullptr;
    PinBuf bound_flag;
    // the fast cell's table rows of every read, made once at creation (phmm_pk_rows); rows_base_dw: image word of the first read
    DevBuf pk_rows;
    uint32_t rows_base_dw = 0;
};

namespace {

// ---- the stages of create_batch, in the order it calls them.  Each reads what it is given and fills a result of its own.

int check_args(const agx_phmm_desc *d, bool probs, int precision)
{
    if (!d || precision < AGX_PHMM_F64 || precision > AGX_PHMM_F32_FMA) {
        agx_set_error("agx_phmm_batch_create: bad descriptor or precision %d", precision);
        return AGX_E_ARG;
    }
    if (d->n_regions && (!d->region_read || !d->region_hap || !d->read_off || !d->hap_off)) {
        agx_set_error("agx_phmm_batch_create: NULL offset table");
        return AGX_E_ARG;
    }
    if (probs && precision != AGX_PHMM_F64) {
        agx_set_error("probability tracks are only supported with AGX_PHMM_F64");
        return AGX_E_ARG;
    }
    return AGX_OK;
}

// A descriptor whose regions name only part of its reads and haplotypes -- a shard of agx_phmm_forward_devices, a
// piece of agx_phmm_forward: they keep the caller's absolute indices -- is narrowed to that part first: the image
// holds what the regions use, not every read and haplotype of the caller (each of config 5's eight shards carried
// the whole batch's 33 MB before).  r_base / h_base: what error messages add to name the caller's numbers.
struct View {
    bool narrowed = false;
    agx_phmm_desc desc;
    std::vector<uint32_t> rr, rh;
    uint32_t r_base = 0, h_base = 0;
};
int narrow_view(const agx_phmm_desc *d, View &view)
{
    const uint32_t ng = d->n_regions;
    uint32_t rmin = d->n_reads, rmax = 0, hmin = d->n_haps, hmax = 0;
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1];
        const uint32_t h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
        if (r1 < r0 || h1 < h0 || r1 > d->n_reads || h1 > d->n_haps) {
            agx_set_error("region %u: read/haplotype ranges out of order or out of bounds", g);
            return AGX_E_ARG;
        }
        rmin = std::min(rmin, r0), rmax = std::max(rmax, r1);
        hmin = std::min(hmin, h0), hmax = std::max(hmax, h1);
    }
    if (!ng || !(rmin > 0 || rmax < d->n_reads || hmin > 0 || hmax < d->n_haps)) return AGX_OK;
    view.narrowed = true;
    view.desc = *d;
    view.rr.assign(d->region_read, d->region_read + ng + 1);
    view.rh.assign(d->region_hap, d->region_hap + ng + 1);
    for (uint32_t &v : view.rr) v -= rmin;
    for (uint32_t &v : view.rh) v -= hmin;
    view.desc.region_read = view.rr.data();
    view.desc.region_hap = view.rh.data();
    view.desc.read_off = d->read_off + rmin; // offsets into the tracks stay absolute
    view.desc.hap_off = d->hap_off + hmin;
    view.desc.n_reads = rmax - rmin;
    view.desc.n_haps = hmax - hmin;
    view.r_base = rmin, view.h_base = hmin;
    return AGX_OK;
}

// lengths are checked once per read / haplotype, not once per pair
int check_lengths(const agx_phmm_desc *d, const View &view)
{
    for (uint32_t r = 0; d->read_off && r < d->n_reads; ++r)
        if (d->read_off[r + 1] - d->read_off[r] > AGX_PHMM_MAX_READ_LEN) {
            agx_set_error("read %u: %llu bases exceed the supported %d", r + view.r_base, (unsigned long long)(d->read_off[r + 1] - d->read_off[r]),
                          AGX_PHMM_MAX_READ_LEN);
            return AGX_E_LIMIT;
        }
    for (uint32_t h = 0; d->hap_off && h < d->n_haps; ++h)
        if (d->hap_off[h + 1] - d->hap_off[h] > AGX_PHMM_MAX_HAP_LEN) {
            agx_set_error("haplotype %u: %llu bases exceed the supported %d", h + view.h_base, (unsigned long long)(d->hap_off[h + 1] - d->hap_off[h]),
                          AGX_PHMM_MAX_HAP_LEN);
            return AGX_E_LIMIT;
        }
    return AGX_OK;
}

// ---- enumerate the pairs in output order: region, read, haplotype (threads over regions)
struct PairCount {
    int64_t n_pairs = 0, cells = 0;
};
int enumerate_pairs(const agx_phmm_desc *d, std::vector<Plan> &gen0, PairCount &count)
{
    const uint32_t ng = d->n_regions;
    // per region: output offset (every pair has an output slot) and offset into gen0 (pairs with work)
    std::vector<int64_t> out0((size_t)ng + 1, 0), fill0((size_t)ng + 1, 0);
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1], h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
        int64_t nr = 0, nh = 0;
        for (uint32_t r = r0; r < r1; ++r) nr += d->read_off[r + 1] != d->read_off[r];
        for (uint32_t h = h0; h < h1; ++h) nh += d->hap_off[h + 1] != d->hap_off[h];
        out0[g + 1] = out0[g] + (int64_t)(r1 - r0) * (h1 - h0);
        fill0[g + 1] = fill0[g] + nr * nh;
        count.cells += (int64_t)(d->read_off[r1] - d->read_off[r0]) * (int64_t)(d->hap_off[h1] - d->hap_off[h0]);
        if (out0[g + 1] > 0x7ffffff0LL) {
            agx_set_error("more than 2^31 pairs in one batch");
            return AGX_E_LIMIT;
        }
    }
    const int64_t n_pairs = count.n_pairs = out0[ng];
    gen0.resize((size_t)fill0[ng]);
    // (grain: about 16384 pairs per part -- smaller parts cost more in hand-over than they save)
    const int64_t region_grain = std::max<int64_t>(1, 16384 / std::max<int64_t>(1, n_pairs / std::max<uint32_t>(ng, 1)));
    agx_parallel_for((int64_t)ng, region_grain, [&](int64_t ga, int64_t gz, int) {
        for (int64_t g = ga; g < gz; ++g) {
            const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1], h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
            size_t at = (size_t)fill0[(size_t)g];
            int64_t o = out0[(size_t)g];
            for (uint32_t r = r0; r < r1; ++r) {
                const uint32_t R = (uint32_t)(d->read_off[r + 1] - d->read_off[r]);
                for (uint32_t h = h0; h < h1; ++h, ++o) {
                    const uint32_t H = (uint32_t)(d->hap_off[h + 1] - d->hap_off[h]);
                    if (R == 0 || H == 0) continue; // sum over an empty row/all-zero row is 0 (log10 -> -inf)
                    Plan p{};
                    p.out = (uint32_t)o;
                    p.read = r;
                    p.hap = h;
                    p.R = R;
                    p.H = H;
                    gen0[at++] = p;
                }
            }
        }
    });
    return AGX_OK;
}

// ---- haplotypes wider than 64 lanes x the widest class of this arithmetic go to the striped kernel: taken out of gen0
std::vector<Plan> split_long(const agx_phmm_desc *d, int precision, std::vector<Plan> &gen0)
{
    std::vector<Plan> gen_long;
    const ClassTable ct = class_table(precision);
    uint32_t span = 0;
    for (int ci = 0; ci < ct.n; ++ci)
        if (ct.cost[ci] != 0) span = std::max(span, 64u * (uint32_t)ct.C[ci]);
    uint64_t longest = 0;
    for (uint32_t h = 0; d->hap_off && h < d->n_haps; ++h) longest = std::max<uint64_t>(longest, d->hap_off[h + 1] - d->hap_off[h]);
    if (longest <= span) return gen_long;
    size_t keep = 0;
    for (const Plan &p : gen0) {
        if (p.H > span)
            gen_long.push_back(p);
        else
            gen0[keep++] = p;
    }
    gen0.resize(keep);
    return gen_long;
}

// ---- image: every read and haplotype once, shared by all plans of the batch.  Offsets come from two
// prefix sums, the bytes are copied by threads (the pairHMM() seam's probability tracks excepted: one pair);
// with a device the image is built straight in pinned staging memory.
struct ImageLayout {
    static constexpr size_t zero_dw = (64 * 32 + 8) / 4; // words 0..: an all-zero haplotype block for vacant packed slots (64 lanes x 32 columns)
    uint32_t n_reads = 0, n_haps = 0;
    size_t img_dw = zero_dw;
    size_t reads_end_dw = zero_dw; // the reads' tracks lie in [zero_dw, reads_end_dw), 5 x ceil(R / 4) words each
    static size_t hap_block_dw(size_t H) // zero slack: any class tiling, and whole stripes of the striped kernel, read in bounds
    {
        const size_t stripe_bytes = 64u * (size_t)stripe_cols();
        const size_t bytes = std::max(H + kHapSlack, (H + stripe_bytes - 1) / stripe_bytes * stripe_bytes + 8);
        return (bytes + 3) / 4;
    }
    int lay(const agx_phmm_desc *d, bool probs, std::vector<uint32_t> &read_dw, std::vector<uint32_t> &hap_dw);
};
int ImageLayout::lay(const agx_phmm_desc *d, bool probs, std::vector<uint32_t> &read_dw, std::vector<uint32_t> &hap_dw)
{
    n_reads = d->read_off ? d->n_reads : 0, n_haps = d->hap_off ? d->n_haps : 0;
    read_dw.assign(n_reads, 0xffffffffu);
    hap_dw.assign(n_haps, 0xffffffffu);
    for (uint32_t r = 0; r < n_reads; ++r) {
        const size_t R = (size_t)(d->read_off[r + 1] - d->read_off[r]), trk = (R + 3) / 4;
        if (probs && (img_dw & 1)) ++img_dw; // doubles need 8-byte alignment
        read_dw[r] = (uint32_t)img_dw;
        img_dw += probs ? R * 8 + trk : 5 * trk;
        if (img_dw > 0xfffffff0ull) break;
    }
    reads_end_dw = img_dw;
    for (uint32_t h = 0; h < n_haps && img_dw <= 0xfffffff0ull; ++h) {
        hap_dw[h] = (uint32_t)img_dw;
        img_dw += hap_block_dw((size_t)(d->hap_off[h + 1] - d->hap_off[h]));
    }
    if (img_dw > 0xfffffff0ull) {
        agx_set_error("packed image exceeds 16 GiB; split the batch");
        return AGX_E_LIMIT;
    }
    return AGX_OK;
}

bool has_tracks(const agx_phmm_desc *d, bool probs)
{
    return d->read_bases && d->hap_bases && (probs || (d->q_base && d->q_ins && d->q_del && d->q_gcp));
}

// What the image fill saw of the batch's bytes on its way (float-FMA and double modes; false throughout otherwise).
// fast: the packed float fill's fast cell (agx_phmm_pk_kernel.hip) divides by 1 - Qg and codes the bases in two bits, so a
// gap-continuation quality of Phred 0 or below, a read base outside ACGTN or a haplotype base outside ACGT anywhere
// in the batch keeps the plain cell.
// wild: a read whose state can run away -- a quality byte below '!' (as a signed char: a "probability" above 1), or a row with
// Qi + Qd > 1 (both gap qualities of Phred 0 ... 3; 3 + 3 is over 1, 3 + 4 is not): 1 - (Qi + Qd) < 0 there, the recurrence is
// no longer sub-stochastic and its state alternates in sign and grows.  No read trains in such a batch.
// not_dna: a read base outside ACGTN or a haplotype base outside ACGT
struct ImageScan {
    bool fast = true, wild = false, not_dna = false;
};
void copy_reads(const agx_phmm_desc *d, const double *const prob[4], const std::vector<uint32_t> &read_dw, uint32_t *img, int64_t ra, int64_t rz)
{
    for (int64_t r = ra; r < rz; ++r) {
        const uint64_t o = d->read_off[r];
        const size_t R = (size_t)(d->read_off[r + 1] - o), trk = (R + 3) / 4;
        if (prob) {
            double *q = reinterpret_cast<double *>(img + read_dw[(size_t)r]);
            for (int k = 0; k < 4; ++k) memcpy(q + (size_t)k * R, prob[k] + o, R * sizeof(double));
            uint8_t *c = reinterpret_cast<uint8_t *>(q + 4 * R);
            memcpy(c, d->read_bases + o, R);
            memset(c + R, 0, trk * 4 - R);
        } else {
            uint8_t *p = reinterpret_cast<uint8_t *>(img + read_dw[(size_t)r]);
            const uint8_t *src[5] = {d->read_bases, d->q_base, d->q_ins, d->q_del, d->q_gcp};
            for (int k = 0; k < 5; ++k) {
                memcpy(p + (size_t)k * trk * 4, src[k] + o, R);
                memset(p + (size_t)k * trk * 4 + R, 0, trk * 4 - R);
            }
        }
    }
}
ImageScan fill_image(const agx_phmm_desc *d, const double *const prob[4], int precision, const ImageLayout &lay, const PlanSeed &seed, uint32_t *img)
{
    const bool probs = prob != nullptr, packed = precision == AGX_PHMM_F32_FMA;
    const bool scan = !probs && precision != AGX_PHMM_F32;
    std::atomic<bool> not_fast{false}, not_dna{false}, wild{false};
    static const auto gap_prob = [] { // Q of a gap quality byte from '!' on, as build_lut() has it
        std::array<double, 256> t{};
        for (int c = 0; c < 128; ++c) t[c] = pow(10.0, -(c - 33.0) * 0.1);
        return t;
    }();
    static const auto dna_table = [] {
        std::array<uint8_t, 256> t{};
        for (const char *p = "ACGT"; *p; ++p) t[(uint8_t)*p] = 3; // bit 0: allowed in a read, bit 1: in a haplotype
        t[(uint8_t)'N'] = 1;
        return t;
    }();
    agx_parallel_for((int64_t)lay.n_reads, 2048, [&](int64_t ra, int64_t rz, int) {
        bool zero = false, other = false, low = false;
        for (int64_t r = ra; r < rz && scan; ++r)
            for (uint64_t k = d->read_off[r]; k < d->read_off[r + 1]; ++k) {
                zero |= packed && (int8_t)d->q_gcp[k] <= (int8_t)'!'; // signed as the reference's char: 0x80.. are "probabilities" above 1
                other |= !(dna_table[d->read_bases[k]] & 1);
                // (a byte below '!' in either gap track, or two gap qualities whose sum can pass 1: only with one of them below Phred 4)
                const int8_t gap_lo = std::min((int8_t)d->q_ins[k], (int8_t)d->q_del[k]);
                low |= packed && ((int8_t)d->q_base[k] < (int8_t)'!' ||
                                  (gap_lo < (int8_t)'!' + 4 && (gap_lo < (int8_t)'!' || gap_prob[d->q_ins[k]] + gap_prob[d->q_del[k]] > 1.0)));
            }
        if (zero || other) not_fast.store(true, std::memory_order_relaxed);
        if (low) wild.store(true, std::memory_order_relaxed);
        if (other) not_dna.store(true, std::memory_order_relaxed);
        copy_reads(d, prob, seed.read_dw, img, ra, rz);
    });
    agx_parallel_for((int64_t)lay.n_haps, 2048, [&](int64_t ha, int64_t hz, int) {
        for (int64_t h = ha; h < hz; ++h) {
            const uint64_t o = d->hap_off[h];
            const size_t H = (size_t)(d->hap_off[h + 1] - o);
            uint8_t *p = reinterpret_cast<uint8_t *>(img + seed.hap_dw[(size_t)h]);
            memcpy(p, d->hap_bases + o, H);
            if (scan) {
                bool other = false;
                for (size_t k = 0; k < H; ++k) other |= !(dna_table[d->hap_bases[o + k]] & 2);
                if (other) {
                    not_fast.store(true, std::memory_order_relaxed);
                    not_dna.store(true, std::memory_order_relaxed);
                }
            }
            memset(p + H, 0, ImageLayout::hap_block_dw(H) * 4 - H);
        }
    });
    return ImageScan{!not_fast.load(), wild.load(), not_dna.load()};
}

// ---- which plan the batch gets
struct PlanChoice {
    bool lut_ring = false, lut_prior = false;
    int trains = 1; // as PlanKind::trains
};
PlanChoice choose_plan(const agx_ctx *ctx, const agx_phmm_desc *d, int precision, bool probs, bool have_tracks, const ImageLayout &lay, const ImageScan &scan)
{
    PlanChoice c;
    const bool f64 = !f32_family(precision), packed = precision == AGX_PHMM_F32_FMA;
    // A packed float batch cannot reuse its records for the double rescue pass: that pass has a plan of its own, made
    // from the kept seed when a fill first counts a pair below the float range (launch_rescue_plan).
    // double modes on plain DNA run the kernel whose read tables carry the priors (other rows, other LDS sizes)
    // (... while the longest read's table stays within a wave's LDS share when two waves per SIMD are resident -- 20 KB, 363
    // rows of 56 bytes: a launch reserves its longest table for every wave, so beyond that fewer waves fit a CU and the
    // 33-byte rows of phmm_fill win -- 7 % at reads of 420 bases, 19 % at 500, 20 % at 600 -- although that kernel selects
    // its priors (tools/lut_vs_select_long_reads.py, profiles/r03as_lut_vs_select.log; the limit was 40 KB until round 3);
    // a 4096-row read fits the 160 KB only there)
    uint64_t longest_read = 0;
    for (uint32_t r = 0; r < lay.n_reads; ++r) longest_read = std::max<uint64_t>(longest_read, d->read_off[r + 1] - d->read_off[r]);
    // (round 3, second step: such reads keep a 256-row ring in LDS, refilled as the wave advances -- the looked-up-prior kernel
    // for every read length; AGX_PHMM_NO_RING in the tuning build restores the 20 KB rule)
    c.lut_ring = ph_lut_is_ring((uint32_t)longest_read + 2u);
    c.lut_prior = f64 && !probs && have_tracks && !scan.not_dna && (!c.lut_ring || !agx_tune("AGX_PHMM_NO_RING")) && !agx_tune("AGX_PHMM_NO_LUT");
    // read trains: the fast cell only, and only where no read's state can run away (ImageScan::wild: a quality byte below '!', or a
    // row with Qi + Qd > 1 -- legal bytes, Phred 0 ... 3): a first read whose state ran to infinity would hand NaN to the second
    // through the reset row's 0 x inf.  (Seen on the device with both gap qualities at Phred 0 and reads of 250 bases: the second
    // read's NaN sums went to the double rescue pass, so its results stayed right but were no longer the plain schedule's bits.)
    const int trains_opt = ctx ? ctx->opt_phmm_trains : AGX_PHMM_TRAINS_AUTO;
    const bool may_train = packed && scan.fast && !scan.wild && !agx_tune("AGX_PHMM_PLAIN_CELL") && !agx_tune("AGX_PHMM_NO_TRAINS");
    c.trains = may_train ? (trains_opt == AGX_PHMM_TRAINS_ON ? 2 : trains_opt == AGX_PHMM_TRAINS_OFF ? 1 : 0) : 1;
    return c;
}

// ---- striped plan: one pair per wavefront, every pair its own read table
struct StripePlan {
    PlanOut po;
    uint32_t steps = 0; // of the longest wave
    size_t lds = 0;
    bool mis_div = false;
};
int plan_stripes(const std::vector<Plan> &gen_long, const PlanSeed &seed, StripePlan &sp)
{
    for (const Plan &p : gen_long) {
        PhWave w{};
        w.first_group = (uint32_t)sp.po.groups1.size();
        w.first_tab = (uint32_t)sp.po.tabs.size();
        w.n_groups = 1;
        w.n_tabs = 1;
        w.G = 64;
        w.steps = p.R + 63u;
        sp.po.tabs.push_back(PhTab{seed.read_dw[p.read], p.R});
        sp.po.groups1.push_back(make_group(seed.hap_dw[p.hap], p, 0));
        sp.po.waves.push_back(w);
        sp.steps = std::max(sp.steps, w.steps);
        sp.lds = std::max(sp.lds, ph_tab_bytes(true, seed.gatk_prior, w.steps + 63u));
        const int64_t n_stripes = (p.H + 64 * stripe_cols() - 1) / (64 * stripe_cols());
        sp.po.padded += n_stripes * w.steps * 64 * stripe_cols();
    }
    // The GATK prior's fifth table column (Qr / 3) does not fit beside the others for reads beyond 3 870 bases (41 bytes x
    // (R + 126) rows > 160 KiB): the striped launch then keeps four columns and divides in its step head -- the same IEEE
    // division the host's table was made with, so the results do not change.
    if (seed.gatk_prior && sp.lds > 160 * 1024) {
        sp.mis_div = true;
        sp.lds = ph_tab_bytes(true, false, sp.steps + 63u);
    }
    return check_lds(sp.lds, sp.lds);
}

// ---- the batch object: what it is, what its launches are, what agx_phmm_batch_info reports
struct BatchFacts {
    int precision;
    bool probs, gatk_prior;
    PairCount count;
    size_t n_work; // pairs with work (every pair of the batch, unless a read or haplotype is empty)
    size_t img_dw;
    int n_cu;
};
// (b is the driver's own pointer, set first: its guard destroys a batch that a later line of this function could not finish)
void new_batch(agx_phmm_batch *&b, agx_ctx *ctx, const BatchFacts &f, const ImageScan &scan, const PlanChoice &choice, const PlanOut &pmain, const StripePlan &sp)
{
    const bool packed = f.precision == AGX_PHMM_F32_FMA;
    b = new agx_phmm_batch();
    agx_ctx_retain(ctx);
    b->ctx = ctx;
    b->precision = f.precision;
    b->probs = f.probs;
    b->gatk_prior = f.gatk_prior;
    b->packed = packed;
    b->file_order = packed && pmain.file_order && sp.po.waves.empty() && (int64_t)f.n_work == f.count.n_pairs;
    b->fast = packed && scan.fast && !agx_tune("AGX_PHMM_PLAIN_CELL");
    b->trains = packed && pmain.trains;
    b->lut_prior = choice.lut_prior;
    b->lut_ring = choice.lut_prior && choice.lut_ring;
    // the code objects this batch will launch from, loaded now rather than inside its first launch
    if (ctx) {
        if (packed) agx_phmm_pk_preload();
        if (packed && pmain.trains) agx_phmm_pk_train_preload();
        agx_phmm_scalar_preload();
        if (choice.lut_prior) agx_phmm_lut_preload();
        agx_copy_preload();
        if (f32_family(f.precision)) agx_phmm_finish_preload();
    }
    b->separate_rescue = packed;
    b->n_pairs = f.count.n_pairs;
    b->main.launches = pmain.launches;
    const size_t groups_bytes = packed ? pmain.groups2.size() * sizeof(PhGroup2) : pmain.groups1.size() * sizeof(PhGroup);
    b->info.n_pairs = f.count.n_pairs;
    b->info.cells = f.count.cells;
    b->info.padded_cells = pmain.padded + sp.po.padded;
    b->info.input_bytes = (int64_t)(f.img_dw * 4 + groups_bytes + pmain.tabs.size() * sizeof(PhTab) +
                                    pmain.waves.size() * sizeof(PhWave));
    // (a packed batch's rescue plan is not counted: it is launched only when a fill underflowed)
    b->info.n_launches = (int32_t)(pmain.launches.size() + (!packed && f32_family(f.precision) ? pmain.launches.size() : 0));
    b->info.n_waves = (int32_t)(pmain.waves.size() + sp.po.waves.size());
    if (!sp.po.waves.empty()) {
        ClassLaunch cl;
        cl.C = stripe_cols();
        cl.n_waves = (uint32_t)sp.po.waves.size();
        cl.lds = cl.lds_rescue = sp.lds;
        b->stripe.launches.push_back(cl);
        b->info.n_launches += 1;
        b->stripe_mis_div = sp.mis_div;
        b->stripe_rows = (sp.steps + 128u + 63u) & ~63u; // a 64-row block may start at the last step, 63 rows ahead
        b->stripe_grid = std::min<uint32_t>(cl.n_waves, (uint32_t)f.n_cu * 8u);
    }
}

// AGX_TRACE_CREATE, what the tests pin: the plans, the image and the batch's flags (tests/phmm_plan_cases.py parses these lines)
void trace_digests(const agx_phmm_batch *b, const PlanOut &pmain, const PlanOut &pstripe, const uint32_t *img, size_t img_dw, const PlanSeed &seed)
{
    fprintf(stderr, "[agx_phmm_batch_create] planned for %d CUs\n", seed.n_cu);
    fprintf(stderr, "[agx_phmm_batch_create] plan digest main %016llx\n", (unsigned long long)plan_hash(b->precision, b->packed ? 2 : 1, pmain, pmain.launches).h);
    if (!pstripe.waves.empty()) {
        Fnv1a f = plan_hash(b->precision, 1, pstripe, b->stripe.launches);
        f.field(b->stripe_rows), f.field(b->stripe_grid), f.field((uint8_t)b->stripe_mis_div);
        fprintf(stderr, "[agx_phmm_batch_create] plan digest stripe %016llx\n", (unsigned long long)f.h);
    }
    Fnv1a f;
    f.field((uint64_t)img_dw);
    f.bytes(img, img_dw * 4);
    for (const std::vector<uint32_t> *v : {&seed.read_dw, &seed.hap_dw}) f.field((uint64_t)v->size()), f.bytes(v->data(), v->size() * sizeof(uint32_t));
    fprintf(stderr, "[agx_phmm_batch_create] image digest %016llx\n", (unsigned long long)f.h);
    fprintf(stderr, "[agx_phmm_batch_create] batch flags fast %d trains %d lut_prior %d lut_ring %d file_order %d\n", (int)b->fast, (int)b->trains,
            (int)b->lut_prior, (int)b->lut_ring, (int)b->file_order);
}

// ---- upload.  Everything goes through one pinned staging block and the context's copy stream: one DMA per array,
// one synchronisation at the end (create is blocking by contract).  *e: the first HIP error of what was queued.
int upload(agx_phmm_batch *b, const PlanOut &pmain, const PlanOut &pstripe, const uint32_t *img, size_t img_dw, PinBuf &stage, hipError_t *e)
{
    agx_ctx *ctx = b->ctx;
    Lut lut;
    build_lut(b->gatk_prior, lut);
    StagedUpload up;
    up.pieces.push_back(Piece{&b->img, nullptr, img_dw * 4}); // already in pinned memory
    if (b->packed)
        up.pieces.push_back(Piece{&b->main.groups, pmain.groups2.data(), pmain.groups2.size() * sizeof(PhGroup2)});
    else
        up.pieces.push_back(Piece{&b->main.groups, pmain.groups1.data(), pmain.groups1.size() * sizeof(PhGroup)});
    up.pieces.push_back(Piece{&b->main.tabs, pmain.tabs.data(), pmain.tabs.size() * sizeof(PhTab)});
    up.pieces.push_back(Piece{&b->main.waves, pmain.waves.data(), pmain.waves.size() * sizeof(PhWave)});
    if (!pstripe.waves.empty()) {
        up.pieces.push_back(Piece{&b->stripe.groups, pstripe.groups1.data(), pstripe.groups1.size() * sizeof(PhGroup)});
        up.pieces.push_back(Piece{&b->stripe.tabs, pstripe.tabs.data(), pstripe.tabs.size() * sizeof(PhTab)});
        up.pieces.push_back(Piece{&b->stripe.waves, pstripe.waves.data(), pstripe.waves.size() * sizeof(PhWave)});
    }
    up.pieces.push_back(Piece{&b->lut, &lut, sizeof lut});
    int rc = up.alloc(ctx, stage);
    if (!rc && !pstripe.waves.empty()) rc = b->stripe_scratch.alloc(ctx, (size_t)b->stripe_grid * 6u * b->stripe_rows * sizeof(double));
    if (!rc) rc = b->sums.alloc(ctx, ((size_t)b->n_pairs + 1) * sizeof(double)); // +1: spare slot of vacant packed halves
    if (!rc) rc = b->counter.alloc(ctx, 2 * sizeof(unsigned long long)); // [0] rescued, [1] below the float range
    if (!rc) rc = b->out_stage.alloc(ctx, 2 * (size_t)b->n_pairs * sizeof(double) + 16);
    if (!rc && b->info.n_launches > 1) rc = agx_ctx_prepare_fanout(ctx);
    if (rc) return rc;
    hipStream_t cs = ctx->copy;
    *e = up.queue(stage, img, cs);
    if (*e == hipSuccess && !pstripe.waves.empty()) *e = hipMemsetAsync(b->stripe_scratch.p, 0, b->stripe_scratch.bytes, cs);
    if (*e == hipSuccess) *e = hipMemsetAsync(b->sums.p, 0, b->sums.bytes, cs); // degenerate pairs keep sum 0
    if (*e == hipSuccess) *e = hipMemsetAsync(b->counter.p, 0, b->counter.bytes, cs);
    return AGX_OK;
}

// The fast cell's table rows -- two float4 of derived constants per read position, several double divisions each --
// are the same in every wave that uses a read and in every launch of the batch: made here, once (phmm_pk_rows), the
// waves copy them into LDS instead of deriving them (3 % of config 3's launch).
int make_pk_rows(agx_phmm_batch *b, const agx_phmm_desc *d, const ImageLayout &lay, const PlanSeed &seed, PinBuf &h_reads, DevBuf &d_reads, hipError_t *e)
{
    agx_ctx *ctx = b->ctx;
    const uint32_t n_reads = lay.n_reads;
    const size_t n_rows = (lay.reads_end_dw - lay.zero_dw) / 5 * 4;
    int rc = b->pk_rows.alloc(ctx, std::max<size_t>(n_rows, 1) * 32);
    if (!rc) rc = h_reads.alloc(ctx, (size_t)n_reads * sizeof(PhTab));
    if (!rc) rc = d_reads.alloc(ctx, (size_t)n_reads * sizeof(PhTab));
    if (rc) return rc;
    PhTab *hr = (PhTab *)h_reads.p;
    for (uint32_t r = 0; r < n_reads; ++r) hr[r] = PhTab{seed.read_dw[r], (uint32_t)(d->read_off[r + 1] - d->read_off[r])};
    b->rows_base_dw = (uint32_t)lay.zero_dw;
    *e = hipMemcpyAsync(d_reads.p, h_reads.p, (size_t)n_reads * sizeof(PhTab), hipMemcpyHostToDevice, ctx->copy);
    const LutPtrs lut = lut_ptrs(b->lut.p);
    if (*e == hipSuccess && agx_phmm_pk_rows_launch((const uint32_t *)b->img.p, (const PhTab *)d_reads.p, n_reads, lut.f, b->gatk_prior ? lut.mis_f : nullptr,
                                                    b->pk_rows.p, b->rows_base_dw, ctx->copy))
        *e = hipErrorLaunchFailure;
    return AGX_OK;
}

// Shared by the byte-track API and the probability-track seam.  When prob[] is non-NULL it holds
// the four probability tracks of every read (Qr,Qi,Qd,Qg concatenated per read, read_off units).
int create_batch(agx_ctx *ctx, const agx_phmm_desc *d, const double *const prob[4], int precision, agx_phmm_batch **out)
{
    if (!out) {
        agx_set_error("agx_phmm_batch_create: out is NULL");
        return AGX_E_ARG;
    }
    *out = nullptr;
    // ctx == NULL: plan only (no device needed) -- the batch answers agx_phmm_batch_info() and nothing else
    int rc = ctx ? agx_bind(ctx) : AGX_OK;
    if (rc) return rc;
    const bool gatk_prior = (precision & AGX_PHMM_GATK_PRIOR) != 0;
    precision &= ~AGX_PHMM_GATK_PRIOR;
    const bool probs = prob != nullptr;
    if ((rc = check_args(d, probs, precision))) return rc;
    const bool packed = precision == AGX_PHMM_F32_FMA;
    const bool trace = agx_tune("AGX_TRACE_CREATE") != nullptr;
    const double t_begin = agx_now_ms();

    std::unique_ptr<PlanSeed> seed_holder(new PlanSeed());
    PlanSeed &seed = *seed_holder;
    seed.n_cu = ctx ? ctx->n_cu : 256;
    seed.gatk_prior = gatk_prior;
    View view;
    if ((rc = narrow_view(d, view))) return rc;
    if (view.narrowed) d = &view.desc;
    if ((rc = check_lengths(d, view))) return rc;
    PairCount count;
    if ((rc = enumerate_pairs(d, seed.gen0, count))) return rc;
    seed.n_pairs = count.n_pairs;
    const std::vector<Plan> gen_long = split_long(d, precision, seed.gen0);
    ImageLayout lay;
    if ((rc = lay.lay(d, probs, seed.read_dw, seed.hap_dw))) return rc;

    // the create's staging blocks and its batch (made below) go back at every exit, an error exit draining the streams first
    PinBuf img_pin, stage, h_reads;
    DevBuf d_reads;
    agx_phmm_batch *b = nullptr;
    DrainOnError done(ctx, [&] {
        agx_phmm_batch_destroy(b);
        for (PinBuf *x : {&img_pin, &stage, &h_reads}) x->release();
        d_reads.release();
    });
    std::vector<uint32_t> img_heap;
    uint32_t *img = nullptr;
    if (ctx) {
        rc = img_pin.alloc(ctx, lay.img_dw * 4);
        if (rc) return rc;
        img = (uint32_t *)img_pin.p;
    } else {
        img_heap.resize(lay.img_dw);
        img = img_heap.data();
    }
    memset(img, 0, lay.zero_dw * 4);
    const bool have_tracks = has_tracks(d, probs);
    if (!seed.gen0.empty() && !have_tracks) {
        agx_set_error("agx_phmm_batch_create: NULL track");
        return AGX_E_ARG;
    }
    const ImageScan scan = have_tracks ? fill_image(d, prob, precision, lay, seed, img) : ImageScan{};
    if (trace) fprintf(stderr, "[phmm create] enumerate %.2f ms\n", agx_now_ms() - t_begin);

    const PlanChoice choice = choose_plan(ctx, d, precision, probs, have_tracks, lay, scan);
    const size_t n_work = seed.gen0.size();
    PlanOut pmain;
    // (the packed plan gets a copy of the pairs: the seed keeps them for the rescue plan)
    rc = packed ? make_plan(seed, seed.gen0, PlanKind{3, 2, false, false, trace, choice.trains}, pmain)
                : make_plan(seed, std::move(seed.gen0), PlanKind{precision, 1, !f32_family(precision), choice.lut_prior, trace, 1}, pmain);
    if (rc) return rc;
    StripePlan stripes;
    if ((rc = plan_stripes(gen_long, seed, stripes))) return rc;
    const double t_plan = agx_now_ms();

    const double t_pack = agx_now_ms();
    new_batch(b, ctx, BatchFacts{precision, probs, gatk_prior, count, n_work, lay.img_dw, seed.n_cu}, scan, choice, pmain, stripes);
    if (packed) b->rescue_seed = std::move(seed_holder); // (`seed` stays valid: the batch owns it now)
    if (trace) trace_digests(b, pmain, stripes.po, img, lay.img_dw, seed);
    if (!ctx) { // planning only
        *out = b;
        b = nullptr;
        done.ok = true;
        return AGX_OK;
    }
    hipError_t e = hipSuccess;
    if ((rc = upload(b, pmain, stripes.po, img, lay.img_dw, stage, &e))) return rc;
    if (e == hipSuccess && b->fast && !probs && lay.n_reads && !agx_tune("AGX_PHMM_NO_ROWS"))
        if ((rc = make_pk_rows(b, d, lay, seed, h_reads, d_reads, &e))) return rc;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy);
    if (e != hipSuccess) {
        agx_set_error("agx_phmm_batch_create: upload -> %s", hipGetErrorString(e));
        return AGX_E_HIP;
    }
    if (trace)
        fprintf(stderr, "[agx_phmm_batch_create] %lld pairs: plan+order %.2f ms, waves+pack %.2f ms, alloc+H2D %.2f ms (%.1f MB)\n",
                (long long)count.n_pairs, t_plan - t_begin, t_pack - t_plan, agx_now_ms() - t_pack, lay.img_dw * 4 / 1e6);
    *out = b;
    b = nullptr;
    done.ok = true; // the copy stream synchronised above
    return AGX_OK;
}

} // namespace

extern "C" {

void agx_phmm_batch_destroy(agx_phmm_batch *b)
{
    if (!b) return;
    if (b->ctx) (void)hipSetDevice(b->ctx->device);
    b->img.release();
    b->stripe_scratch.release();
    for (agx_phmm_batch::DevPlan *pl : {&b->main, &b->rescue, &b->stripe}) {
        pl->groups.release();
        pl->tabs.release();
        pl->waves.release();
    }
    b->sums.release();
    b->out_stage.release();
    b->bound_flag.release();
    b->pk_rows.release();
    b->lut.release();
    b->counter.release();
    agx_ctx_release(b->ctx); // the batch's own reference: a context outlives its batches
    delete b;
}

int agx_phmm_batch_create(agx_ctx *ctx, const agx_phmm_desc *d, int precision, agx_phmm_batch **out)
{
    AGX_GUARD_BEGIN
    return create_batch(ctx, d, nullptr, precision, out);
    AGX_GUARD_END("agx_phmm_batch_create")
}

int agx_phmm_batch_launch(agx_phmm_batch *b)
{
    if (!b) {
        agx_set_error("agx_phmm_batch_launch: null batch");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it cannot be launched");
        return AGX_E_NODEVICE;
    }
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    hipStream_t s = agx_enqueue_stream(b->ctx);
    const LutPtrs lut = lut_ptrs(b->lut.p);
    const bool f32 = f32_family(b->precision);
    // The two counters are zero at creation and are reset by whoever reads them (the log10 kernel of agx_phmm_batch_results; a
    // bound batch whose flag stayed clear has counted nothing): only a launch whose predecessor's counts nobody took resets
    // them itself.
    if (f32 && b->counters_dirty) AGX_HIP(hipMemsetAsync(b->counter.p, 0, 2 * sizeof(unsigned long long), s));
    b->counters_dirty = f32;
    b->rescue_pending = b->separate_rescue;
    if (b->bound) *(volatile unsigned *)b->bound_flag.p = 0; // set by the fill when a pair goes to the rescue plan
    const void *mis_for_d = b->gatk_prior ? lut.mis_d : nullptr, *mis_for_f = b->gatk_prior ? lut.mis_f : nullptr;
    auto launch_scalar = [&](const agx_phmm_batch::DevPlan &pl, const ClassLaunch &cl, int mode, hipStream_t st) -> int {
        const bool f64 = mode != 2;
        const size_t lds = mode == 3 && !b->separate_rescue ? cl.lds_rescue : cl.lds; // same records, wider table rows
        const int r = agx_phmm_launch_class(mode, cl.C, cl.all_g16, (const uint32_t *)b->img.p, (const PhGroup *)pl.groups.p,
                                            (const PhTab *)pl.tabs.p, (const PhWave *)pl.waves.p + cl.first_wave, cl.n_waves,
                                            f64 ? lut.d : lut.f, f64 ? mis_for_d : mis_for_f, (double *)b->sums.p,
                                            (double)AGX_PHMM_F32_RESCUE, (unsigned long long *)b->counter.p, lds, st);
        if (r) {
            agx_set_error("phmm_fill<C=%d, mode %d> launch failed: %s", cl.C, mode, hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
        return AGX_OK;
    };
    // the counter reset above is ordered before the fork; different classes run side by side
    {
        FanOut fan(b->ctx, (int)(b->main.launches.size() + b->stripe.launches.size()));
        rc = fan.begin();
        if (rc) return rc;
        int k = 0;
        for (const ClassLaunch &cl : b->stripe.launches) { // longest-running waves first
            const bool fma = b->precision == AGX_PHMM_F64_FMA || b->precision == AGX_PHMM_F32_FMA;
            const int mode = b->probs ? 4 : fma ? 1 : 0;
            // a float batch's long pairs are computed in double: stored negated like its rescued pairs
            const int r = agx_phmm_stripe_launch(mode, cl.C, (const uint32_t *)b->img.p, (const PhGroup *)b->stripe.groups.p,
                                                 (const PhTab *)b->stripe.tabs.p, (const PhWave *)b->stripe.waves.p, cl.n_waves,
                                                 b->stripe_grid, lut.d, b->stripe_mis_div ? nullptr : mis_for_d, b->stripe_mis_div ? 1 : 0, (double *)b->sums.p,
                                                 (double *)b->stripe_scratch.p, b->stripe_rows, f32 ? 1 : 0, cl.lds,
                                                 fan.stream(k++));
            if (r) {
                agx_set_error("phmm_fill_striped launch failed: %s", hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
        }
        for (const ClassLaunch &cl : b->main.launches) {
            hipStream_t st = fan.stream(k++);
            if (b->packed) {
                const PhUnderflow uf = PhUnderflow{(double)AGX_PHMM_F32_RESCUE, (uint32_t)b->n_pairs, (unsigned long long *)b->counter.p + 1,
                                                                   (double)(FLT_MAX / 16), (float)((b->gatk_prior ? kGuardGatk : kGuardRef) * 3.3219280948873623),
                                                                   b->bound, b->bound ? (unsigned *)b->bound_flag.p : nullptr, log10((double)(FLT_MAX / 16)),
                                                                   b->pk_rows.p, b->rows_base_dw};
                const int r = b->trains ? agx_phmm_pk_train_launch_class(cl.C, cl.all_g16, (const uint32_t *)b->img.p, (const PhGroup2 *)b->main.groups.p,
                                                                         (const PhTab *)b->main.tabs.p, (const PhWave *)b->main.waves.p + cl.first_wave,
                                                                         cl.n_waves, lut.f, mis_for_f, (double *)b->sums.p, uf, cl.lds, st)
                                        : agx_phmm_pk_launch_class(cl.C, cl.all_g16, b->fast, (const uint32_t *)b->img.p, (const PhGroup2 *)b->main.groups.p,
                                                                   (const PhTab *)b->main.tabs.p, (const PhWave *)b->main.waves.p + cl.first_wave,
                                                                   cl.n_waves, lut.f, mis_for_f, (double *)b->sums.p, uf, cl.lds, st);
                if (r) {
                    agx_set_error("phmm_fill_pk<C=%d> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
                    return AGX_E_HIP;
                }
            } else if (b->lut_prior) {
                const int r = agx_phmm_lut_launch_class(b->precision == AGX_PHMM_F64_FMA, cl.C, cl.all_g16, (const uint32_t *)b->img.p,
                                                        (const PhGroup *)b->main.groups.p, (const PhTab *)b->main.tabs.p,
                                                        (const PhWave *)b->main.waves.p + cl.first_wave, cl.n_waves, lut.d, mis_for_d,
                                                        (double *)b->sums.p, cl.lds, !agx_tune("AGX_PHMM_LUT_ONE_LOOP"), b->lut_ring, st);
                if (r) {
                    agx_set_error("phmm_fill_lut<C=%d> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
                    return AGX_E_HIP;
                }
            } else {
                int mode = b->precision;
                if (b->probs) mode = 4;
                rc = launch_scalar(b->main, cl, mode, st);
                // AGX_PHMM_F32: the double recomputation of underflowed pairs reuses the class's records
                if (!rc && b->precision == AGX_PHMM_F32) rc = launch_scalar(b->main, cl, 3, st);
                if (rc) return rc;
            }
        }
        rc = fan.end();
        if (rc) return rc;
    }
    return AGX_OK;
}

// The double rescue plan of a packed float batch (its own records over the same pairs): every wave looks at its pairs'
// float sums and recomputes those below the float range.  Run from agx_phmm_batch_results, when the fill counted any.
static int launch_rescue_plan(agx_phmm_batch *b)
{
    if (b->rescue_broken) {
        agx_set_error("agx_phmm_batch_results: the double rescue pass of this batch could not be planned earlier; create the batch again");
        return AGX_E_NOMEM;
    }
    if (b->rescue_seed) { // first underflow of this batch: plan the double pass over the same pairs and upload its records
        struct Broken { // any way out of this block but its end leaves the batch without the plan it needs
            agx_phmm_batch *b;
            bool done = false;
            ~Broken() { b->rescue_broken = !done; }
        } broken{b};
        PlanOut pr;
        const bool trace = agx_tune("AGX_TRACE_CREATE") != nullptr;
        std::unique_ptr<PlanSeed> seed = std::move(b->rescue_seed);
        int rc = make_plan(*seed, std::move(seed->gen0), PlanKind{AGX_PHMM_F64, 1, true, false, trace, 1}, pr);
        if (rc) return rc;
        if (trace) fprintf(stderr, "[agx_phmm_batch_create] plan digest rescue %016llx\n", (unsigned long long)plan_hash(AGX_PHMM_F64, 1, pr, pr.launches).h);
        StagedUpload up;
        up.pieces = {{&b->rescue.groups, pr.groups1.data(), pr.groups1.size() * sizeof(PhGroup)},
                     {&b->rescue.tabs, pr.tabs.data(), pr.tabs.size() * sizeof(PhTab)},
                     {&b->rescue.waves, pr.waves.data(), pr.waves.size() * sizeof(PhWave)}};
        PinBuf stage;
        DrainOnError done(b->ctx, [&] { stage.release(); }); // the records' blocks stay with the batch
        rc = up.alloc(b->ctx, stage);
        if (!rc && pr.launches.size() > 1) rc = agx_ctx_prepare_fanout(b->ctx);
        if (rc) return rc;
        AGX_HIP(up.queue(stage, nullptr, b->ctx->copy));
        AGX_HIP(hipStreamSynchronize(b->ctx->copy));
        done.ok = true;
        b->rescue.launches = pr.launches;
        broken.done = true;
    }
    const LutPtrs lut = lut_ptrs(b->lut.p);
    FanOut fan(b->ctx, (int)b->rescue.launches.size());
    int rc = fan.begin();
    if (rc) return rc;
    int k = 0;
    for (const ClassLaunch &cl : b->rescue.launches) {
        const int r = agx_phmm_launch_class(3, cl.C, cl.all_g16, (const uint32_t *)b->img.p, (const PhGroup *)b->rescue.groups.p,
                                            (const PhTab *)b->rescue.tabs.p, (const PhWave *)b->rescue.waves.p + cl.first_wave, cl.n_waves,
                                            lut.d, b->gatk_prior ? lut.mis_d : nullptr, (double *)b->sums.p, (double)AGX_PHMM_F32_RESCUE,
                                            (unsigned long long *)b->counter.p, cl.lds, fan.stream(k++));
        if (r) {
            agx_set_error("phmm_fill<C=%d, rescue> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
    }
    return fan.end();
}

int agx_phmm_batch_results(agx_phmm_batch *b, double *log10_lik, double *raw_sum)
{
    AGX_GUARD_BEGIN
    if (!b || (!log10_lik && b->n_pairs)) {
        agx_set_error("agx_phmm_batch_results: null argument");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no results");
        return AGX_E_NODEVICE;
    }
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    if (b->bound && log10_lik == b->bound && !raw_sum) {
        // bound results: the fill wrote them into this array itself; only a pair sent to the rescue plan (underflow,
        // accuracy guard) makes the long way below necessary
        AGX_HIP(hipStreamSynchronize(b->ctx->stream));
        if (*(volatile unsigned *)b->bound_flag.p == 0) {
            b->rescue_pending = false;
            b->info.n_rescued = 0;
            b->counters_dirty = false; // no pair was counted: the counters are still zero
            return AGX_OK;
        }
    }
    // through pinned staging on the launch stream: the DMAs queue right behind the last kernel
    const size_t sum_bytes = (size_t)b->n_pairs * sizeof(double);
    const bool f32 = f32_family(b->precision);
    // antidiagsPairHMM.c:242 -- both logarithms in double: by the host libm for the double modes (bit-identical to
    // the reference's output), by the device for the float modes (agx_phmm_finish_kernel.hip)
    const double c64 = log10(DBL_MAX / 16), c32 = log10((double)(FLT_MAX / 16));
    const bool want_sums = raw_sum != nullptr || !f32;
    char *const stage = (char *)b->out_stage.p; // [two counters][logs (float modes)][sums (when wanted)]
    volatile unsigned long long *host_counter = (volatile unsigned long long *)stage; // written by the log10 kernel itself
    double *s = nullptr, *dev_logs = nullptr;                                         // (float modes; the double modes have no rescue pass)
    hipStream_t st = agx_enqueue_stream(b->ctx);
    for (int round = 0; round < 2; ++round) {
        host_counter[0] = host_counter[1] = 0;
        char *at = stage + 16;
        if (f32 && b->n_pairs) {
            // the log10 kernel stores straight into page-locked host memory -- the caller's array when that is
            // page-locked (agx_host_alloc), else the staging block: consecutive 8-byte stores, no D2H copy behind it
            dev_logs = agx_is_pinned_host(log10_lik, sum_bytes) ? log10_lik : (double *)at;
            if (agx_phmm_finish_launch((const double *)b->sums.p, dev_logs, (uint32_t)b->n_pairs, c64, c32,
                                       (unsigned long long *)b->counter.p, (unsigned long long *)stage, st)) {
                agx_set_error("phmm_finish launch failed: %s", hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
            at += sum_bytes;
        }
        if (want_sums) {
            s = (double *)at;
            if (b->n_pairs && agx_copy_out_launch(b->sums.p, s, sum_bytes, st)) {
                agx_set_error("agx_phmm_batch_results: copy kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
                return AGX_E_HIP;
            }
            at += sum_bytes;
        }
        AGX_HIP(hipStreamSynchronize(st));
        // a packed float batch launches its double rescue plan only now, and only when the fill counted a pair below
        // the float range (config 3: never) -- then the results are taken a second time
        if (!(b->rescue_pending && host_counter[1] != 0)) break;
        b->rescue_pending = false;
        rc = launch_rescue_plan(b);
        if (rc) return rc;
    }
    b->rescue_pending = false;
    if (f32 && b->n_pairs) {
        if (b->counters_dirty) b->info.n_rescued = (int64_t)host_counter[0]; // (a second fetch without a launch in between finds them reset: the figure stays)
        b->counters_dirty = false;
    } else
        b->info.n_rescued = (int64_t)host_counter[0];
    if (f32) {
        if (b->n_pairs && dev_logs != log10_lik) memcpy(log10_lik, dev_logs, sum_bytes);
    } else
        agx_parallel_for(b->n_pairs, 2048, [&](int64_t lo, int64_t hi, int) {
            for (int64_t k = lo; k < hi; ++k) log10_lik[k] = log10(s[k]) - c64;
        });
    if (raw_sum && b->n_pairs) {
        if (f32) // the rescue pass stores its double-scaled sum negated so the two scalings stay apart: callers get |sum|
            for (int64_t k = 0; k < b->n_pairs; ++k) raw_sum[k] = s[k] < 0 ? -s[k] : s[k];
        else
            memcpy(raw_sum, s, sum_bytes);
    }
    return AGX_OK;
    AGX_GUARD_END("agx_phmm_batch_results")
}

int agx_phmm_batch_bind_results(agx_phmm_batch *b, double *log10_lik)
{
    if (!b) {
        agx_set_error("agx_phmm_batch_bind_results: null batch");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device)");
        return AGX_E_NODEVICE;
    }
    if (log10_lik && !agx_is_pinned_host(log10_lik, (size_t)std::max<int64_t>(b->n_pairs, 1) * sizeof(double))) {
        agx_set_error("agx_phmm_batch_bind_results: the array is not page-locked memory of agx_host_alloc (or too short for %lld results)", (long long)b->n_pairs);
        return AGX_E_ARG;
    }
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    AGX_HIP(hipStreamSynchronize(b->ctx->stream)); // launches in flight still write the old destination
    // taken by packed float batches whose records are in output order (one (R, H) shape, every pair with work); a hint otherwise
    const bool take = log10_lik && b->packed && b->file_order && b->n_pairs > 0;
    if (take && !b->bound_flag.p) {
        rc = b->bound_flag.alloc(b->ctx, 64);
        if (rc) return rc;
    }
    b->bound = take ? log10_lik : nullptr;
    return AGX_OK;
}

int agx_phmm_batch_info(const agx_phmm_batch *b, agx_phmm_info *info)
{
    if (!b || !info) {
        agx_set_error("agx_phmm_batch_info: null argument");
        return AGX_E_ARG;
    }
    *info = b->info;
    return AGX_OK;
}

int agx_phmm_forward(agx_ctx *ctx, const agx_phmm_desc *d, int precision, double *log10_lik)
{
    AGX_GUARD_BEGIN
    // A large batch goes through in pieces of whole regions (cut by cells, like the shards of agx_phmm_forward_devices):
    // piece k + 1 is enumerated, planned and uploaded while piece k is being filled, so the host's 3-4 ms for config 5's
    // 262 144 pairs hide behind the 12 ms of fills instead of standing in front of them.
    int pieces = 1;
    if (ctx && d && d->n_regions >= 2 && d->region_read && d->region_hap && d->read_off && d->hap_off) {
        double cells = 0;
        for (uint32_t g = 0; g < d->n_regions; ++g) {
            const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1], h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
            if (r1 < r0 || h1 < h0 || r1 > d->n_reads || h1 > d->n_haps) {
                cells = 0; // malformed: let the one-batch path report it
                break;
            }
            cells += (double)(d->read_off[r1] - d->read_off[r0]) * (double)(d->hap_off[h1] - d->hap_off[h0]);
        }
        pieces = (int)std::min<double>({8.0, cells / kPhmmPieceCells, (double)d->n_regions});
        if (pieces < 2) pieces = 1;
    }
    if (pieces == 1) {
        agx_phmm_batch *b = nullptr;
        int rc = agx_phmm_batch_create(ctx, d, precision, &b);
        if (rc) return rc;
        rc = agx_phmm_batch_launch(b);
        if (!rc) rc = agx_phmm_batch_results(b, log10_lik, nullptr);
        agx_phmm_batch_destroy(b);
        return rc;
    }
    std::vector<uint32_t> cut((size_t)pieces + 1);
    int rc = agx_phmm_shard_cuts(d, pieces, cut.data());
    if (rc) return rc;
    std::vector<agx_phmm_batch *> bs((size_t)pieces, nullptr);
    struct Cleanup {
        std::vector<agx_phmm_batch *> &v;
        ~Cleanup()
        {
            for (agx_phmm_batch *b : v) agx_phmm_batch_destroy(b);
        }
    } cleanup{bs};
    std::vector<int64_t> first_out((size_t)pieces + 1, 0);
    for (int k = 0; k < pieces; ++k) {
        int64_t n = 0;
        for (uint32_t g = cut[(size_t)k]; g < cut[(size_t)k + 1]; ++g)
            n += (int64_t)(d->region_read[g + 1] - d->region_read[g]) * (d->region_hap[g + 1] - d->region_hap[g]);
        first_out[(size_t)k + 1] = first_out[(size_t)k] + n;
        if (cut[(size_t)k + 1] <= cut[(size_t)k]) continue;
        agx_phmm_desc sub = *d;
        sub.region_read = d->region_read + cut[(size_t)k]; // absolute read / haplotype indices stay valid
        sub.region_hap = d->region_hap + cut[(size_t)k];
        sub.n_regions = cut[(size_t)k + 1] - cut[(size_t)k];
        rc = agx_phmm_batch_create(ctx, &sub, precision, &bs[(size_t)k]);
        if (!rc) rc = agx_phmm_batch_launch(bs[(size_t)k]);
        if (rc) return rc;
    }
    for (int k = 0; k < pieces; ++k) {
        if (!bs[(size_t)k]) continue;
        rc = agx_phmm_batch_results(bs[(size_t)k], log10_lik + first_out[(size_t)k], nullptr);
        if (rc) return rc;
        agx_phmm_batch_destroy(bs[(size_t)k]);
        bs[(size_t)k] = nullptr;
    }
    return AGX_OK;
    AGX_GUARD_END("agx_phmm_forward")
}

int agx_phmm_shard_cuts(const agx_phmm_desc *d, int n_shards, uint32_t *cut)
{
    if (!d || n_shards < 1 || !cut || (d->n_regions && (!d->region_read || !d->region_hap || !d->read_off || !d->hap_off))) {
        agx_set_error("agx_phmm_shard_cuts: bad arguments");
        return AGX_E_ARG;
    }
    for (uint32_t g = 0; g < d->n_regions; ++g) {
        const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1], h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
        if (r1 < r0 || h1 < h0 || r1 > d->n_reads || h1 > d->n_haps) {
            agx_set_error("region %u: ranges out of order or out of bounds", g);
            return AGX_E_ARG;
        }
    }
    // whole regions stay together, weighed by cells
    agx_cut_by_weight((int64_t)d->n_regions, n_shards, cut, [d](int64_t g) {
        const uint32_t r0 = d->region_read[g], r1 = d->region_read[g + 1], h0 = d->region_hap[g], h1 = d->region_hap[g + 1];
        return (double)(d->read_off[r1] - d->read_off[r0]) * (double)(d->hap_off[h1] - d->hap_off[h0]);
    });
    return AGX_OK;
}

int agx_phmm_forward_devices(const int *devices, int n_devices, const agx_phmm_desc *d, int precision, double *log10_lik)
{
    AGX_GUARD_BEGIN
    std::vector<int64_t> first_out; // [g]: the first result of region g
    auto cuts = [&](int64_t *cut) {
        std::vector<uint32_t> c((size_t)n_devices + 1);
        const int rc = agx_phmm_shard_cuts(d, n_devices, c.data());
        if (rc) return rc;
        std::copy(c.begin(), c.end(), cut);
        first_out.assign((size_t)d->n_regions + 1, 0);
        for (uint32_t g = 0; g < d->n_regions; ++g)
            first_out[g + 1] = first_out[g] + (int64_t)(d->region_read[g + 1] - d->region_read[g]) * (d->region_hap[g + 1] - d->region_hap[g]);
        return AGX_OK;
    };
    auto shard = [&](agx_ctx *c, int64_t lo, int64_t hi) {
        agx_phmm_desc sub = *d;
        sub.region_read = d->region_read + lo; // absolute read/hap indices stay valid
        sub.region_hap = d->region_hap + lo;
        sub.n_regions = (uint32_t)(hi - lo);
        return agx_phmm_forward(c, &sub, precision, log10_lik + first_out[(size_t)lo]);
    };
    const bool args_ok = d && (!d->n_regions || (d->region_read && d->region_hap && d->read_off && d->hap_off && log10_lik));
    return agx_run_shards("agx_phmm_forward_devices", devices, n_devices, args_ok, cuts, shard);
    AGX_GUARD_END("agx_phmm_forward_devices")
}

int agx_phmm_forward_multi(int n_devices, const agx_phmm_desc *d, int precision, double *log10_lik)
{
    int devs[1024];
    n_devices = agx_first_devices(n_devices, devs);
    return n_devices ? agx_phmm_forward_devices(devs, n_devices, d, precision, log10_lik) : AGX_E_NODEVICE;
}

void agx_pairHMM(double *likelihood, double *M, double *X, double *Y, char *R, char *H, int read_len, int haplotype_len,
                 double *Qr, double *Qi, double *Qd, double *Qg)
{
    (void)M;
    (void)X;
    (void)Y; // the reference's rolling anti-diagonal scratch (antidiagsPairHMM.c:452-455): unused here
    if (!likelihood) return;
    *likelihood = NAN;
    if (read_len < 0 || haplotype_len < 0 || !R || !H || !Qr || !Qi || !Qd || !Qg) {
        agx_set_error("agx_pairHMM: bad arguments");
        return;
    }
    try {
    agx_ctx *ctx = nullptr;
    std::mutex *busy = nullptr;
    if (agx_shared_ctx(0, 0, &ctx, &busy) != AGX_OK) return; // process-wide, created on first use
    // the context's own mutex, the one a shard of agx_*_devices on (device 0, slot 0) holds: calls take turns with those too
    std::lock_guard<std::mutex> turn(*busy);
    const uint64_t roff[2] = {0, (uint64_t)read_len}, hoff[2] = {0, (uint64_t)haplotype_len};
    const uint32_t reg[2] = {0, 1};
    agx_phmm_desc d{};
    d.read_bases = reinterpret_cast<const uint8_t *>(R);
    d.read_off = roff;
    d.n_reads = 1;
    d.hap_bases = reinterpret_cast<const uint8_t *>(H);
    d.hap_off = hoff;
    d.n_haps = 1;
    d.region_read = reg;
    d.region_hap = reg;
    d.n_regions = 1;
    const double *prob[4] = {Qr, Qi, Qd, Qg};
    agx_phmm_batch *b = nullptr;
    if (create_batch(ctx, &d, prob, AGX_PHMM_F64, &b) != AGX_OK) return;
    double v = NAN;
    if (agx_phmm_batch_launch(b) == AGX_OK && agx_phmm_batch_results(b, &v, nullptr) == AGX_OK) *likelihood = v;
    agx_phmm_batch_destroy(b);
    } catch (const std::exception &ex) {
        agx_set_error("agx_pairHMM: %s", ex.what());
    }
}

} // extern "C"
