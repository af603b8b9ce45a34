// Host side of the Smith-Waterman path: validation, lane-tiling choice, wave formation, uploads,
// launches, multi-device sharding (include/agx.h, "Smith-Waterman" section).
//
// What the host does per batch (agx_sw_batch_create), every step threaded over the process's pool:
//   A  one pass over len[]: orientation (shorter sequence across the lanes), limits, cell count
//   B  lane tiling per pair from a per-length lookup table (the lower envelope of the class cost lines),
//      then the batch-level rules: tail regime, class consolidation, dominant shape
//   C  two stable counting passes: long rows first, then (class, lanes per group)
//   D  waves, group records and image offsets in closed form per (class, G) bucket
// while the caller's `bases` and `off` arrays travel to the device as they are; a device kernel
// (agx_sw_pack_kernel.hip) then builds the padded image and checks the symbols.  No byte of a sequence
// is touched by the host.
//
// This file: the create of a score-only batch (which every other kind of batch is built on) -- create_batch, a driver over the
// stages defined ahead of it --, launch, scores and the one-shot and multi-device calls.  The planner (passes B to D: tiling tables,
// rules, sorts, layout, record writers) is in agx_sw_plan.cpp, align batches in agx_sw_align.cpp, banded ones in agx_sw_band.cpp,
// CIGARs in agx_sw_cigar.cpp; agx_sw_batch.h holds the batch object and what these files need of each other.
#include "agx_sw_batch.h"

#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "agx_parallel.h"

using namespace agx_sw_host;

namespace {

// Tuning build only (see agx_tune; the planner's knobs are in agx_sw_plan.cpp).  The shipped library runs on the defaults.
bool positive(long n) { return n > 0; }
int tuned_kernel() // AGX_SW_KERNEL; 0 = no override
{
    static const int v = [] {
        const char *e = agx_tune("AGX_SW_KERNEL");
        if (e && strcmp(e, "i32") == 0) return AGX_SW_KERNEL_INT32;
        if (e && strcmp(e, "pk1") == 0) return AGX_SW_KERNEL_PACKED_SIGNED;
        if (e && strcmp(e, "pk2") == 0) return AGX_SW_KERNEL_PACKED_BIASED;
        return 0;
    }();
    return v;
}
// agx_sw_score sends a large batch through in pieces (upload of piece k + 1 beside the fill of piece k); tuning build:
// AGX_SW_PIECE_MB, AGX_SW_PIECE_MIN_PAIRS
inline uint64_t piece_bytes() { static const uint64_t v = (uint64_t)agx_knob_int(agx_tune("AGX_SW_PIECE_MB"), 32, positive) << 20; return v; }
inline int64_t piece_min_pairs() { static const int64_t v = agx_knob_int(agx_tune("AGX_SW_PIECE_MIN_PAIRS"), 32768, positive); return v; }
// completion on the dispatch (ensure_done_event), taken off for an A/B: AGX_SW_DONE_EVENT=0
inline bool done_event_on()
{
    static const bool v = [] {
        const char *e = agx_tune("AGX_SW_DONE_EVENT");
        return !(e && e[0] == '0' && !e[1]);
    }();
    return v;
}
// AGX_TRACE_FETCH: a line for every bind_scores (was the array taken?) and every fetch from a bound array (what it waited for)
inline bool trace_fetch() { static const bool v = agx_tune("AGX_TRACE_FETCH") != nullptr; return v; }
constexpr size_t kRawPad = 64;       // bytes in front of and behind the uploaded sequences (16-byte aligned pieces, agx_sw_pack_kernel.hip)

} // namespace

namespace {
int finish_create(agx_sw_batch *b);
void drop_pending(agx_sw_batch *b);
int ensure_done_event(agx_sw_batch *b);
}

extern "C" {

void agx_sw_batch_destroy(agx_sw_batch *b)
{
    if (!b) return;
    if (b->ctx) (void)hipSetDevice(b->ctx->device);
    drop_pending(b);
    if (b->done) (void)hipEventDestroy(b->done);
    b->img.release();
    b->groups.release();
    b->waves.release();
    b->scores.release();
    b->table.release();
    b->out_stage.release();
    b->ends.release();
    b->ends_stage.release();
    b->lstat.release();
    b->lstat_stage.release();
    b->band_pos.release();
    b->band_pos_stage.release();
    b->band_stop.release();
    b->band_stop_stage.release();
    b->goff.release();
    b->walkrec.release();
    agx_ctx_release(b->ctx); // the batch's own reference: a context outlives its batches
    delete b;
}

int agx_sw_batch_create(agx_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                        agx_sw_batch **out)
{
    return agx_sw_batch_create_scored(ctx, nullptr, bases, off, len, n_pairs, out);
}

int agx_sw_batch_create_scored(agx_ctx *ctx, const agx_sw_scoring *scoring, const uint8_t *bases, const uint64_t *off,
                               const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    AGX_GUARD_BEGIN
    return create_batch(ctx, scoring, nullptr, bases, off, len, n_pairs, out);
    AGX_GUARD_END("agx_sw_batch_create")
}

int agx_sw_batch_create_matrix(agx_ctx *ctx, const agx_sw_matrix *matrix, const uint8_t *bases, const uint64_t *off,
                               const uint32_t *len, int64_t n_pairs, agx_sw_batch **out)
{
    if (!matrix) {
        agx_set_error("agx_sw_batch_create_matrix: matrix is NULL");
        return AGX_E_ARG;
    }
    AGX_GUARD_BEGIN
    return create_batch(ctx, nullptr, matrix, bases, off, len, n_pairs, out);
    AGX_GUARD_END("agx_sw_batch_create_matrix")
}

} // extern "C"

namespace {

// Batches of at least this many pairs are candidates for the device planner: below it the host's threaded passes
// take well under a millisecond and the batch is in the tail regime anyway.
constexpr int64_t kDevPlanMinPairs = 49152;

// temporaries of a device-planned batch (released when create_batch leaves)
struct DevPlan {
    PinBuf h_len, h_buckets, h_padded;
    DevBuf d_len, d_buckets, d_padded, keys_a, keys_b, vals_a, vals_b, wkeys_a, wkeys_b, wids_a, wids_b, waves_tmp, temp;
    std::vector<uint32_t> hist; // pairs per (class, G) bucket
    size_t img_dw = 0;
    hipEvent_t uploaded = nullptr; // recorded on the copy stream behind this batch's sequences
    hipEvent_t done = nullptr; // recorded behind this batch's planning kernels (its own: two creates may be in flight on one context)
    void release()
    {
        if (done) (void)hipEventDestroy(done);
        if (uploaded) (void)hipEventDestroy(uploaded);
        done = uploaded = nullptr;
        for (PinBuf *x : {&h_len, &h_buckets, &h_padded}) x->release();
        for (DevBuf *x : {&d_len, &d_buckets, &d_padded, &keys_a, &keys_b, &vals_a, &vals_b, &wkeys_a, &wkeys_b, &wids_a, &wids_b, &waves_tmp, &temp})
            x->release();
    }
};

// A pageable source on its way to the device: the runtime's own staging moved fresh pages at 4-5 GB/s (25-35 ms per 143 MB chunk
// of the command line).  Staged here instead: slices are copied by a few threads into a ring of pinned blocks, each slice's DMA
// runs while the next is being copied.
int copy_through_ring(agx_ctx *ctx, uint8_t *dst, const uint8_t *src, size_t bytes, size_t slice)
{
    constexpr int kRing = 3;
    PinBuf ring[kRing];
    hipEvent_t done[kRing] = {nullptr, nullptr, nullptr};
    int r = AGX_OK;
    for (int k = 0; k < kRing && !r; ++k) {
        r = ring[k].alloc(ctx, slice);
        if (!r && hipEventCreateWithFlags(&done[k], hipEventDisableTiming) != hipSuccess) r = AGX_E_HIP;
    }
    size_t at = 0;
    for (int k = 0; !r && at < bytes; ++k, at += slice) {
        const int slot = k % kRing;
        const size_t n = std::min(slice, bytes - at);
        if (k >= kRing && hipEventSynchronize(done[slot]) != hipSuccess) r = AGX_E_HIP;
        const int parts = std::max(1, agx_host_threads()); // every pool thread: 4 (round 2) and 8 copied a 16 MB slice in 0.4 ms, above its 0.29 ms DMA
        const size_t per = (n + parts - 1) / parts;
        agx_pool_run(parts, [&](int t) {
            const size_t lo = std::min(n, (size_t)t * per), hi = std::min(n, lo + per);
            if (lo < hi) agx_stream_copy((uint8_t *)ring[slot].p + lo, src + at + lo, hi - lo);
        });
        if (!r && (hipMemcpyAsync(dst + at, ring[slot].p, n, hipMemcpyHostToDevice, ctx->copy) != hipSuccess || hipEventRecord(done[slot], ctx->copy) != hipSuccess))
            r = AGX_E_HIP;
    }
    for (int k = 0; k < kRing; ++k) {
        if (done[k]) {
            (void)hipEventSynchronize(done[k]); // the ring goes back to the pool: its DMAs must be over
            (void)hipEventDestroy(done[k]);
        }
        ring[k].release();
    }
    return r;
}

// The caller's arrays start travelling while the plan is made: the sequences (as they are, or a dense copy), their offsets, the
// matrix's code table and the symbol check's flag, queued on the copy stream -- by a helper thread, because a pageable source
// makes hipMemcpyAsync block while the runtime stages it.  Owns the device blocks the pack kernel reads and the thread.
struct Uploader {
    DevBuf d_raw, d_off, d_code, d_flag;
    PinBuf h_dense, h_dense_off;
    uint64_t raw_bytes = 0; // what goes up: the extent of `bases` the batch uses, or its sequences alone
    uint64_t raw_base = 0;  // the offset in `bases` of the first byte uploaded
    std::thread thread;

    // queues the copies inline when nothing would block, on the thread otherwise; without a device (or pairs) only the extents
    void start(agx_ctx *ctx_, const agx_sw_matrix *matrix_, const uint8_t *bases_, const uint64_t *off_, const uint32_t *len_, int64_t n_pairs_,
               uint64_t ext_lo_, uint64_t ext_hi, uint64_t sum_len_)
    {
        ctx = ctx_, matrix = matrix_, bases = bases_, off = off_, len = len_, n_pairs = n_pairs_, ext_lo = ext_lo_, sum_len = sum_len_;
        // `bases` is normally dense; a caller whose sequences are islands in a much larger array gets a dense
        // copy (pinned, its own offsets) instead of an upload of the gaps
        dense_copy = (ext_hi - ext_lo) > 4 * sum_len + ((uint64_t)64 << 20);
        raw_bytes = dense_copy ? sum_len : ext_hi - ext_lo;
        raw_base = dense_copy ? 0 : ext_lo;
        if (!ctx || n_pairs <= 0) return;
        // page-locked arrays (agx_host_alloc) go down without the runtime staging anything: hipMemcpyAsync returns at once,
        // and the helper thread -- 50 us to start and join, a tenth of a config-2-sized call -- is not needed
        const bool queued_at_once = !dense_copy && !matrix && agx_is_pinned_host(bases + ext_lo, (size_t)raw_bytes) &&
                                    agx_is_pinned_host(off, (size_t)n_pairs * 2 * sizeof(uint64_t));
        if (queued_at_once) run();
        else thread = std::thread([this] { run(); });
    }
    // everything is queued (or has failed: the error text is set)
    int join()
    {
        if (thread.joinable()) thread.join();
        if (rc) agx_set_error("%s", err);
        return rc;
    }
    void release() // (the thread has been joined: every exit of create_batch does, see DrainOnError)
    {
        for (DevBuf *x : {&d_raw, &d_off, &d_code, &d_flag}) x->release();
        for (PinBuf *x : {&h_dense, &h_dense_off}) x->release();
    }

private:
    agx_ctx *ctx = nullptr;
    const agx_sw_matrix *matrix = nullptr;
    const uint8_t *bases = nullptr;
    const uint64_t *off = nullptr;
    const uint32_t *len = nullptr;
    int64_t n_pairs = 0;
    uint64_t ext_lo = 0, sum_len = 0;
    bool dense_copy = false;
    int rc = AGX_OK; // the thread's verdict, read after the join (its error text cannot go through agx_set_error: another thread)
    char err[300] = "";

    void run()
    {
        try {
            if (hipSetDevice(ctx->device) != hipSuccess) {
                rc = AGX_E_HIP;
                snprintf(err, sizeof err, "hipSetDevice failed on the upload thread");
                return;
            }
            int r = d_raw.alloc(ctx, (size_t)raw_bytes + 2 * kRawPad); // the pack kernels read 16-byte pieces that may begin before / end behind the sequences
            if (!r) r = d_off.alloc(ctx, (size_t)n_pairs * 2 * sizeof(uint64_t));
            if (!r) r = d_flag.alloc(ctx, 2 * sizeof(uint32_t));
            if (!r && matrix) r = d_code.alloc(ctx, 256);
            const uint8_t *src = bases + ext_lo;
            const uint64_t *src_off = off;
            if (!r && dense_copy) {
                r = h_dense.alloc(ctx, (size_t)sum_len + 16);
                if (!r) r = h_dense_off.alloc(ctx, (size_t)n_pairs * 2 * sizeof(uint64_t));
                if (!r) {
                    uint64_t *o = (uint64_t *)h_dense_off.p, at = 0;
                    for (int64_t k = 0; k < 2 * n_pairs; ++k) {
                        o[k] = at;
                        if (len[k]) memcpy((uint8_t *)h_dense.p + at, bases + off[k], len[k]);
                        at += len[k];
                    }
                    src = (const uint8_t *)h_dense.p;
                    src_off = o;
                }
            }
            if (r) {
                rc = r;
                snprintf(err, sizeof err, "%s", agx_last_error());
                return;
            }
            hipError_t e = hipSuccess;
            // Pinned sources go down in one DMA, pageable ones through the ring
            // (known page-locked = allocated by agx_host_alloc; anything else is treated as pageable)
            constexpr size_t kSlice = (size_t)16 << 20;
            const bool pageable = raw_bytes > 2 * kSlice && !dense_copy && !agx_is_pinned_host(src, (size_t)raw_bytes);
            if (pageable) {
                if (copy_through_ring(ctx, (uint8_t *)d_raw.p + kRawPad, src, (size_t)raw_bytes, kSlice)) e = hipErrorUnknown;
            } else if (raw_bytes)
                e = hipMemcpyAsync((uint8_t *)d_raw.p + kRawPad, src, (size_t)raw_bytes, hipMemcpyHostToDevice, ctx->copy);
            if (e == hipSuccess)
                e = hipMemcpyAsync(d_off.p, src_off, (size_t)n_pairs * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->copy);
            if (e == hipSuccess && matrix) e = hipMemcpyAsync(d_code.p, matrix->code, 256, hipMemcpyHostToDevice, ctx->copy);
            if (e == hipSuccess) e = hipMemsetAsync(d_flag.p, 0, 4, ctx->copy);                    // [0] offending pairs
            if (e == hipSuccess) e = hipMemsetAsync((char *)d_flag.p + 4, 0xff, 4, ctx->copy);     // [1] smallest of them
            if (e != hipSuccess) {
                rc = AGX_E_HIP;
                snprintf(err, sizeof err, "upload of the sequences -> %s", hipGetErrorString(e));
            }
        } catch (const std::exception &ex) {
            rc = AGX_E_NOMEM;
            snprintf(err, sizeof err, "upload thread: %s", ex.what());
        }
    }
};

} // namespace

// everything a create leaves behind while its device work is still in flight
struct SwPending {
    Uploader up;
    PinBuf h_groups, h_waves, h_flag;
    DevPlan dp;
    hipStream_t tail = nullptr; // the stream the pack kernel and the verdict's copy were queued on
    hipEvent_t ready = nullptr; // recorded behind them: what a launch waits for
    bool device_plan = false, matrix = false;
    ~SwPending()
    {
        // a deferred batch destroyed before finish_create: its kernels may still read the temporaries (tail covers the
        // copy and planning streams)
        if (tail) (void)hipStreamSynchronize(tail);
        if (ready) (void)hipEventDestroy(ready);
        dp.release();
        up.release();
        for (PinBuf *x : {&h_groups, &h_waves, &h_flag}) x->release();
    }
};

namespace {

void drop_pending(agx_sw_batch *b)
{
    delete b->pending;
    b->pending = nullptr;
}

void set_symbol_error(bool matrix, long long pair)
{
    if (matrix)
        agx_set_error("pair %lld contains a byte outside the substitution matrix's alphabet", pair);
    else
        agx_set_error("pair %lld contains byte 0x00, which is reserved as the padding symbol", pair);
}

// The closing wait of a create, blocking or deferred, for the stream its pack kernel and verdict copy were queued on: then the
// device planner's padded-cell count and the symbol check's verdict are on the host.
int wait_for_verdict(agx_sw_batch *b, const SwPending &p, hipStream_t tail)
{
    const hipError_t e = hipStreamSynchronize(tail);
    if (e != hipSuccess) {
        agx_set_error("agx_sw_batch_create: upload -> %s", hipGetErrorString(e));
        return AGX_E_HIP;
    }
    if (p.device_plan) b->info.padded_cells = (int64_t) * (const unsigned long long *)p.dp.h_padded.p; // (the planning stream ended before the pack kernel began)
    const uint32_t *flag = (const uint32_t *)p.h_flag.p;
    if (flag && flag[0]) {
        set_symbol_error(p.matrix, flag[1]);
        return AGX_E_SYMBOL;
    }
    return AGX_OK;
}

// the closing wait of a deferred create
int finish_create(agx_sw_batch *b)
{
    if (!b->pending) return AGX_OK;
    const int rc = wait_for_verdict(b, *b->pending, b->pending->tail);
    drop_pending(b);
    return rc;
}

// the family-2 tiling table on the device, made on the context's first device-planned batch
int ensure_device_table(agx_ctx *ctx, hipStream_t s)
{
    if (ctx->sw_seg_first) return AGX_OK;
    const TilingTable &tt = full_tiling_table(2);
    std::vector<uint32_t> segs(tt.segs.size());
    for (size_t k = 0; k < segs.size(); ++k) segs[k] = (tt.segs[k].ly_from & 0xffffu) | ((uint32_t)tt.segs[k].cls << 16) | ((uint32_t)tt.segs[k].G << 24);
    void *d_first = nullptr, *d_segs = nullptr;
    AGX_HIP(hipMalloc(&d_first, tt.first.size() * sizeof(uint32_t)));
    if (hipMalloc(&d_segs, std::max<size_t>(segs.size(), 1) * sizeof(uint32_t)) != hipSuccess) {
        (void)hipFree(d_first);
        agx_set_error("device tiling table: out of device memory");
        return AGX_E_NOMEM;
    }
    // (pageable sources: these two copies return when the data has left the host buffers)
    hipError_t e = hipMemcpyAsync(d_first, tt.first.data(), tt.first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !segs.empty()) e = hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(d_first);
        (void)hipFree(d_segs);
        agx_set_error("device tiling table: upload -> %s", hipGetErrorString(e));
        return AGX_E_HIP;
    }
    ctx->sw_seg_first = d_first;
    ctx->sw_segs = d_segs;
    return AGX_OK;
}

// Allocates the batch's record arrays and the planner's temporaries, uploads len[] and the bucket table and queues the
// planning kernels on the context's planning stream (the pack kernel follows them there).
int launch_device_plan(agx_ctx *ctx, DevPlan &dp, agx_sw_batch *b, uint32_t n_pairs, uint32_t n_fill, uint32_t longest_long, int slots, uint32_t img0,
                       size_t n_groups, size_t n_waves)
{
    hipStream_t ps = ctx->plan;
    agx_sw_plan_preload();
    int rc;
    {
        static std::mutex once_per_context; // the table is made by whichever create comes first
        std::lock_guard<std::mutex> l(once_per_context);
        rc = ensure_device_table(ctx, ps);
    }
    if (!rc && (hipEventCreateWithFlags(&dp.done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&dp.uploaded, hipEventDisableTiming) != hipSuccess)) {
        agx_set_error("device planner: cannot create an event");
        rc = AGX_E_HIP;
    }
    const size_t pw = (size_t)n_pairs * sizeof(uint32_t), ww = std::max<size_t>(n_waves, 1) * sizeof(uint32_t);
    const size_t temp_bytes = agx_sw_plan_temp_bytes(n_pairs, (uint32_t)n_waves);
    if (!rc) rc = b->groups.alloc(ctx, std::max<size_t>(n_groups, 1) * sizeof(SwGroup2));
    if (!rc) rc = b->waves.alloc(ctx, std::max<size_t>(n_waves, 1) * sizeof(SwWave));
    if (!rc) rc = dp.d_len.alloc(ctx, 2 * pw);
    if (!rc) rc = dp.d_buckets.alloc(ctx, dp.h_buckets.bytes);
    if (!rc) rc = dp.d_padded.alloc(ctx, 64);
    if (!rc) rc = dp.h_padded.alloc(ctx, 64);
    for (DevBuf *x : {&dp.keys_a, &dp.keys_b, &dp.vals_a, &dp.vals_b})
        if (!rc) rc = x->alloc(ctx, pw);
    for (DevBuf *x : {&dp.wkeys_a, &dp.wkeys_b, &dp.wids_a, &dp.wids_b})
        if (!rc) rc = x->alloc(ctx, ww);
    if (!rc) rc = dp.waves_tmp.alloc(ctx, std::max<size_t>(n_waves, 1) * sizeof(SwWave));
    if (!rc) rc = dp.temp.alloc(ctx, temp_bytes);
    if (rc) return rc;
    AGX_HIP(hipMemcpyAsync(dp.d_len.p, dp.h_len.p, 2 * pw, hipMemcpyHostToDevice, ps));
    AGX_HIP(hipMemcpyAsync(dp.d_buckets.p, dp.h_buckets.p, dp.h_buckets.bytes, hipMemcpyHostToDevice, ps));
    AGX_HIP(hipMemsetAsync(dp.d_padded.p, 0, 8, ps));
    SwPlanArgs a{};
    a.len = (const uint32_t *)dp.d_len.p;
    a.n_pairs = n_pairs;
    a.n_fill = n_fill;
    a.seg_first = (const uint32_t *)ctx->sw_seg_first;
    a.segs = (const uint32_t *)ctx->sw_segs;
    a.longest = longest_long;
    a.buckets = (const uint32_t *)dp.d_buckets.p;
    a.img0 = img0;
    a.slots = slots;
    a.n_waves = (uint32_t)n_waves;
    a.keys_a = (uint32_t *)dp.keys_a.p, a.keys_b = (uint32_t *)dp.keys_b.p, a.vals_a = (uint32_t *)dp.vals_a.p, a.vals_b = (uint32_t *)dp.vals_b.p;
    a.wave_keys_a = (uint32_t *)dp.wkeys_a.p, a.wave_keys_b = (uint32_t *)dp.wkeys_b.p, a.wave_ids_a = (uint32_t *)dp.wids_a.p, a.wave_ids_b = (uint32_t *)dp.wids_b.p;
    a.waves_tmp = (SwWave *)dp.waves_tmp.p;
    a.waves = (SwWave *)b->waves.p;
    a.groups = (uint32_t *)b->groups.p;
    a.padded = (unsigned long long *)dp.d_padded.p;
    a.temp = dp.temp.p;
    a.temp_bytes = temp_bytes;
    a.n_cu = ctx->n_cu;
    if (agx_sw_plan_launch(a, ps)) {
        agx_set_error("device planner: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return AGX_E_HIP;
    }
    AGX_HIP(hipMemcpyAsync(dp.h_padded.p, dp.d_padded.p, 8, hipMemcpyDeviceToHost, ps));
    AGX_HIP(hipEventRecord(dp.done, ps));
    return AGX_OK;
}

// AGX_TRACE_CREATE: a host-made plan as one number, 64-bit FNV-1a (agx_internal.h) over the kernel choice (family, rising, wide,
// stage as int32), the launches (C, first_wave, n_waves), the wave and group records as they go to the device and, for the traced
// fill, its offsets and walk records field by field (no struct padding).  tests/test_sw_plan_digest_cpu.py pins it per kind of
// batch.  hash_head: the kernel choice and the launches, what a plan says before its records
void hash_head(Fnv1a &f, const agx_sw_batch *b)
{
    for (int32_t v : {(int32_t)b->family, (int32_t)b->rising, (int32_t)b->wide, (int32_t)b->stage}) f.field(v);
    hash_launches(f, b->launches);
}
uint64_t plan_digest(const agx_sw_batch *b, const std::vector<SwWave> &waves, const void *groups, size_t groups_bytes)
{
    Fnv1a f;
    hash_head(f, b);
    f.bytes(waves.data(), waves.size() * sizeof(SwWave));
    f.bytes(groups, groups_bytes);
    if (b->cigar == 2) {
        f.bytes(b->tr_goff.data(), b->tr_goff.size() * sizeof(uint64_t));
        f.field(b->tr_dwords);
        f.field(b->tr_slot_words);
        for (const SwWalkRec &r : b->tr_walk) {
            f.field(r.goff), f.field(r.x_dw), f.field(r.y_dw), f.field(r.ca), f.field(r.cb), f.field(r.G), f.field(r.C), f.field(r.slot);
        }
    }
    return f.h;
}

// AGX_TRACE_CREATE: the same plan part by part, each hashed afresh, so that two digests that differ say where: the head (kernel
// choice and launches), the wave records, the group records; then the groups, how many of them have a vacant second half (a
// packed plan's group whose second score slot is the spare one, n_pairs) and the columns per lane of every launch.
void trace_plan_parts(const agx_sw_batch *b, bool packed, const std::vector<SwWave> &waves, const void *groups, size_t groups_bytes)
{
    Fnv1a head, wv, gr;
    hash_head(head, b);
    wv.bytes(waves.data(), waves.size() * sizeof(SwWave));
    gr.bytes(groups, groups_bytes);
    const size_t n_groups = groups_bytes / (packed ? sizeof(SwGroup2) : sizeof(SwGroup));
    size_t vacant = 0;
    if (packed)
        for (size_t g = 0; g < n_groups; ++g) vacant += ((const SwGroup2 *)groups)[g].out[1] == (uint32_t)b->n_pairs;
    std::string cs;
    for (const ClassLaunch &cl : b->launches) cs += " " + std::to_string(cl.C);
    fprintf(stderr, "[agx_sw_batch_create] plan parts: head %016llx waves %016llx groups %016llx; %zu groups, %zu vacant halves; launch C%s\n",
            (unsigned long long)head.h, (unsigned long long)wv.h, (unsigned long long)gr.h, n_groups, vacant, cs.empty() ? " none" : cs.c_str());
}

// ---- the stages of create_batch, in the order it calls them.  Each reads what it is given and fills a result of its own.

// what kind of batch a create makes, beyond its scoring: the arguments of create_batch that select kernels and limits
struct BatchKind {
    const agx_sw_matrix *matrix;
    int align, mode, stats, cigar;
};

// ---- the arguments: the arrays of the pairs, and (after the scoring has been checked) the symbols behind them
int check_arrays(const uint64_t *off, const uint32_t *len, int64_t n_pairs)
{
    if (n_pairs < 0 || (n_pairs > 0 && (!off || !len))) {
        agx_set_error("agx_sw_batch_create: bad arguments (n_pairs=%lld)", (long long)n_pairs);
        return AGX_E_ARG;
    }
    if (n_pairs > 0x7fffffffLL / 2) {
        agx_set_error("agx_sw_batch_create: more than 2^30 pairs in one batch");
        return AGX_E_LIMIT;
    }
    return AGX_OK;
}
int check_bases(const uint8_t *bases, const uint32_t *len, int64_t n_pairs)
{
    if (n_pairs > 0 && !bases)
        for (int64_t p = 0; p < 2 * n_pairs; ++p)
            if (len[p]) {
                agx_set_error("agx_sw_batch_create: bases is NULL");
                return AGX_E_ARG;
            }
    return AGX_OK;
}

// ---- scoring -> kernel constants
struct SwConstants {
    agx_sw_scoring sc{};
    std::vector<int16_t> table; // matrix mode: [kSwMatDim][kSwMatDim], row/column 0 = padding
    SwParams prm{};
    int bias = 0; // B of the biased packed fill
};
int make_constants(const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, SwConstants &k)
{
    const agx_sw_scoring ref_scoring = AGX_SW_SCORING_REFERENCE;
    agx_sw_scoring &sc = k.sc;
    sc = scoring ? *scoring : ref_scoring;
    if (matrix) {
        const int n = matrix->n_symbols;
        if (n < 1 || n > AGX_SW_MATRIX_MAX_SYMBOLS) {
            agx_set_error("substitution matrix: %d symbols, supported 1..%d", n, AGX_SW_MATRIX_MAX_SYMBOLS);
            return AGX_E_ARG;
        }
        int lo = 0;
        for (int a = 0; a < n; ++a)
            for (int c = 0; c < n; ++c) {
                if (matrix->score[a][c] != matrix->score[c][a]) {
                    agx_set_error("substitution matrix is not symmetric at (%d, %d)", a, c);
                    return AGX_E_ARG;
                }
                lo = std::min(lo, (int)matrix->score[a][c]);
            }
        for (int c = 0; c < 256; ++c)
            if (matrix->code[c] != 0xff && matrix->code[c] >= n) {
                agx_set_error("substitution matrix: code[%d] = %d is not a symbol number below %d", c, matrix->code[c], n);
                return AGX_E_ARG;
            }
        // the generic range check below sees a match/mismatch pair that always passes
        sc = agx_sw_scoring{1, 0, matrix->gap_open, matrix->gap_extend};
        const int gf = matrix->gap_open + matrix->gap_extend;
        // padding cells score the matrix minimum (<= 0): they cannot raise a local-alignment maximum
        k.table.assign((size_t)kSwMatDim * kSwMatDim, (int16_t)(lo - gf));
        for (int a = 0; a < n; ++a)
            for (int c = 0; c < n; ++c) k.table[(size_t)(a + 1) * kSwMatDim + (c + 1)] = (int16_t)(matrix->score[a][c] - gf);
    }
    // mismatch <= 0: padding relies on never-matching symbols not raising a score
    if (sc.match < 1 || sc.match > 12 || sc.mismatch > 0 || sc.mismatch < sc.match - 128 || sc.gap_open > 0 ||
        sc.gap_open < -1000 || sc.gap_extend > 0 || sc.gap_extend < -1000) {
        agx_set_error("scoring {match %d, mismatch %d, open %d, extend %d} outside the supported range", sc.match,
                      sc.mismatch, sc.gap_open, sc.gap_extend);
        return AGX_E_LIMIT;
    }
    SwParams &prm = k.prm;
    prm.ge = sc.gap_extend;
    prm.gf = sc.gap_open + sc.gap_extend;
    prm.hd = sc.match - prm.gf;
    prm.delta = sc.match - sc.mismatch;
    prm.shift = 0;
    while ((1 << prm.shift) < prm.delta) ++prm.shift;
    auto twice = [](int v) { return (uint32_t)(uint16_t)(int16_t)v * 0x10001u; };
    prm.ge2 = twice(prm.ge);
    prm.gf2 = twice(prm.gf);
    prm.hd2 = twice(prm.hd);
    prm.delta2 = twice(prm.delta);
    prm.age2 = twice(-prm.ge);
    prm.agf2 = twice(-prm.gf);
    k.bias = 0x0400 + std::max(-prm.gf - prm.ge, prm.delta);
    prm.bias2 = twice(k.bias);
    return AGX_OK;
}

// ---- where the per-pair passes of the planner will run.  A large batch for the packed biased fill is a candidate
// for the device planner (agx_sw_plan_kernel.hip): pass A then only reduces -- no per-pair record is written on the
// host -- and the batch-level rules decide later whether the candidate stands (a uniform batch, one in the tail
// regime or with a dominant shape is planned on the host as before).
bool device_plan_candidate(const agx_ctx *ctx, const BatchKind &kind, int64_t n_pairs, int want)
{
    const int planner_opt = ctx ? ctx->opt_sw_planner : AGX_SW_PLANNER_HOST;
    return ctx && !kind.matrix && !kind.align && planner_opt != AGX_SW_PLANNER_HOST && n_pairs > 0 &&
           (planner_opt == AGX_SW_PLANNER_DEVICE || n_pairs >= kDevPlanMinPairs) &&
           (want == AGX_SW_KERNEL_AUTO || want == AGX_SW_KERNEL_PACKED_BIASED) && tail_beta_override() < 0 &&
           !max_classes_override() && !agx_tune("AGX_SW_SORT_WAVES") && !agx_tune("AGX_SW_ONE_LAUNCH") &&
           !agx_tune("AGX_SW_WAVES_PER_CLASS") && !agx_tune("AGX_SW_HOST_PLAN");
}

// no wide classes in matrix mode; an align batch lays the FIRST sequence across the lanes (agx_sw_loc_kernel.hip), its limit is on that one
// (a stats batch: the classes the stats builds exist for bound the query, also where the batch's own fill is the plain one --
// its begin pass is not)
// (a cigar batch: likewise the classes the traced builds exist for)
uint32_t longest_short_allowed(const BatchKind &kind)
{
    return kind.stats    ? (uint32_t)AGX_SW_STATS_MAX_QUERY_LEN
           : kind.cigar  ? (uint32_t)AGX_SW_CIGAR_MAX_QUERY_LEN
           : kind.matrix ? (uint32_t)kSwPackedMaxShort
           : kind.align  ? (uint32_t)AGX_SW_ALIGN_MAX_QUERY_LEN
                         : AGX_SW_MAX_SHORT_LEN;
}

// ---- pass A (threads over pairs): orient, check the limits, count cells, extent of `bases`
struct PassA {
    std::vector<PairPlan> all; // want_records: every pair, oriented, not yet tiled
    int64_t cells = 0, n_fill = 0; // n_fill: pairs with something to fill
    uint32_t longest_short = 0, longest_long = 0;
    uint64_t ext_lo = ~0ull, ext_hi = 0, sum_len = 0; // the bytes of `bases` the batch uses
    std::vector<uint8_t> present;                     // [lx] != 0: some pair has that shorter length
    bool one_shape = true;                            // every pair with something to fill has the shape `shape` (lx << 16 | ly)
    uint32_t shape = 0xffffffffu;
};
int pass_a(const uint64_t *off, const uint32_t *len, int64_t n_pairs, int align, uint32_t hard_max_short, bool want_records, PassA &a)
{
    struct alignas(128) Worker { // a cache line pair of its own: every thread updates its part per pair
        int64_t bad_pair = -1; // the first pair of this part beyond the limits
        int64_t cells = 0, n_fill = 0;
        uint32_t longest_short = 0, longest_long = 0;
        uint32_t shape0 = 0xffffffffu; // first (lx, ly) this part saw
        bool mixed = false;            // ... and whether it saw another one
        uint64_t lo = ~0ull, hi = 0, sum_len = 0;
        std::vector<uint8_t> present; // [lx] != 0: this part saw that shorter length
    };
    if (want_records) a.all.resize((size_t)n_pairs);
    PairPlan *allp = want_records ? a.all.data() : nullptr;
    std::vector<Worker> wk((size_t)agx_host_threads());
    agx_parallel_for(n_pairs, 8192, [&](int64_t lo, int64_t hi, int tid) {
        Worker &me = wk[(size_t)tid];
        me.present.assign((size_t)hard_max_short + 1, 0);
        for (int64_t p = lo; p < hi; ++p) {
            PairPlan scratch;
            const uint32_t la = len[2 * p], lb = len[2 * p + 1];
            init_pair_plan(allp ? allp[(size_t)p] : scratch, p, la, lb, align);
            me.cells += (int64_t)la * lb;
            me.sum_len += (uint64_t)la + lb;
            if (la) {
                me.lo = std::min(me.lo, off[2 * p]);
                me.hi = std::max(me.hi, off[2 * p] + la);
            }
            if (lb) {
                me.lo = std::min(me.lo, off[2 * p + 1]);
                me.hi = std::max(me.hi, off[2 * p + 1] + lb);
            }
            if (la == 0 || lb == 0) continue; // no interior cell: score stays 0
            const bool second_short = !align && lb < la;
            const uint32_t lx = second_short ? lb : la, ly = second_short ? la : lb;
            if (lx > hard_max_short || ly > 0xffffu) {
                if (me.bad_pair < 0) me.bad_pair = p;
                continue;
            }
            me.longest_short = std::max(me.longest_short, lx);
            me.longest_long = std::max(me.longest_long, ly);
            me.present[lx] = 1;
            const uint32_t key = lx << 16 | ly;
            if (me.shape0 == 0xffffffffu) me.shape0 = key;
            else if (key != me.shape0) me.mixed = true;
            ++me.n_fill;
        }
    });
    for (const Worker &w : wk) {
        a.cells += w.cells;
        a.longest_short = std::max(a.longest_short, w.longest_short);
        a.longest_long = std::max(a.longest_long, w.longest_long);
        a.ext_lo = std::min(a.ext_lo, w.lo);
        a.ext_hi = std::max(a.ext_hi, w.hi);
        a.sum_len += w.sum_len;
    }
    for (const Worker &w : wk)
        if (w.bad_pair >= 0) {
            const int64_t p = w.bad_pair;
            agx_set_error("pair %lld: lengths %u x %u exceed the supported %u x 65535 (%s)", (long long)p,
                          len[2 * p], len[2 * p + 1], hard_max_short, align ? "query x target of an align batch" : "shorter x longer");
            return AGX_E_LIMIT;
        }
    if (a.ext_hi < a.ext_lo) a.ext_lo = a.ext_hi = 0; // no byte at all
    a.present.assign((size_t)a.longest_short + 1, 0);
    for (const Worker &w : wk)
        for (size_t lx = 0; lx < a.present.size() && lx < w.present.size(); ++lx) a.present[lx] |= w.present[lx];
    // one shape in the whole batch?
    for (const Worker &w : wk) {
        a.n_fill += w.n_fill;
        if (w.mixed) a.one_shape = false;
        if (w.shape0 != 0xffffffffu) {
            if (a.shape == 0xffffffffu) a.shape = w.shape0;
            else if (a.shape != w.shape0) a.one_shape = false;
        }
    }
    return AGX_OK;
}

// ---- kernel family.  The packed int16 kernels cover shorter sides up to 64 x 40 columns; one longer
// pair moves the whole batch to the int32 kernel, which also has the wide classes (up to 64 x 160).
// Biased formulation: every stored half must be the pattern of a positive normal half-precision number,
// [0x0400, 0x7c00): smallest B - max(|gf| + |ge|, delta), largest B + (longest shorter side + 1) * match + |gf|.
// (tests/test_sw_range_cpu.py reads from the trace that a batch one symbol beyond an edge of these rules changes its kernel)
KernelChoice choose_kernel(int want, const SwConstants &k, uint32_t longest_short, uint32_t longest_long, const BatchKind &kind)
{
    const SwParams &prm = k.prm;
    const bool matrix = kind.matrix != nullptr;
    int family = want == AGX_SW_KERNEL_INT32 ? 0 : want == AGX_SW_KERNEL_PACKED_SIGNED ? 1 : 2;
    if (matrix || longest_short > (uint32_t)kSwPackedMaxShort) family = 0; // the matrix lookup exists in the int32 kernel only
    // The int32 kernel asked for (BASELINE config 2 as worded) runs the packed plan and its DNA-coded image in 32-bit state,
    // one pair of a lane group at a time (agx_sw_i32d_kernel.hip: 7.5 instead of 8.5 instructions per cell), wherever the
    // coded match exists: delta and mismatch + |gf| must be bytes, the shorter sides within the packed plan's 2560 columns.
    if (family == 0 && !matrix && longest_short <= (uint32_t)kSwPackedMaxShort && prm.delta < 128 && prm.hd >= prm.delta && !agx_tune("AGX_SW_I32_CLASSIC")) family = 3;
    if (kind.align) family = kind.mode ? 5 : 4; // the locating / anchored fill: int32 state on the byte image, one pair per lane group
    if (family == 2 && !((int64_t)k.bias + ((int64_t)longest_short + 1) * k.sc.match - prm.gf < 0x7c00)) family = 1;
    // ... and its rising-offset variant adds (steps + 2) |ge| on top, steps <= longest longer side + 63
    int rising = family == 2 &&
                 (int64_t)k.bias + ((int64_t)longest_short + 1) * k.sc.match - prm.gf + ((int64_t)longest_long + 66 + 3) * -(int64_t)prm.ge < 0x7c00;
    // ... with column classes when the wrapping column's diagonal constant, mismatch + |gf| - 3 |ge|, is not negative
    if (rising && prm.hd - prm.delta + 3 * prm.ge >= 0) rising = 4;
    if (const char *e = agx_tune("AGX_SW_RISE")) rising = e[0] == '0' ? 0 : e[0] == '1' && rising ? 1 : rising;
    KernelChoice kc;
    kc.family = family;
    kc.rising = rising;
    kc.packed = family >= 1 && family <= 3;
    kc.coded_plan = family == 2 || family == 3;
    kc.costs = kind.stats == 2 ? kSwStatsClassCost : kind.cigar == 2 ? kSwTraceClassCost : class_costs(family); // (the stats and traced builds: fewer classes)
    kc.slots = kc.packed ? 2 : 1;
    return kc;
}

// What is chosen once the plan is known.
// ---- class period of the column classes (rising == 4; agx_sw_pk2w_kernel.hip).  With period P column j of
// a lane carries (j mod P) |ge| where it carried at most 3 |ge|; P = the largest period among the classes this batch
// launches.  Every constant of the cell goes in as ONE 32-bit add of k * 0x10001, k of either sign, which is exact in both
// halves whenever both results lie in [0, 0x10000): what has to hold is that every half the cell produces is a pattern
// of [0x0400, 0x7c00).  From below that holds as before: each result is a true value >= B - max(|gf|, -mismatch) plus an
// offset that is never negative -- the wrap column's and the first column's diagonal sums land on class 0's offset
// (t + 1) |ge|, and so do f - P |ge| at the wrap and max(zl, fl) - c_end on arrival.  From above, with steps <= ll + 63:
//   the diagonal sum, at most (steps + P - 1) |ge| of offset:            B + (ls + 1) match + (ll + 62 + P) |ge|
//   z and the horizontal gap ahead of its wrap, (steps + P) |ge|:        B + ls match - |gf| + (ll + 63 + P) |ge|
//   the running maxima, (steps + P + 4) |ge| after their last rise:      B + ls match - |gf| + (ll + 67 + P) |ge|
// all of which B + (ls + 1) match + |gf| + (ll + 65 + P) |ge| bounds (|gf| >= |ge|): the rising cell's own rule with P for 4.
// ---- staged wave priority of the biased packed fill (agx_sw_pk2_kernel.inc, "Staged priority"): only for a batch whose
// waves are ALL resident at once -- two on each of a CU's four SIMDs, the kernels' allocation (at most 256 VGPRs).  A batch
// that back-fills covers the tails of its waves with new ones, and there a wave near its end must not lose to a fresh one.
struct PeriodAndStage {
    int period = 4;    // the largest period among the launched classes (family 2 with column classes only)
    bool wide = false; // ... and whether the batch runs it
    int64_t resident = 0;
    int stage = 0;
};
PeriodAndStage choose_period_and_stage(const KernelChoice &kc, uint32_t launched_classes, size_t n_waves_total, int n_cu, const SwConstants &k,
                                       uint32_t longest_short, uint32_t longest_long)
{
    PeriodAndStage ps;
    if (kc.family != 2) return ps;
    if (kc.rising == 4) {
        for (int c = 0; c < kSwNumClasses; ++c)
            if ((launched_classes >> c & 1u) && kSwClasses[c] <= kSwPackedMaxShort / 64) ps.period = std::max(ps.period, sw_pk2_period(kSwClasses[c]));
        ps.wide = ps.period > 4 && (int64_t)k.bias + ((int64_t)longest_short + 1) * k.sc.match - k.prm.gf +
                                               ((int64_t)longest_long + 65 + ps.period) * -(int64_t)k.prm.ge < 0x7c00;
        if (const char *e = agx_tune("AGX_SW_PERIOD")) ps.wide = ps.wide && !(e[0] == '4' && !e[1]); // "4": the narrow kernel, for A/B
    }
    ps.resident = 8 * (int64_t)n_cu; // (n_cu: 0 without a device)
    bool stage = kc.rising == 4 && n_waves_total > 0 && (int64_t)n_waves_total <= ps.resident; // (the kernels with column classes have the build)
    if (const char *e = agx_tune("AGX_SW_STAGE")) stage = stage && !(e[0] == '0' && !e[1]); // "0": no staging, for A/B
    ps.stage = stage ? 1 : 0;
    return ps;
}

// plan-only batches check the symbols on the host; with a device the pack kernel does it
int check_symbols_host(const agx_sw_matrix *matrix, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs)
{
    std::vector<int64_t> bad((size_t)agx_host_threads(), -1);
    agx_parallel_for(n_pairs, 4096, [&](int64_t lo, int64_t hi, int tid) {
        for (int64_t p = lo; p < hi && bad[(size_t)tid] < 0; ++p) {
            const uint32_t la = len[2 * p], lb = len[2 * p + 1];
            if (la == 0 || lb == 0) continue;
            const uint8_t *q = bases + off[2 * p], *r = bases + off[2 * p + 1];
            bool hit = false;
            if (matrix) {
                for (uint32_t k = 0; k < la; ++k) hit |= matrix->code[q[k]] == 0xff;
                for (uint32_t k = 0; k < lb; ++k) hit |= matrix->code[r[k]] == 0xff;
            } else
                hit = memchr(q, 0, la) || memchr(r, 0, lb);
            if (hit) bad[(size_t)tid] = p;
        }
    });
    int64_t first_bad = -1;
    for (int64_t v : bad)
        if (v >= 0 && (first_bad < 0 || v < first_bad)) first_bad = v;
    if (first_bad < 0) return AGX_OK;
    set_symbol_error(matrix != nullptr, first_bad);
    return AGX_E_SYMBOL;
}

// the batch object, with everything a create knows before the plan; with a device, the code objects it will launch from are
// loaded now rather than inside its first launch
agx_sw_batch *new_batch(agx_ctx *ctx, int64_t n_pairs, const KernelChoice &kc, const SwConstants &k, const BatchKind &kind)
{
    agx_sw_batch *b = new agx_sw_batch();
    agx_ctx_retain(ctx);
    b->ctx = ctx;
    b->n_pairs = n_pairs;
    b->family = kc.family;
    b->rising = kc.rising;
    const bool matrix = kind.matrix != nullptr;
    const int family = kc.family, stats = kind.stats, cigar = kind.cigar;
    if (ctx) {
        agx_sw_pack_preload();
        agx_copy_preload();
        if (family == 2) agx_sw_pk2_preload();
        if (family == 3) agx_sw_i32d_preload();
        if (family == 0 && !matrix) agx_sw_i32_preload();
        if (family == 4 && stats != 2) (matrix ? agx_sw_loc_mat_preload : agx_sw_loc_preload)();
        if (family == 5 && stats != 2 && cigar != 2) (matrix ? agx_sw_anch_mat_preload : agx_sw_anch_preload)();
        if (cigar == 2) {
            (matrix ? agx_sw_trace_mat_preload : agx_sw_trace_preload)();
            agx_sw_walk_preload();
        }
        if (family == 4 && stats == 2) (matrix ? agx_sw_loc_mat_stats_preload : agx_sw_loc_stats_preload)();
        if (family == 5 && stats == 2) (matrix ? agx_sw_anch_mat_stats_preload : agx_sw_anch_stats_preload)();
    }
    b->matrix = matrix;
    if (matrix) b->mat = *kind.matrix;
    b->align = kind.align;
    b->mode = kind.mode;
    b->stats = stats;
    b->cigar = cigar;
    b->scoring = k.sc;
    b->prm = k.prm;
    b->prm.n_out = (uint32_t)n_pairs + 1u;
    return b;
}

// ---- device planner: the candidate's verdict.  Pass A2 (threads over pairs) tiles every pair by lookup in the
// full table and only COUNTS: pairs per (class, G) bucket -- from which every group, wave and record offset
// follows without a scan -- image words, estimated waves, the votes of the sampled dominant shape; it also
// copies len[] into page-locked memory for its upload.  The rules that need another tiling (tail regime,
// class consolidation, dominant shape) send the batch to the host planner.  dp: the length copy, the histogram, the image size.
int device_plan_verdict(agx_ctx *ctx, const uint32_t *len, int64_t n_pairs, int slots, bool trace, DevPlan &dp, bool *device_plan)
{
    const int n_cu = ctx->n_cu;
    const TilingTable &tt = full_tiling_table(2);
    const int rc = dp.h_len.alloc(ctx, (size_t)n_pairs * 2 * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t cand = 0;
    const int votes = sampled_majority_shape((size_t)n_pairs, std::max<size_t>(1, (size_t)n_pairs / 512), [&](size_t p, uint32_t *sh) {
        const uint32_t la = len[2 * p], lb = len[2 * p + 1];
        *sh = std::min(la, lb) << 16 | (std::max(la, lb) & 0xffffu);
        return la != 0 && lb != 0;
    }, &cand);
    struct Count {
        std::vector<uint32_t> hist;
        uint64_t words = 0;
        double waves = 0;
        int64_t votes = 0;
        bool untiled = false;
    };
    std::vector<Count> cnt((size_t)agx_host_threads());
    uint32_t *pinned_len = (uint32_t *)dp.h_len.p;
    agx_parallel_for(n_pairs, 8192, [&](int64_t lo, int64_t hi, int tid) {
        Count &me = cnt[(size_t)tid];
        me.hist.assign((size_t)kSwPlanBuckets, 0);
        memcpy(pinned_len + 2 * lo, len + 2 * lo, (size_t)(hi - lo) * 2 * sizeof(uint32_t));
        for (int64_t p = lo; p < hi; ++p) {
            const uint32_t la = len[2 * p], lb = len[2 * p + 1];
            if (la == 0 || lb == 0) continue;
            const uint32_t lx = std::min(la, lb), ly = std::max(la, lb);
            Tiling tl;
            if (!tt.pick(lx, ly, &tl, nullptr)) {
                me.untiled = true;
                continue;
            }
            ++me.hist[(size_t)tl.cls * 64 + (size_t)(64 - tl.G)];
            me.words += ((uint64_t)tl.G * kSwClasses[tl.cls] + 3) / 4 + 1 + ((uint64_t)ly + 3) / 4;
            me.waves += (double)tl.G / 64.0 / slots;
            me.votes += (lx << 16 | (ly & 0xffffu)) == cand;
        }
    });
    dp.hist.assign((size_t)kSwPlanBuckets, 0);
    uint64_t words = 0;
    double waves_est = 0;
    int64_t cand_count = 0;
    bool untiled = false;
    for (const Count &c : cnt) {
        if (c.hist.empty()) continue;
        for (int k = 0; k < kSwPlanBuckets; ++k) dp.hist[(size_t)k] += c.hist[(size_t)k];
        words += c.words;
        waves_est += c.waves;
        cand_count += c.votes;
        untiled |= c.untiled;
    }
    const double fill = waves_est / (5.0 * 4.0 * n_cu);
    dp.img_dw = (size_t)kSwPackedMaxShort / 4 + 1 + words;
    *device_plan = !untiled && fill >= 0.48 && waves_est >= 2048.0 && !(votes > 0 && cand_count * 2 >= n_pairs) && dp.img_dw <= 0xffffffffull;
    if (trace)
        fprintf(stderr, "[agx_sw_batch_create] device planner verdict %d: untiled %d, waves %.0f (fill %.2f), sampled shape votes %d -> %lld of %lld pairs, image %zu words\n",
                (int)*device_plan, (int)untiled, waves_est, fill, votes, (long long)cand_count, (long long)n_pairs, dp.img_dw);
    return AGX_OK;
}

// a candidate the verdict sent back: the host planner's per-pair records, as pass A would have written them
void records_after_all(const uint32_t *len, int64_t n_pairs, std::vector<PairPlan> &all)
{
    all.resize((size_t)n_pairs);
    PairPlan *allp = all.data();
    agx_parallel_for(n_pairs, 8192, [&](int64_t lo, int64_t hi, int) {
        for (int64_t p = lo; p < hi; ++p) init_pair_plan(allp[(size_t)p], p, len[2 * p], len[2 * p + 1], 0);
    });
}

// ---- a device-made plan: the buckets' extents from their counts, then everything per pair on the device, on the planning
// stream, beside the upload of the sequences
int plan_on_device(agx_ctx *ctx, SwPending &tmp, agx_sw_batch *b, int64_t n_pairs, uint32_t longest_long, int slots, size_t img0, PlanLayout &lay)
{
    DevPlan &dp = tmp.dp;
    int rc;
    {
        static std::mutex once_per_context;
        std::lock_guard<std::mutex> l(once_per_context);
        rc = agx_ctx_prepare_plan(ctx);
    }
    if (!rc) rc = dp.h_buckets.alloc(ctx, (size_t)kSwPlanBuckets * 5 * sizeof(uint32_t));
    if (rc) return rc;
    size_t entries = 0;
    lay = layout_from_buckets(dp.hist, slots, (uint32_t *)dp.h_buckets.p, &entries);
    lay.img_dw = dp.img_dw;
    rc = launch_device_plan(ctx, dp, b, (uint32_t)n_pairs, (uint32_t)entries, longest_long, slots, (uint32_t)img0, lay.n_groups, lay.n_waves_total);
    if (!rc) rc = tmp.h_flag.alloc(ctx, 2 * sizeof(uint32_t));
    return rc;
}

// ---- the records of a host-made plan, written straight into pinned staging when there is a device (groups_host: plan-only,
// no pinned memory without a device).  *groups_data: where the group records are
int write_records(agx_ctx *ctx, SwPending &tmp, const PlanLayout &lay, const std::vector<PairPlan> &plan, const KernelChoice &kc, int64_t n_pairs,
                  agx_sw_batch *b, std::vector<uint8_t> &groups_host, void **groups_data)
{
    if (ctx) {
        int rc = tmp.h_groups.alloc(ctx, lay.groups_bytes);
        if (!rc) rc = tmp.h_waves.alloc(ctx, lay.waves_bytes);
        if (!rc) rc = tmp.h_flag.alloc(ctx, 2 * sizeof(uint32_t));
        if (rc) return rc;
        *groups_data = tmp.h_groups.p;
        if (lay.waves_bytes) memcpy(tmp.h_waves.p, lay.waves.data(), lay.waves_bytes);
    } else {
        groups_host.resize(lay.groups_bytes);
        *groups_data = groups_host.data();
    }
    write_group_records(lay, plan, kc, n_pairs, *groups_data);
    if (b->cigar == 2) write_trace_records(lay, plan, n_pairs, b);
    return AGX_OK;
}

// ---- device image: records up, image built and checked by the pack kernel, all on the copy stream -- or, for a
// device-planned batch, on the PLANNING stream, behind its records, once its sequences have arrived (an event on the copy
// stream): the copy stream then carries nothing but uploads, and the next piece of a one-shot call (agx_sw_score: two
// creator threads) uploads right behind this one instead of behind this one's pack kernel.  *tail: the stream to wait for
int queue_device_image(agx_ctx *ctx, agx_sw_batch *b, SwPending &tmp, const PlanLayout &lay, const KernelChoice &kc, const SwConstants &k,
                       const BatchKind &kind, hipStream_t *tail)
{
    const bool device_plan = tmp.device_plan, matrix = kind.matrix != nullptr;
    const int align = kind.align, stats = kind.stats, cigar = kind.cigar;
    const size_t n_pairs = (size_t)b->n_pairs;
    Uploader &up = tmp.up;
    int rc = b->img.alloc(ctx, std::max<size_t>(lay.img_dw, 4) * 4);
    if (!rc && !device_plan) rc = b->groups.alloc(ctx, lay.groups_bytes); // (the device planner has written its own already)
    if (!rc && !device_plan) rc = b->waves.alloc(ctx, lay.waves_bytes);
    if (!rc && matrix) rc = b->table.alloc(ctx, k.table.size() * sizeof(int16_t));
    if (!rc) rc = b->scores.alloc(ctx, (n_pairs + 1) * sizeof(int32_t)); // +1: spare slot of vacant packed halves
    if (!rc) rc = b->out_stage.alloc(ctx, (n_pairs + 1) * sizeof(int32_t));
    if (!rc && align) rc = b->ends.alloc(ctx, (n_pairs + 1) * sizeof(uint32_t));
    if (!rc && align) rc = b->ends_stage.alloc(ctx, (n_pairs + 1) * sizeof(uint32_t));
    if (!rc && stats == 2) rc = b->lstat.alloc(ctx, (n_pairs + 1) * sizeof(uint32_t));
    if (!rc && stats == 2) rc = b->lstat_stage.alloc(ctx, (n_pairs + 1) * sizeof(uint32_t));
    if (!rc && cigar == 2) rc = b->goff.alloc(ctx, std::max<size_t>(b->tr_goff.size(), 1) * sizeof(uint64_t));
    if (!rc && cigar == 2) rc = b->walkrec.alloc(ctx, std::max<size_t>(b->tr_walk.size(), 1) * sizeof(SwWalkRec));
    if (!rc && lay.launches.size() > 1) rc = agx_ctx_prepare_fanout(ctx);
    if (rc) return rc;
    hipStream_t cs = ctx->copy;
    hipError_t e = hipSuccess;
    hipStream_t ts = device_plan ? ctx->plan : cs;
    *tail = ts;
    if (device_plan) {
        e = hipEventRecord(tmp.dp.uploaded, cs); // the uploader has queued everything (joined by now)
        if (e == hipSuccess) e = hipStreamWaitEvent(ts, tmp.dp.uploaded, 0);
    }
    if (e == hipSuccess && !device_plan && lay.groups_bytes) e = hipMemcpyAsync(b->groups.p, tmp.h_groups.p, lay.groups_bytes, hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && !device_plan && lay.waves_bytes) e = hipMemcpyAsync(b->waves.p, tmp.h_waves.p, lay.waves_bytes, hipMemcpyHostToDevice, cs);
    if (e == hipSuccess && matrix)
        e = hipMemcpyAsync(b->table.p, k.table.data(), k.table.size() * sizeof(int16_t), hipMemcpyHostToDevice, ts);
    if (e == hipSuccess && cigar == 2 && !b->tr_goff.empty())
        e = hipMemcpyAsync(b->goff.p, b->tr_goff.data(), b->tr_goff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ts);
    if (e == hipSuccess && cigar == 2 && !b->tr_walk.empty())
        e = hipMemcpyAsync(b->walkrec.p, b->tr_walk.data(), b->tr_walk.size() * sizeof(SwWalkRec), hipMemcpyHostToDevice, ts);
    // pairs with an empty side are never touched by a kernel: their score is this zero
    if (e == hipSuccess) e = hipMemsetAsync(b->scores.p, 0, b->scores.bytes, ts);
    if (e == hipSuccess && align) e = hipMemsetAsync(b->ends.p, 0xff, b->ends.bytes, ts); // ... and their end cell is "none"
    if (e == hipSuccess && stats == 2) e = hipMemsetAsync(b->lstat.p, 0, b->lstat.bytes, ts); // ... and they paired nothing
    if (e == hipSuccess && kc.packed) e = hipMemsetAsync(b->img.p, 0, (size_t)kSwPackedMaxShort + 4, ts);
    uint32_t *flag = (uint32_t *)tmp.h_flag.p;
    flag[0] = 0;
    flag[1] = 0xffffffffu;
    if (e == hipSuccess && lay.n_groups) {
        const char *dna_knob = agx_tune("AGX_SW_DNA");
        // the DNA-coded cell adds (mismatch + |gf|) and a table byte: both must be non-negative bytes
        const bool dna = kc.coded_plan && k.prm.delta < 128 && k.prm.hd >= k.prm.delta && !(dna_knob && dna_knob[0] == '0');
        const int n_cu = ctx->n_cu;
        const int pr = dna // the biased packed fill has a DNA-coded cell: its pack kernel decides per wavefront
                           ? agx_sw_pack_dna_launch((const uint8_t *)up.d_raw.p + kRawPad, (const uint64_t *)up.d_off.p, up.raw_base, b->groups.p, b->waves.p,
                                                    (uint32_t)lay.n_waves_total, (uint32_t)n_pairs, (uint32_t *)b->img.p, (uint32_t *)up.d_flag.p,
                                                    n_cu, ts)
                           : agx_sw_pack_launch(matrix, kc.slots, (const uint8_t *)up.d_raw.p + kRawPad, (const uint64_t *)up.d_off.p, up.raw_base,
                                                b->groups.p, (uint32_t)lay.n_groups, (uint32_t)n_pairs, (uint32_t *)b->img.p,
                                                (const uint8_t *)up.d_code.p, (uint32_t *)up.d_flag.p, n_cu, ts);
        if (pr) {
            agx_set_error("sw_pack launch failed: %s", hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
        e = hipMemcpyAsync(flag, up.d_flag.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ts);
    }
    if (e != hipSuccess) {
        agx_set_error("agx_sw_batch_create: upload -> %s", hipGetErrorString(e));
        return AGX_E_HIP;
    }
    return AGX_OK;
}

// AGX_TRACE_CREATE: what was chosen once the plan was known, and the plan's digest (tests parse these lines)
// A device-made plan's records never reach the host otherwise: the trace waits for the planning kernels (dp.done) and copies the
// wave and group records back, before the pack kernel marks the waves, and hashes them as it does a host-made plan's.
int trace_plan(const agx_sw_batch *b, const KernelChoice &kc, const PeriodAndStage &ps, const PlanLayout &lay, const DevPlan *dp, const void *groups_data)
{
    if (kc.family == 2 && kc.rising == 4) fprintf(stderr, "[agx_sw_batch_create] class period %d of %d\n", ps.wide ? ps.period : 4, ps.period);
    if (kc.family == 2)
        fprintf(stderr, "[agx_sw_batch_create] staged priority %d: %lld waves, %lld resident at once\n", ps.stage, (long long)lay.n_waves_total,
                (long long)ps.resident);
    if (!dp) {
        fprintf(stderr, "[agx_sw_batch_create] plan digest %016llx\n", (unsigned long long)plan_digest(b, lay.waves, groups_data, lay.groups_bytes));
        trace_plan_parts(b, kc.packed, lay.waves, groups_data, lay.groups_bytes);
        return AGX_OK;
    }
    fprintf(stderr, "[agx_sw_batch_create] plan digest: on device\n");
    std::vector<SwWave> waves(lay.n_waves_total);
    std::vector<SwGroup2> groups(lay.n_groups);
    const size_t groups_bytes = lay.n_groups * sizeof(SwGroup2);
    AGX_HIP(hipEventSynchronize(dp->done));
    if (!waves.empty()) AGX_HIP(hipMemcpy(waves.data(), b->waves.p, waves.size() * sizeof(SwWave), hipMemcpyDeviceToHost));
    if (!groups.empty()) AGX_HIP(hipMemcpy(groups.data(), b->groups.p, groups_bytes, hipMemcpyDeviceToHost));
    fprintf(stderr, "[agx_sw_batch_create] device plan digest %016llx\n", (unsigned long long)plan_digest(b, waves, groups.data(), groups_bytes));
    trace_plan_parts(b, true, waves, groups.data(), groups_bytes);
    return AGX_OK;
}

// what agx_sw_batch_info answers (a device-made plan's padded cells arrive with the verdict)
void set_info(agx_sw_batch *b, int64_t cells, const PlanLayout &lay, bool device_plan)
{
    b->info.n_pairs = b->n_pairs;
    b->info.cells = cells;
    b->info.padded_cells = lay.padded;
    b->info.input_bytes = (int64_t)(lay.img_dw * 4 + lay.groups_bytes + lay.waves_bytes);
    b->info.n_launches = (int32_t)lay.launches.size();
    b->info.n_waves = (int32_t)lay.n_waves_total;
    b->info.planned_on_device = device_plan ? 1 : 0;
}

// the stage timestamps of the AGX_TRACE_CREATE line (ms), which the driver takes between its stages
struct CreateTimes {
    double begin = 0, pass_a = 0, plan = 0, sort = 0, waves = 0, records = 0, joined = 0;
};
void trace_times(const CreateTimes &t, int64_t n_pairs, bool with_device, bool device_plan, uint64_t raw_bytes)
{
    if (!with_device) {
        fprintf(stderr, "[agx_sw_batch_create, plan only] %lld pairs: pass A %.2f ms | tiling %.2f, sort %.2f, waves %.2f, records %.2f\n",
                (long long)n_pairs, t.pass_a - t.begin, t.plan - t.pass_a, t.sort - t.plan, t.waves - t.sort, t.records - t.waves);
        return;
    }
    fprintf(stderr,
            "[agx_sw_batch_create] %lld pairs%s: pass A %.2f ms | tiling %.2f, sort %.2f, waves %.2f, records %.2f | waited %.2f ms more "
            "for the upload of %.1f MB | device pack + sync %.2f ms\n",
            (long long)n_pairs, device_plan ? " (planned on the device)" : "", t.pass_a - t.begin, t.plan - t.pass_a, t.sort - t.plan, t.waves - t.sort,
            t.records - t.waves, t.joined - t.records, raw_bytes / 1e6, agx_now_ms() - t.joined);
}

} // namespace

namespace agx_sw_host {

int matrix_constants(const agx_sw_matrix *matrix, agx_sw_scoring &sc, SwParams &prm, std::vector<int16_t> &table)
{
    SwConstants k;
    const int rc = make_constants(nullptr, matrix, k);
    if (rc) return rc;
    sc = k.sc;
    prm = k.prm;
    table.swap(k.table);
    return AGX_OK;
}

// The create of every Smith-Waterman batch that is not banded: the stages above and agx_sw_plan.cpp's, top to bottom.
int create_batch(agx_ctx *ctx, const agx_sw_scoring *scoring, const agx_sw_matrix *matrix, const uint8_t *bases,
                 const uint64_t *off, const uint32_t *len, int64_t n_pairs, agx_sw_batch **out, bool defer, int align, int mode, int stats,
                 int cigar)
{
    if (!out) {
        agx_set_error("agx_sw_batch_create: out is NULL");
        return AGX_E_ARG;
    }
    *out = nullptr;
    // ctx == NULL: plan only (no device needed) -- the batch answers agx_sw_batch_info() and nothing else
    int rc = ctx ? agx_bind(ctx) : AGX_OK;
    if (rc) return rc;
    const int n_cu = ctx ? ctx->n_cu : 256;
    if ((rc = check_arrays(off, len, n_pairs))) return rc;
    const BatchKind kind{matrix, align, mode, stats, cigar};
    SwConstants k;
    if ((rc = make_constants(scoring, matrix, k))) return rc;

    const bool trace = agx_tune("AGX_TRACE_CREATE") != nullptr;
    CreateTimes t;
    t.begin = agx_now_ms();
    if ((rc = check_bases(bases, len, n_pairs))) return rc;
    const int want = tuned_kernel() ? tuned_kernel() : ctx ? ctx->opt_sw_kernel : AGX_SW_KERNEL_AUTO;
    const bool dev_candidate = device_plan_candidate(ctx, kind, n_pairs, want);
    PassA a;
    if ((rc = pass_a(off, len, n_pairs, align, longest_short_allowed(kind), !dev_candidate, a))) return rc;
    t.pass_a = agx_now_ms();

    const KernelChoice kc = choose_kernel(want, k, a.longest_short, a.longest_long, kind);
    if (trace)
        fprintf(stderr, "[agx_sw_batch_create] family %d rising %d: longest shorter side %u, longest longer side %u\n", kc.family, kc.rising,
                a.longest_short, a.longest_long);
    if (!ctx && n_pairs > 0 && (rc = check_symbols_host(matrix, bases, off, len, n_pairs))) return rc;

    // Every exit from here: the uploader's thread joined (it uses what tmp owns), then on an error the streams drained, before
    // the batch and tmp give their blocks back -- `done` is declared after both and so leaves first.
    std::unique_ptr<SwPending> tmp(new SwPending()); // released when this function leaves, or kept by the batch (defer)
    tmp->matrix = matrix != nullptr;
    agx_sw_batch *b = new_batch(ctx, n_pairs, kc, k, kind); // destroyed by `done` on an error exit
    DrainOnError done(ctx, [&] { agx_sw_batch_destroy(b); }, &tmp->up.thread);
    tmp->up.start(ctx, matrix, bases, off, len, n_pairs, a.ext_lo, a.ext_hi, a.sum_len);

    const bool uniform = a.one_shape && a.n_fill == n_pairs && n_pairs >= 1024 && n_cu > 0;
    bool device_plan = false;
    if (dev_candidate && kc.family == 2 && !uniform && n_cu > 0 && a.n_fill > 0 && a.longest_short <= (uint32_t)kSwPackedMaxShort) {
        if ((rc = device_plan_verdict(ctx, len, n_pairs, kc.slots, trace, tmp->dp, &device_plan))) return rc;
    } else if (trace)
        fprintf(stderr, "[agx_sw_batch_create] no device planner: candidate %d, family %d, uniform %d, n_fill %lld, longest shorter side %u\n",
                (int)dev_candidate, kc.family, (int)uniform, (long long)a.n_fill, a.longest_short);
    tmp->device_plan = device_plan;
    if (dev_candidate && !device_plan) { // the host planner after all
        records_after_all(len, n_pairs, a.all);
        tmp->dp.h_len.release();
    }

    // ---- the plan: file order for a uniform batch, else passes B and C on the host -- or everything per pair on the device
    std::vector<PairPlan> plan;
    const bool planned = uniform && plan_uniform(a.all, a.shape, n_cu, kc, matrix != nullptr, plan);
    if (planned) b->file_order = true;
    t.plan = t.sort = agx_now_ms();
    if (!planned && !device_plan) {
        if ((rc = plan_host(a.all, a.present, a.longest_long, n_cu, kc, matrix != nullptr, plan, &t.plan))) return rc;
        t.sort = agx_now_ms();
    }
    t.waves = t.records = t.sort;

    // ---- pass D and the records
    const size_t img0 = kc.packed ? (size_t)kSwPackedMaxShort / 4 + 1 : 0; // the zero block vacant slots point at
    PlanLayout lay;
    std::vector<uint8_t> groups_host;
    void *groups_data = nullptr;
    if (device_plan) {
        if ((rc = plan_on_device(ctx, *tmp, b, n_pairs, a.longest_long, kc.slots, img0, lay))) return rc;
        t.waves = t.records = agx_now_ms();
    } else {
        if ((rc = layout_from_plan(plan, kc, img0, lay))) return rc;
        t.waves = agx_now_ms();
        if ((rc = write_records(ctx, *tmp, lay, plan, kc, n_pairs, b, groups_host, &groups_data))) return rc;
        t.records = agx_now_ms();
    }
    b->launches = lay.launches;
    const PeriodAndStage ps = choose_period_and_stage(kc, lay.launched_classes, lay.n_waves_total, ctx ? ctx->n_cu : 0, k, a.longest_short, a.longest_long);
    b->wide = ps.wide;
    b->stage = ps.stage;
    if (ps.wide && ctx) agx_sw_pk2w_preload();
    if (trace && (rc = trace_plan(b, kc, ps, lay, device_plan ? &tmp->dp : nullptr, groups_data))) return rc;
    set_info(b, a.cells, lay, device_plan);
    if (!ctx) { // planning only
        if (trace) trace_times(t, n_pairs, false, false, 0);
        *out = b;
        b = nullptr;
        done.ok = true;
        return AGX_OK;
    }

    // ---- the device image, and the two exits
    if ((rc = tmp->up.join())) return rc;
    t.joined = agx_now_ms();
    hipStream_t ts = nullptr;
    if ((rc = queue_device_image(ctx, b, *tmp, lay, kc, k, kind, &ts))) return rc;
    if (defer) { // the caller finishes later (finish_create): everything stays queued
        hipError_t e = hipEventCreateWithFlags(&tmp->ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(tmp->ready, ts);
        if (e != hipSuccess) {
            agx_set_error("agx_sw_batch_create: upload -> %s", hipGetErrorString(e));
            return AGX_E_HIP;
        }
        tmp->tail = ts;
        b->pending = tmp.release();
        *out = b;
        b = nullptr;
        done.ok = true; // finish_create waits for tail
        return AGX_OK;
    }
    if ((rc = wait_for_verdict(b, *tmp, ts))) return rc; // blocking by contract; the staging buffers are free again
    if ((rc = ensure_done_event(b))) return rc;
    if (trace) fprintf(stderr, "[agx_sw_batch_create] done event %d\n", b->done ? 1 : 0);
    if (trace) trace_times(t, n_pairs, true, device_plan, tmp->up.raw_bytes);
    *out = b;
    b = nullptr;
    done.ok = true; // ts synchronised above, and it covers the copy stream
    return AGX_OK;
}

} // namespace agx_sw_host

namespace {

// ---- Completion on the dispatch.  A launch carries no completion signal of its own, so a stream wait makes the runtime queue a
// marker packet with a signal behind the fill, and the command processor must take that packet, after the last wave has retired,
// before the host's poll sees anything.  A batch of the biased packed fill with ONE launch therefore owns an event, and its launch
// -- while the batch is bound: nothing else waits for the event -- hands it to the runtime as the kernel's stop event (hipExtLaunchKernelGGL): the fill's own packet then carries the signal.
// agx_sw_batch_scores waits for that event instead of the stream -- in its bound branch, where nothing else is queued behind
// the fill -- while the launch is still the last thing the library put on the stream (agx_ctx::enqueued), and for the stream
// otherwise.  The kind of wait is the runtime's in both cases.  profiles/sw_step_boundary.md: bench.py's config-2 step 156.2-156.9 -> 153.8-154.2 us.
int ensure_done_event(agx_sw_batch *b)
{
    const bool one_fill = b->ctx && b->family == 2 && !b->banded && !b->matrix && !b->align && b->launches.size() == 1;
    if (one_fill && done_event_on() && !b->done) AGX_HIP(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    return AGX_OK;
}

} // namespace

extern "C" {

int agx_sw_batch_launch(agx_sw_batch *b)
{
    if (!b) {
        agx_set_error("agx_sw_batch_launch: null batch");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it cannot be launched");
        return AGX_E_NODEVICE;
    }
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    b->rebound = false; // what this launch writes is what the next fetch reads
    if (b->banded) return band_launch(b);
    // a batch whose create was not finished: its fill waits for the pack kernel on the device, not on the host
    if (b->pending && b->pending->ready) AGX_HIP(hipStreamWaitEvent(agx_enqueue_stream(b->ctx), b->pending->ready, 0));
    SwParams prm = b->prm;
    if (b->bound) prm.n_out = (uint32_t)b->n_pairs; // the caller's array has no spare slot
    prm.stage = (uint32_t)b->stage;
    b->cig_valid = false; // what agx_sw_batch_cigars kept belongs to the launch before
    if (b->cigar == 2 && !b->trace_p && b->tr_dwords) {
        agx_set_error("agx_sw_batch_launch: a traced fill without its trace block");
        return AGX_E_INTERNAL;
    }
    FanOut fan(b->ctx, (int)b->launches.size());
    rc = fan.begin();
    if (rc) return rc;
    // (ensure_done_event: the biased packed fill only; only a fetch from the bound array waits for the event, so only a bound
    // batch's launch carries it -- every other launch is the plain one)
    hipEvent_t stop = b->bound && b->launches.size() == 1 ? b->done : nullptr;
    int k = 0;
    // widest class first: its waves have the longest rows-times-columns chain, so they should not be the tail
    for (auto it = b->launches.rbegin(); it != b->launches.rend(); ++it) {
        const ClassLaunch &cl = *it;
        hipStream_t st = fan.stream(k++);
        const uint32_t *img = (const uint32_t *)b->img.p;
        const SwWave *wv = (const SwWave *)b->waves.p + cl.first_wave;
        int32_t *scores = b->bound ? b->bound : (int32_t *)b->scores.p;
        const int anch_capture = b->mode != AGX_SW_MODE_EXTEND, anch_flags = b->mode == AGX_SW_MODE_FIT ? 1 : b->mode == AGX_SW_MODE_GLOBAL ? 2 : 0;
        int r;
        uint32_t *lstat = (uint32_t *)b->lstat.p;
        if (b->cigar == 2 && b->matrix)
            r = agx_sw_trace_mat_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p, b->trace_p,
                                              (const uint64_t *)b->goff.p, (const int16_t *)b->table.p, st);
        else if (b->cigar == 2)
            r = agx_sw_trace_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p, b->trace_p,
                                          (const uint64_t *)b->goff.p, st);
        else if (b->stats == 2 && b->family == 5 && b->matrix)
            r = agx_sw_anch_mat_stats_launch_class(cl.C, anch_capture, anch_flags, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores,
                                                   (uint32_t *)b->ends.p, lstat, (const int16_t *)b->table.p, st);
        else if (b->stats == 2 && b->family == 5)
            r = agx_sw_anch_stats_launch_class(cl.C, anch_capture, anch_flags, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores,
                                               (uint32_t *)b->ends.p, lstat, st);
        else if (b->stats == 2 && b->matrix)
            r = agx_sw_loc_mat_stats_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p, lstat,
                                                  (const int16_t *)b->table.p, st);
        else if (b->stats == 2)
            r = agx_sw_loc_stats_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p, lstat, st);
        else if (b->family == 5 && b->matrix)
            r = agx_sw_anch_mat_launch_class(cl.C, anch_capture, anch_flags, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores,
                                             (uint32_t *)b->ends.p, (const int16_t *)b->table.p, st);
        else if (b->family == 5)
            r = agx_sw_anch_launch_class(cl.C, anch_capture, anch_flags, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores,
                                         (uint32_t *)b->ends.p, st);
        else if (b->align && b->matrix)
            r = agx_sw_loc_mat_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p,
                                            (const int16_t *)b->table.p, st);
        else if (b->align)
            r = agx_sw_loc_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores, (uint32_t *)b->ends.p, st);
        else if (b->matrix)
            r = agx_sw_mat_launch_class(cl.C, prm, img, (const SwGroup *)b->groups.p, wv, cl.n_waves, scores,
                                        (const int16_t *)b->table.p, st);
        else if (b->family == 3)
            r = cl.C == 0 ? agx_sw_i32d_launch_any(prm, img, (const SwGroup2 *)b->groups.p, wv, cl.n_waves, scores, st)
                          : agx_sw_i32d_launch_class(cl.C, prm, img, (const SwGroup2 *)b->groups.p, wv, cl.n_waves, scores, st);
        else if (b->family == 2) {
            r = cl.C == 0 ? agx_sw_pk2_launch_any(b->rising, b->wide, prm, img, (const SwGroup2 *)b->groups.p, wv, cl.n_waves, scores, st, stop)
                          : agx_sw_pk2_launch_class(cl.C, b->rising, b->wide, prm, img, (const SwGroup2 *)b->groups.p, wv, cl.n_waves, scores, st, stop);
            // only these launchers take the event.  This launch is the stream's last, and its event will arrive:
            // agx_sw_batch_scores may wait for it alone
            if (!r && stop && cl.n_waves) b->done_at = b->ctx->enqueued;
        }
        else if (b->family == 1)
            r = agx_sw_pk_launch_class(cl.C, prm, img, (const SwGroup2 *)b->groups.p, wv, cl.n_waves, scores, st);
        else
            r = (cl.C > 40 ? agx_sw_wide_launch_class : agx_sw_launch_class)(cl.C, prm, img, (const SwGroup *)b->groups.p, wv,
                                                                             cl.n_waves, scores, st);
        if (r) {
            agx_set_error("sw_fill<%d> launch failed: %s", cl.C, hipGetErrorString(hipGetLastError()));
            return AGX_E_HIP;
        }
    }
    return fan.end();
}

int agx_sw_batch_scores(agx_sw_batch *b, int32_t *scores)
{
    if (!b || (!scores && b->n_pairs)) {
        agx_set_error("agx_sw_batch_scores: null argument");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device): it has no scores");
        return AGX_E_NODEVICE;
    }
    int rc = agx_bind(b->ctx);
    if (rc) return rc;
    if (b->banded) { // the mode's score is the hit's
        AGX_GUARD_BEGIN
        std::vector<agx_sw_hit> h((size_t)b->n_pairs);
        rc = b->band_at ? band_at_hits(b, h.data(), false) : band_hits(b, h.data());
        for (int64_t p = 0; !rc && p < b->n_pairs; ++p) scores[p] = h[(size_t)p].score;
        return rc;
        AGX_GUARD_END("agx_sw_batch_scores")
    }
    if (b->rebound) {
        agx_set_error("agx_sw_batch_scores: agx_sw_batch_bind_scores changed where this batch's scores go and no launch has run since; launch first");
        return AGX_E_ARG;
    }
    if (b->pending) { // (the pieces of agx_sw_score finish before they fetch; kept for safety)
        rc = finish_create(b);
        if (rc) return rc;
    }
    if (b->n_pairs == 0) {
        AGX_HIP(hipStreamSynchronize(b->ctx->stream));
        return AGX_OK;
    }
    const size_t bytes = (size_t)b->n_pairs * sizeof(int32_t);
    if (b->bound && scores == b->bound) { // the launches wrote them there themselves: nothing to copy
        // completion on the dispatch (ensure_done_event): while this batch's launch is the last thing the library put on the
        // stream, its own stop event says all a stream wait would -- and the runtime queues no marker behind the fill to learn it
        const bool own = b->done && b->done_at && b->done_at == b->ctx->enqueued;
        if (trace_fetch()) fprintf(stderr, "[agx_sw_batch_scores] wait: %s\n", own ? "event" : "stream");
        if (own)
            AGX_HIP(hipEventSynchronize(b->done));
        else
            AGX_HIP(hipStreamSynchronize(b->ctx->stream));
        return AGX_OK;
    }
    if (b->bound) { // bound elsewhere: the device array was not written by the last launch
        AGX_HIP(hipStreamSynchronize(b->ctx->stream));
        memcpy(scores, b->bound, bytes);
        return AGX_OK;
    }
    // one copy kernel right behind the last fill on the launch stream: straight into the caller's array when that is
    // page-locked (agx_host_alloc), else into pinned staging and a host copy from there
    int32_t *dst = agx_is_pinned_host(scores, bytes) ? scores : (int32_t *)b->out_stage.p;
    if (agx_copy_out_launch(b->scores.p, dst, bytes, agx_enqueue_stream(b->ctx))) {
        agx_set_error("agx_sw_batch_scores: copy kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        return AGX_E_HIP;
    }
    AGX_HIP(hipStreamSynchronize(b->ctx->stream));
    if (dst != scores) memcpy(scores, dst, bytes);
    for (size_t k = 0; k < b->fix_pair.size(); ++k) scores[b->fix_pair[k]] = b->fix_score[k];
    return AGX_OK;
}

int agx_sw_batch_bind_scores(agx_sw_batch *b, int32_t *scores)
{
    if (!b) {
        agx_set_error("agx_sw_batch_bind_scores: null batch");
        return AGX_E_ARG;
    }
    if (!b->ctx) {
        agx_set_error("this batch was planned without a context (no device)");
        return AGX_E_NODEVICE;
    }
    if (scores && !agx_is_pinned_host(scores, (size_t)std::max<int64_t>(b->n_pairs, 1) * sizeof(int32_t))) {
        agx_set_error("agx_sw_batch_bind_scores: the array is not page-locked memory of agx_host_alloc (or too short for %lld scores)", (long long)b->n_pairs);
        return AGX_E_ARG;
    }
    const int rc = agx_bind(b->ctx);
    if (rc) return rc;
    AGX_HIP(hipStreamSynchronize(b->ctx->stream)); // launches in flight still write the old destination
    // only a batch whose records are in file order takes the binding (a sorted batch's waves would scatter 4-byte
    // writes over PCIe: measured slower than the copy kernel behind the fill); the call is a hint otherwise
    int32_t *const bound = (scores && b->file_order && b->n_pairs > 0 && !b->matrix && !b->align) ? scores : nullptr;
    if (bound != b->bound) b->rebound = true; // the last launch wrote elsewhere: agx_sw_batch_scores refuses until the next one
    b->bound = bound;
    if (trace_fetch()) fprintf(stderr, "[agx_sw_batch_bind_scores] bound %d\n", bound ? 1 : 0);
    return AGX_OK;
}

int agx_sw_batch_info(const agx_sw_batch *b, agx_sw_info *info)
{
    if (!b || !info) {
        agx_set_error("agx_sw_batch_info: null argument");
        return AGX_E_ARG;
    }
    *info = b->info;
    return AGX_OK;
}

int agx_sw_score(agx_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                 int32_t *scores)
{
    AGX_GUARD_BEGIN
    // A batch of 64 MB and more goes through in up to eight contiguous pieces of at least 32 MB of sequence: piece k + 1 is
    // uploaded, planned and packed (copy and planning streams) while piece k is being filled (launch stream), so the call
    // lasts about as long as the upload plus the last piece's fill instead of upload + fill (1 048 576 mixed pairs, 573 MB,
    // from page-locked memory: 25.2 -> 12.7 ms).  Scores are fetched at the end, piece by piece, into
    // the caller's array.
    int pieces = 1;
    if (ctx && n_pairs >= 2 * piece_min_pairs() && len) {
        std::vector<uint64_t> part((size_t)agx_host_threads(), 0);
        agx_parallel_for(n_pairs, 65536, [&](int64_t lo, int64_t hi, int t) {
            uint64_t s = 0;
            for (int64_t p = 2 * lo; p < 2 * hi; ++p) s += len[p];
            part[(size_t)t] = s;
        });
        uint64_t bytes = 0;
        for (uint64_t v : part) bytes += v;
        // at most eight pieces (more cost a pageable source's staging more than they hide), none below 32 MB / 32 768 pairs
        // (tools/piece_size_sweep.sh: config 4's 72 MB shard 2.96 -> 2.31 ms in two pieces, 2.73 in four)
        pieces = (int)std::min<uint64_t>({(uint64_t)8, bytes / piece_bytes(), (uint64_t)(n_pairs / piece_min_pairs())});
        if (pieces < 2) pieces = 1;
    }
    if (pieces == 1) {
        agx_sw_batch *b = nullptr;
        int rc = agx_sw_batch_create(ctx, bases, off, len, n_pairs, &b);
        if (rc) return rc;
        rc = agx_sw_batch_launch(b);
        if (!rc) rc = agx_sw_batch_scores(b, scores);
        agx_sw_batch_destroy(b); // its buffers return to the context's pools for the next call
        return rc;
    }
    std::vector<agx_sw_batch *> bs((size_t)pieces, nullptr);
    struct Cleanup {
        std::vector<agx_sw_batch *> &v;
        ~Cleanup()
        {
            for (agx_sw_batch *b : v) agx_sw_batch_destroy(b);
        }
    } cleanup{bs};
    auto cut = [&](int k) { return n_pairs * k / pieces; };
    // Every piece is created WITHOUT its closing wait and launched behind an event: the copy stream carries the pieces'
    // uploads back to back, the planning stream their planning and pack kernels, the launch stream their fills, and
    // the host is ahead of all three.  The verdicts of the symbol checks are collected afterwards, piece by piece (the
    // first failing piece holds the smallest offending pair).
    auto renumber = [&](int rc, int64_t lo) { // the messages name pair numbers: of the whole batch, not of the piece
        if (rc == AGX_E_SYMBOL || rc == AGX_E_LIMIT) {
            unsigned long long p = 0;
            char rest[400] = "";
            if (sscanf(agx_last_error(), "pair %llu%399[^\n]", &p, rest) >= 1) agx_set_error("pair %llu%s", p + (unsigned long long)lo, rest);
        }
        return rc;
    };
    const bool trace = agx_tune("AGX_TRACE_CREATE") != nullptr;
    const double t_begin = agx_now_ms();
    for (int k = 0; k < pieces; ++k) {
        const int64_t lo = cut(k), hi = cut(k + 1);
        const double ta = agx_now_ms();
        int rc = renumber(create_batch(ctx, nullptr, nullptr, bases, off + 2 * lo, len + 2 * lo, hi - lo, &bs[(size_t)k], true), lo);
        if (!rc) rc = agx_sw_batch_launch(bs[(size_t)k]);
        if (rc) return rc;
        if (trace) fprintf(stderr, "[agx_sw_score] piece %d of %d queued in %.2f ms (at %.2f)\n", k, pieces, agx_now_ms() - ta, agx_now_ms() - t_begin);
    }
    for (int k = 0; k < pieces; ++k) {
        const int rc = renumber(finish_create(bs[(size_t)k]), cut(k));
        if (rc) return rc;
        if (trace) fprintf(stderr, "[agx_sw_score] piece %d finished at %.2f ms\n", k, agx_now_ms() - t_begin);
    }
    for (int k = 0; k < pieces; ++k) {
        const int rc = agx_sw_batch_scores(bs[(size_t)k], scores + cut(k));
        if (rc) return rc;
        agx_sw_batch_destroy(bs[(size_t)k]);
        bs[(size_t)k] = nullptr;
    }
    return AGX_OK;
    AGX_GUARD_END("agx_sw_score")
}

int agx_sw_shard_cuts(const uint32_t *len, int64_t n_pairs, int n_shards, int64_t *cut)
{
    if (n_pairs < 0 || n_shards < 1 || !cut || (n_pairs > 0 && !len)) {
        agx_set_error("agx_sw_shard_cuts: bad arguments");
        return AGX_E_ARG;
    }
    agx_cut_by_weight(n_pairs, n_shards, cut, [len](int64_t p) { return (double)len[2 * p] * len[2 * p + 1]; }); // by cells
    return AGX_OK;
}

int agx_sw_score_devices(const int *devices, int n_devices, const uint8_t *bases, const uint64_t *off, const uint32_t *len,
                         int64_t n_pairs, int32_t *scores)
{
    AGX_GUARD_BEGIN
    return agx_run_shards(
        "agx_sw_score_devices", devices, n_devices, n_pairs >= 0 && (n_pairs == 0 || (off && len && scores)),
        [&](int64_t *cut) { return agx_sw_shard_cuts(len, n_pairs, n_devices, cut); },
        [&](agx_ctx *c, int64_t lo, int64_t hi) { return agx_sw_score(c, bases, off + 2 * lo, len + 2 * lo, hi - lo, scores + lo); });
    AGX_GUARD_END("agx_sw_score_devices")
}

int agx_sw_score_multi(int n_devices, const uint8_t *bases, const uint64_t *off, const uint32_t *len, int64_t n_pairs,
                       int32_t *scores)
{
    int devs[1024];
    n_devices = agx_first_devices(n_devices, devs);
    return n_devices ? agx_sw_score_devices(devs, n_devices, bases, off, len, n_pairs, scores) : AGX_E_NODEVICE;
}

} // extern "C"
