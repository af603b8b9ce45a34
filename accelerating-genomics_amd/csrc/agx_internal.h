// Internal to libagx.so: context object, error plumbing, pooled device / pinned buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/agx.h"

extern "C" void agx_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define AGX_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            agx_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? AGX_E_NOMEM : AGX_E_HIP;                        \
        }                                                                                      \
    } while (0)

// Every extern "C" entry point that can allocate runs its body through this: a C caller must never see
// a C++ exception (std::bad_alloc from a std::vector, std::system_error from a thread).
#define AGX_GUARD_BEGIN try {
#define AGX_GUARD_END(fn_name)                                     \
    }                                                              \
    catch (const std::bad_alloc &)                                 \
    {                                                              \
        agx_set_error("%s: out of host memory", fn_name);          \
        return AGX_E_NOMEM;                                        \
    }                                                              \
    catch (const std::exception &ex_)                              \
    {                                                              \
        agx_set_error("%s: %s", fn_name, ex_.what());              \
        return AGX_E_NOMEM;                                        \
    }

// Experiment and test knobs (AGX_SW_FORCE_C, AGX_*_TAIL_BETA, AGX_FANOUT, ...) exist only in the tuning
// build (libagx_tuning.so, -DAGX_TUNING; tools/ and the calibration scripts load that one).  The shipped
// libagx.so reads no environment variable: it behaves the same in every process.
static inline const char *agx_tune(const char *name)
{
#ifdef AGX_TUNING
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// A knob's value: e (pass the agx_tune("NAME") call itself, so that the name stays where the knob list's test finds it) read
// as an integer or a real number; dflt when the knob is unset or its value fails the knob's own rule ok.
static inline long agx_knob_int(const char *e, long dflt, bool (*ok)(long) = nullptr)
{
    if (!e) return dflt;
    const long v = atol(e);
    return !ok || ok(v) ? v : dflt;
}
static inline double agx_knob_real(const char *e, double dflt, bool (*ok)(double) = nullptr)
{
    if (!e) return dflt;
    const double v = atof(e);
    return !ok || ok(v) ? v : dflt;
}

// the create traces' clock (AGX_TRACE_CREATE)
static inline double agx_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// AGX_TRACE_CREATE: a plan (or an image) as one number, 64-bit FNV-1a field by field -- never over struct padding; a float or
// a double goes in by its bit pattern.  tests/test_sw_plan_digest_cpu.py, tests/test_sw_band_plan_digest_cpu.py and
// tests/test_phmm_plan_digest_cpu.py pin the digests per kind of batch.
struct Fnv1a {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n)
    {
        for (size_t k = 0; k < n; ++k) h = (h ^ ((const uint8_t *)p)[k]) * 0x100000001b3ull;
    }
    template <typename T>
    void field(T v)
    {
        bytes(&v, sizeof v);
    }
};

constexpr int kAuxStreams = 3;

struct PoolBlock {
    void *p;
    size_t bytes;
};

struct agx_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Work the library has put on `stream`, counted (agx_enqueue_stream): a Smith-Waterman launch that carries its batch's done
    // event notes the count it leaves behind, and agx_sw_batch_scores waits for that event only while the count still stands
    // there -- after anything else it waits for the stream, as every other fetch does (agx_sw.cpp, "Completion on the dispatch")
    uint64_t enqueued = 0;
    int n_cu = 0;
    // Uploads run on their own stream so that building batch k+1 overlaps the fill of batch k.
    hipStream_t copy = nullptr;
    // Side streams for batches that need several kernel launches (one per lane-tiling class):
    // the launches are independent, so they are spread over the main stream and these, forked
    // and joined with events -- the tail of one class overlaps the head of the next.
    hipStream_t aux[kAuxStreams] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[kAuxStreams] = {nullptr, nullptr, nullptr};
    // Batches keep their context alive: agx_ctx_destroy() only drops the creator's reference, the
    // streams and the pools go when the last batch has been destroyed too (any destroy order is fine).
    std::atomic<int> refs{1};
    // Free device / pinned-host blocks kept for the next batch: hipMalloc / hipFree / hipHostMalloc cost
    // 0.1 .. several ms each and hipFree synchronises the device.
    std::mutex pool_mu;
    std::vector<PoolBlock> free_dev, free_pin;
    size_t cached_dev = 0, cached_pin = 0;
    // Device-side planning (agx_sw_plan_kernel.hip): its own stream, so that the planning kernels run beside the
    // upload of the sequences on `copy`, an event the pack kernel waits for, and the tiling table of the packed
    // biased fill on the device (made on first use, freed with the context).
    hipStream_t plan = nullptr;
    int prio_hi = 0; // highest stream priority of the device (copy and planning streams)
    hipEvent_t plan_done = nullptr;
    void *sw_seg_first = nullptr, *sw_segs = nullptr;
    // options (agx_ctx_set_option)
    int opt_sw_kernel = 0;
    int opt_sw_planner = 0;
    int opt_phmm_trains = 0;
    int64_t opt_sw_trace_bytes = (int64_t)1 << 30; // AGX_OPT_SW_TRACE_BYTES
};

int agx_ctx_prepare_fanout(agx_ctx *c); // side streams + events for batches of several launches
int agx_ctx_prepare_plan(agx_ctx *c);   // the planning stream and its event
void agx_ctx_retain(agx_ctx *c);
void agx_ctx_release(agx_ctx *c); // frees everything when the last reference goes

// Usage: FanOut f(ctx, n_launches); f.begin(); ... launch k on f.stream(k) ...; f.end();
// Everything is ordered after prior work on ctx->stream and before later work on it.
struct FanOut {
    agx_ctx *c;
    int n;
    bool used[kAuxStreams] = {false, false, false};
    FanOut(agx_ctx *ctx, int n_launches) : c(ctx), n(n_launches) {}
    int begin();
    hipStream_t stream(int k);
    int end();
};

// Device buffer drawn from its context's pool (freed explicitly so error paths stay simple C-style).
struct DevBuf {
    agx_ctx *ctx = nullptr;
    void *p = nullptr;
    size_t bytes = 0; // requested size; the block behind it may be larger
    size_t block = 0;
    int alloc(agx_ctx *c, size_t n);
    void release();
};

// Pinned host staging buffer drawn from the context's pool.
struct PinBuf {
    agx_ctx *ctx = nullptr;
    void *p = nullptr;
    size_t bytes = 0, block = 0;
    int alloc(agx_ctx *c, size_t n);
    void release();
};

// The exits of a batch create.  A create queues copies and kernels on the context's copy and planning streams that read its
// pinned staging and write pooled device blocks (the batch's own and its temporaries).  On success it has waited for them, or
// hands them on with the batch (the pieces of agx_sw_score, finished later); an error exit -- a return or an exception -- may
// leave them running, and a block handed back to its pool could be taken by another create mid-transfer.  So a DrainOnError
// is declared after the owners of those blocks and runs first as the create leaves: it joins the upload thread (which may
// still be queuing), drains both streams unless the create set ok, and then calls release, which frees the temporaries and
// destroys the half-built batch.  A success path gains no wait.
template <typename F>
struct DrainOnError {
    agx_ctx *ctx; // null: a plan-only batch, nothing was queued
    F release;
    std::thread *uploader = nullptr;
    bool ok = false;
    DrainOnError(agx_ctx *c, F f, std::thread *t = nullptr) : ctx(c), release(f), uploader(t) {}
    DrainOnError(const DrainOnError &) = delete;
    ~DrainOnError()
    {
        if (uploader && uploader->joinable()) uploader->join();
        if (!ok && ctx)
            for (hipStream_t s : {ctx->copy, ctx->plan})
                if (s) (void)hipStreamSynchronize(s);
        release();
    }
};

static inline int agx_bind(const agx_ctx *c)
{
    if (!c) {
        agx_set_error("null context");
        return AGX_E_ARG;
    }
    AGX_HIP(hipSetDevice(c->device));
    return AGX_OK;
}

// The context's stream for a call that is about to put work on it -- a kernel, a copy, an event record, a wait for an event:
// every such site takes the stream here, so that agx_ctx::enqueued counts them all.  (Waiting for the stream takes c->stream.)
static inline hipStream_t agx_enqueue_stream(agx_ctx *c)
{
    ++c->enqueued;
    return c->stream;
}

// memcpy with streaming stores, for staging copies into page-locked memory (agx_runtime.cpp)
void agx_stream_copy(void *dst, const void *src, size_t n);

// true when [p, p + bytes) lies in a block handed out by agx_host_alloc (page-locked: the device can DMA into or
// out of it directly).  A registry of our own rather than hipPointerGetAttributes: asked about an ordinary
// malloc'ed pointer, the runtime's first answer in a process took 7.5 ms (tools/first_call_costs.py) -- inside
// the launch -> scores window of a fresh process.  Memory pinned by other means is treated as pageable (staged).
bool agx_is_pinned_host(const void *p, size_t bytes);

// device -> page-locked host memory by a kernel on stream s (agx_copy_kernel.hip); both pointers 16-byte aligned
int agx_copy_out_launch(const void *src, void *dst, size_t bytes, hipStream_t s);
void agx_copy_preload();

// Process-wide contexts for the entry points that take device ordinals instead of a context
// (agx_*_devices, agx_*_multi, agx_pairHMM): created on first use, kept until the process ends.
// slot distinguishes several shards mapped onto the same device.
// *busy (may be NULL) receives the context's own mutex: a shard holds it while it uses the context, so that two
// host threads calling agx_*_devices at once take turns per (device, slot) instead of interleaving on its streams.
int agx_shared_ctx(int device, int slot, agx_ctx **out, std::mutex **busy = nullptr);

// Contiguous shards balanced by weight: cut[0] = 0, cut[n_shards] = n_units, shard d ends behind the first unit
// at which the running sum of weight(i) + 1, in unit order, reaches d / n_shards of the total (dist.shard_bounds mirrors it).
template <typename T, typename W>
void agx_cut_by_weight(int64_t n_units, int n_shards, T *cut, W weight)
{
    for (int d = 0; d <= n_shards; ++d) cut[d] = (T)n_units;
    cut[0] = 0;
    double total = 0;
    for (int64_t i = 0; i < n_units; ++i) total += weight(i) + 1.0;
    double acc = 0;
    int d = 1;
    for (int64_t i = 0; i < n_units && d < n_shards; ++i) {
        acc += weight(i) + 1.0;
        while (d < n_shards && acc >= total * d / n_shards) cut[d++] = (T)(i + 1);
    }
}

// The body of agx_*_devices (fn: its name, for the messages).  Checks, in this order: a device is visible (AGX_E_NODEVICE), the
// caller's args_ok (AGX_E_ARG), every ordinal in range (AGX_E_NODEVICE).  Then cuts(cut) fills the n_devices + 1 shard
// boundaries, and shard(ctx, lo, hi) runs for every shard with work, one host thread each (agx_fan_out), on a process-wide
// context of devices[k] whose lock it holds.  The first failing shard in shard order is reported as "device %d: ...".
int agx_run_shards(const char *fn, const int *devices, int n_devices, bool args_ok, const std::function<int(int64_t *cut)> &cuts,
                   const std::function<int(agx_ctx *ctx, int64_t lo, int64_t hi)> &shard);
// agx_*_multi: devices 0 .. n - 1 into devs[1024], n = n_devices, or every visible device when n_devices <= 0 or exceeds them;
// returns n, 0 (with the error text set) when no device is visible
int agx_first_devices(int n_devices, int *devs);
