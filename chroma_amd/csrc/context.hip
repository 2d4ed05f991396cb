// context.hip -- contexts of libchroma_hip.so: chroma_init / chroma_shutdown, the thread's error message, the device-memory
// pool behind chroma_malloc / chroma_free, the pinned staging rings behind the chroma_memcpy_* copies.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "chroma_internal.h"
#include "host_utils.h"

// ---------------------------------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// ---- device memory: a pool -----------------------------------------------------------------------------------
// Simulation builds a GPUPhotons per event batch: ten arrays allocated, used for one propagate, dropped.  hipMalloc and
// hipFree each cost ~0.1-1 ms for blocks of hundreds of MB and hipFree synchronises the device, so blocks are kept
// instead: chroma_free parks a block (with an event recorded on the context's stream: work already queued on it may
// still use the block), chroma_malloc hands a parked block of exactly the requested size back once that event has
// completed -- no waiting, no new allocation.  Capped at CHROMA_POOL_MB (default: 40 % of the device's memory);
// chroma_pool_trim releases everything parked (also done by itself when hipMalloc runs out of memory).
static size_t pool_round(size_t nbytes) { return (std::max(nbytes, (size_t)4) + 255) & ~(size_t)255; }

static void pool_release_all(chroma_ctx *ctx)       // (pool_mu held)
{
    for (auto &kv : ctx->pool) { hipEventSynchronize(kv.second.ev); hipFree(kv.second.ptr); ctx->pool_events.push_back(kv.second.ev); }
    ctx->pool.clear();
    ctx->pool_bytes = 0;
}

hipError_t ctx_malloc(chroma_ctx *ctx, void **ptr, size_t bytes)
{
    hipError_t e = hipMalloc(ptr, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lock(ctx->pool_mu);
        if (!ctx->pool.empty()) { pool_release_all(ctx); e = hipMalloc(ptr, bytes); }
    }
    return e;
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
extern "C" {

const char *chroma_last_error(void) { return g_last_error.c_str(); }
const char *chroma_version(void) { return "chroma_hip 0.1 (gfx950)"; }

int chroma_device_count(int *count)
{
    if (!count) return set_error(CHROMA_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return set_error(CHROMA_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return CHROMA_OK;
}

int chroma_init(int device, chroma_ctx **out)
{
    if (!out) return set_error(CHROMA_ERR_INVALID, "null ctx");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return set_error(CHROMA_ERR_NO_DEVICE, "no HIP device available (libchroma_hip needs an MI355X/gfx950 GPU)");
    if (device < 0) device = 0;
    if (device >= n) return set_error(CHROMA_ERR_INVALID, "device %d out of range (%d devices)", device, n);
    HIP_TRY(hipSetDevice(device));
    chroma_ctx *ctx = new chroma_ctx;
    ctx->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        ctx->pool_limit = (size_t)(0.4 * (double)total_b);
        if (const char *e = getenv("CHROMA_POOL_MB")) ctx->pool_limit = (size_t)std::max(0ll, atoll(e)) << 20;
    }
    const CallScope scope(ctx);
    CallState &cs = scope.state();
    HIP_TRY(hipStreamCreateWithFlags(&cs.aux_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&cs.ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&cs.ev_join, hipEventDisableTiming));
    HIP_TRY(hipMalloc((void **)&cs.d_counters, sizeof(DeviceCounters)));
    HIP_TRY(hipMemset(cs.d_counters, 0, sizeof(DeviceCounters)));
    HIP_TRY(hipMalloc((void **)&cs.d_words, SCRATCH_WORDS * sizeof(uint32_t)));
    HIP_TRY(hipMemset(cs.d_words, 0, SCRATCH_WORDS * sizeof(uint32_t)));
    HIP_TRY(hipHostMalloc((void **)&cs.h_words, SCRATCH_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipMalloc((void **)&cs.d_step, sizeof(StepState)));
    HIP_TRY(hipMemset(cs.d_step, 0, sizeof(StepState)));
    HIP_TRY(hipHostMalloc((void **)&cs.h_step, sizeof(StepState), hipHostMallocDefault));
    { const int rc = propagate_settings(scope); if (rc) return rc; }
    HIP_TRY(hipEventCreate(&cs.ev_start));
    HIP_TRY(hipEventCreate(&cs.ev_stop));
    HIP_TRY(hipEventCreate(&cs.ev_mid));
    *out = ctx;
    return CHROMA_OK;
}

int chroma_shutdown(chroma_ctx *ctx)
{
    if (!ctx) return CHROMA_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipStreamSynchronize(ctx->copy_stream);
    chroma_comm_destroy(ctx);
    { std::lock_guard<std::mutex> lock(ctx->pool_mu); pool_release_all(ctx); for (hipEvent_t e : ctx->pool_events) hipEventDestroy(e); ctx->pool_events.clear(); }
    for (int i = 0; i < chroma_ctx::STAGE_N; i++) { if (ctx->stage[i]) hipHostFree(ctx->stage[i]); if (ctx->stage_ev[i]) hipEventDestroy(ctx->stage_ev[i]); }
    for (int i = 0; i < chroma_ctx::STAGE_N; i++) { if (ctx->stage_down[i]) hipHostFree(ctx->stage_down[i]); if (ctx->stage_down_ev[i]) hipEventDestroy(ctx->stage_down_ev[i]); }
    hipStreamDestroy(ctx->copy_stream);
    {
        const CallScope scope(ctx);          // (gone before the context and its mutex are)
        CallState &cs = scope.state();
        if (cs.aux_stream) { hipStreamSynchronize(cs.aux_stream); hipStreamDestroy(cs.aux_stream); }
        if (cs.ev_fork) hipEventDestroy(cs.ev_fork);
        if (cs.ev_join) hipEventDestroy(cs.ev_join);
        for (const QueueBuffer &b : queue_buffers(cs)) if (*b.ptr) hipFree(*b.ptr);
        if (cs.wide_spill) hipFree(cs.wide_spill);
        if (cs.coop_spill) hipFree(cs.coop_spill);
        if (cs.d_step) hipFree(cs.d_step);
        if (cs.call_scratch) hipFree(cs.call_scratch);
        if (cs.h_step) hipHostFree(cs.h_step);
        for (hipEvent_t e : cs.step_events) hipEventDestroy(e);
        hipFree(cs.d_counters);
        hipFree(cs.d_words);
        hipHostFree(cs.h_words);
        hipEventDestroy(cs.ev_start);
        hipEventDestroy(cs.ev_stop);
        hipEventDestroy(cs.ev_mid);
    }
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return CHROMA_OK;
}

int chroma_synchronize(chroma_ctx *ctx)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHROMA_OK;
}

int chroma_mem_info(chroma_ctx *ctx, size_t *free_bytes, size_t *total_bytes)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return CHROMA_OK;
}

int chroma_device_name(chroma_ctx *ctx, char *buf, size_t buflen)
{
    if (!ctx || !buf || !buflen) return set_error(CHROMA_ERR_INVALID, "bad argument");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return CHROMA_OK;
}


int chroma_malloc(chroma_ctx *ctx, size_t nbytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return set_error(CHROMA_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t size = pool_round(nbytes);
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    auto range = ctx->pool.equal_range(size);
    for (auto it = range.first; it != range.second; ++it) {
        // (still in use by queued work: hipErrorNotReady is not an error here, and must not stay behind as the thread's
        //  "last error" for the next hipGetLastError() after a kernel launch to find)
        if (hipEventQuery(it->second.ev) != hipSuccess) { (void)hipGetLastError(); continue; }
        *d_ptr = it->second.ptr;
        ctx->pool_events.push_back(it->second.ev);
        ctx->pool.erase(it);
        ctx->pool_bytes -= size;
        ctx->live[*d_ptr] = size;
        ctx->pool_hits++;
        return CHROMA_OK;
    }
    hipError_t e = hipMalloc(d_ptr, size);
    if (e == hipErrorOutOfMemory && !ctx->pool.empty()) {
        (void)hipGetLastError();
        pool_release_all(ctx);
        e = hipMalloc(d_ptr, size);
    }
    if (e != hipSuccess) return set_error((int)e, "hipMalloc(%zu bytes) failed: %s", size, hipGetErrorString(e));
    ctx->live[*d_ptr] = size;
    ctx->pool_misses++;
    return CHROMA_OK;
}

int chroma_free(chroma_ctx *ctx, void *d_ptr)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (!d_ptr) return CHROMA_OK;
    // (a Python __del__ or the prefetch worker may call this from a thread whose current device is another GPU's)
    HIP_TRY(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    auto it = ctx->live.find(d_ptr);
    if (it == ctx->live.end()) {                   // not one of ours (should not happen): the old behaviour
        HIP_TRY(hipStreamSynchronize(ctx->stream)); HIP_TRY(hipFree(d_ptr));
        return CHROMA_OK;
    }
    const size_t size = it->second;
    ctx->live.erase(it);
    bool park = ctx->pool_bytes + size <= ctx->pool_limit;
    hipEvent_t ev = nullptr;
    if (park) {
        // a block is parked behind an event on the context's stream; should the event not come about, the block is
        // simply freed (after the stream has drained) -- it must never be left neither parked nor freed
        if (!ctx->pool_events.empty()) { ev = ctx->pool_events.back(); ctx->pool_events.pop_back(); }
        else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; park = false; }
        if (park && hipEventRecord(ev, ctx->stream) != hipSuccess) { ctx->pool_events.push_back(ev); park = false; }
    }
    if (!park) {
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(ctx->stream)); HIP_TRY(hipFree(d_ptr));
        return CHROMA_OK;
    }
    ctx->pool.emplace(size, chroma_ctx::PoolBlock{d_ptr, ev});
    ctx->pool_bytes += size;
    return CHROMA_OK;
}

int chroma_pool_trim(chroma_ctx *ctx)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    pool_release_all(ctx);
    return CHROMA_OK;
}

int chroma_pool_stats(chroma_ctx *ctx, uint64_t *parked_bytes, uint64_t *reused, uint64_t *allocated)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->pool_mu);
    if (parked_bytes) *parked_bytes = ctx->pool_bytes;
    if (reused) *reused = ctx->pool_hits;
    if (allocated) *allocated = ctx->pool_misses;
    return CHROMA_OK;
}

// ---- host -> device ------------------------------------------------------------------------------------------
// A copy from pageable host memory runs at ~11 GB/s through the runtime's own bounce buffer (one thread).  Large copies
// are staged here instead: the host threads copy 64 MB pieces into a ring of PINNED buffers in parallel and each piece
// goes to the device by DMA while the next is being staged.  (r03: 11.2 -> 16 GB/s with 32 MB pieces and 64 threads on
// a 16-core quota; the thread count now follows the quota.)
static int staged_htod(chroma_ctx *ctx, hipStream_t stream, void *d_dst, const void *h_src, size_t nbytes)
{
    std::lock_guard<std::mutex> lock(ctx->stage_mu);
    for (int i = 0; i < chroma_ctx::STAGE_N; i++)
        if (!ctx->stage[i]) {
            HIP_TRY(hipHostMalloc(&ctx->stage[i], chroma_ctx::STAGE_BYTES, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&ctx->stage_ev[i], hipEventDisableTiming));
        }
    size_t off = 0;
    int k = 0;
    while (off < nbytes) {
        const size_t len = std::min(chroma_ctx::STAGE_BYTES, nbytes - off);
        HIP_TRY(hipEventSynchronize(ctx->stage_ev[k]));            // (the DMA that last read this buffer is done)
        char *dst = (char *)ctx->stage[k];
        const char *src = (const char *)h_src + off;
        chroma_host::parallel_for(len, [&](size_t a, size_t b) { memcpy(dst + a, src + a, b - a); }, 1u << 20);
        HIP_TRY(hipMemcpyAsync((char *)d_dst + off, dst, len, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ctx->stage_ev[k], stream));
        off += len;
        k = (k + 1) % chroma_ctx::STAGE_N;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_memcpy_htod(chroma_ctx *ctx, void *d_dst, const void *h_src, size_t nbytes)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (nbytes == 0) return CHROMA_OK;
    if (nbytes >= (8u << 20)) return staged_htod(ctx, ctx->stream, d_dst, h_src, nbytes);
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHROMA_OK;
}

// The same copy on the context's SECOND stream: not ordered with the work queued on the main stream, so that the
// photons of the next event batch can go up while the current batch propagates (Simulation, one thread ahead).  The
// destination must not be in use by queued work: a block fresh from chroma_malloc never is.  Returns when the data is
// on the device.
int chroma_upload(chroma_ctx *ctx, void *d_dst, const void *h_src, size_t nbytes)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (nbytes == 0) return CHROMA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (nbytes >= (8u << 20)) return staged_htod(ctx, ctx->copy_stream, d_dst, h_src, nbytes);
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, ctx->copy_stream));
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    return CHROMA_OK;
}

// ---- device -> host: the same ring the other way round -- a piece comes down by DMA into a pinned buffer while the host
// threads copy the previous one out to (pageable, possibly never touched) destination memory in parallel
static int staged_dtoh(chroma_ctx *ctx, hipStream_t stream, void *h_dst, const void *d_src, size_t nbytes)
{
    std::lock_guard<std::mutex> lock(ctx->stage_down_mu);
    for (int i = 0; i < chroma_ctx::STAGE_N; i++)
        if (!ctx->stage_down[i]) {
            HIP_TRY(hipHostMalloc(&ctx->stage_down[i], chroma_ctx::STAGE_BYTES, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&ctx->stage_down_ev[i], hipEventDisableTiming));
        }
    const size_t npieces = (nbytes + chroma_ctx::STAGE_BYTES - 1) / chroma_ctx::STAGE_BYTES;
    auto issue = [&](size_t i) -> hipError_t {
        const size_t off = i * chroma_ctx::STAGE_BYTES, len = std::min(chroma_ctx::STAGE_BYTES, nbytes - off);
        const int k = (int)(i % chroma_ctx::STAGE_N);
        hipError_t e = hipMemcpyAsync(ctx->stage_down[k], (const char *)d_src + off, len, hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipEventRecord(ctx->stage_down_ev[k], stream);
    };
    HIP_TRY(issue(0));
    for (size_t i = 0; i < npieces; i++) {
        if (i + 1 < npieces) HIP_TRY(issue(i + 1));               // (its buffer was copied out two pieces ago)
        const size_t off = i * chroma_ctx::STAGE_BYTES, len = std::min(chroma_ctx::STAGE_BYTES, nbytes - off);
        const int k = (int)(i % chroma_ctx::STAGE_N);
        HIP_TRY(hipEventSynchronize(ctx->stage_down_ev[k]));
        const char *src = (const char *)ctx->stage_down[k];
        char *dst = (char *)h_dst + off;
        chroma_host::parallel_for(len, [&](size_t a, size_t b) { memcpy(dst + a, src + a, b - a); }, 1u << 20);
    }
    return CHROMA_OK;
}

int chroma_memcpy_dtoh(chroma_ctx *ctx, void *h_dst, const void *d_src, size_t nbytes)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (nbytes == 0) return CHROMA_OK;
    if (nbytes >= (8u << 20)) return staged_dtoh(ctx, ctx->stream, h_dst, d_src, nbytes);
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHROMA_OK;
}

int chroma_memcpy_dtod(chroma_ctx *ctx, void *d_dst, const void *d_src, size_t nbytes)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (nbytes == 0) return CHROMA_OK;
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CHROMA_OK;
}

int chroma_memset32(chroma_ctx *ctx, void *d_dst, uint32_t value, size_t count)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (count == 0) return CHROMA_OK;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_dst, (int)value, count, ctx->stream));
    return CHROMA_OK;
}

}  // extern "C"
