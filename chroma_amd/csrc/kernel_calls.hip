// kernel_calls.hip -- the entry points that are the checks of their arguments around one kernel launch on the context's
// stream, as the reference's kernels are called from Python: the photon-array calls, DAQ, PDFs, chroma_render, point
// transforms, the probe, the bomb generator, the photons from particle steps, the time-binned DAQ and its trigger.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "chroma_internal.h"
#include "propagate_device.h"

#include "kernels_photons_hits.h"

#include "kernels_daq_render.h"

#include "kernels_daq_pulses.h"
#include "kernels_daq_noise.h"

#include "kernels_daq_trigger.h"

#include "kernels_pdf.h"

#include "kernels_steps.h"

// The count and copy calls: the hit word cleared, the launch it is given run on it (none for an empty range), the word read back
template <class Launch>
static int counted_launch(const CallScope &scope, bool any, uint32_t *count, Launch &&launch)
{
    uint32_t n = 0;
    int rc = scope.clear_words(W_HIT_COUNT); if (rc) return rc;
    if (any) { launch(scope.state().d_words + W_HIT_COUNT); HIP_TRY(hipGetLastError()); }
    rc = scope.read_word(W_HIT_COUNT, &n);
    if (count) *count = n;
    return rc;
}

// ---- photons from particle steps (kernels_steps.h) ----
// The context's scratch block of the two calls, in this order: the 64-bit total, the source's three tables, the 2 n + 1 counts,
// the scan's workspace.  A call grows the block when it has to and copies the tables up (they are host arrays of the caller's).
struct StepsScratch {
    unsigned long long *total; float *refractive_index, *scintillation_cdf, *time_cdf; uint32_t *counts; void *scan; size_t scan_bytes;
};
static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
static int steps_block(const CallScope &scope, size_t need)
{
    CallState &cs = scope.state();
    if (cs.steps_scratch_bytes >= need) return CHROMA_OK;
    HIP_TRY(hipStreamSynchronize(scope.ctx->stream));
    if (cs.steps_scratch) { HIP_TRY(hipFree(cs.steps_scratch)); cs.steps_scratch = nullptr; cs.steps_scratch_bytes = 0; }
    HIP_TRY(ctx_malloc(scope.ctx, &cs.steps_scratch, need));
    cs.steps_scratch_bytes = need;
    return CHROMA_OK;
}
static int steps_scratch(const CallScope &scope, const chroma_light_source *src, uint64_t nsegments, StepsScratch *out)
{
    hipStream_t stream = scope.ctx->stream;
    const size_t ncounts = 2 * (size_t)nsegments + 1;
    size_t scan_bytes = 0;
    { uint32_t *nul = nullptr; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nul, nul, (int)ncounts, stream)); }
    const size_t wl_bytes = round256(src->wavelength_n * sizeof(float)), t_bytes = src->time_cdf ? round256(src->time_n * sizeof(float)) : 0;
    const size_t need = 256 + 2 * wl_bytes + t_bytes + round256(ncounts * sizeof(uint32_t)) + round256(scan_bytes);
    int rc = steps_block(scope, need); if (rc) return rc;
    char *p = (char *)scope.state().steps_scratch;
    out->total = (unsigned long long *)p; p += 256;
    out->refractive_index = (float *)p; p += wl_bytes;
    out->scintillation_cdf = src->scintillation_cdf ? (float *)p : nullptr; p += wl_bytes;
    out->time_cdf = src->time_cdf ? (float *)p : nullptr; p += t_bytes;
    out->counts = (uint32_t *)p; p += round256(ncounts * sizeof(uint32_t));
    out->scan = p; out->scan_bytes = scan_bytes;
    HIP_TRY(hipMemcpyAsync(out->refractive_index, src->refractive_index, src->wavelength_n * sizeof(float), hipMemcpyHostToDevice, stream));
    if (src->scintillation_cdf)
        HIP_TRY(hipMemcpyAsync(out->scintillation_cdf, src->scintillation_cdf, src->wavelength_n * sizeof(float), hipMemcpyHostToDevice, stream));
    if (src->time_cdf) HIP_TRY(hipMemcpyAsync(out->time_cdf, src->time_cdf, src->time_n * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));          // (the caller's tables are his again when the call returns)
    return CHROMA_OK;
}

// ---- a medium per segment ----
// The device-resident table of chroma_light_media_create: ONE block of the context's pool, the three tables first (a row per
// medium), then the per-medium yields and n_max, then the prompt bytes.  Never written after it is made.
struct chroma_light_media {
    chroma_ctx *ctx;
    void *block;
    steps::Media view;
};
// the media calls' share of the context's scratch block: the 64-bit total, the 2 n + 1 counts, the scan's workspace (no tables)
static int media_scratch(const CallScope &scope, uint64_t nsegments, StepsScratch *out)
{
    const size_t ncounts = 2 * (size_t)nsegments + 1;
    size_t scan_bytes = 0;
    { uint32_t *nul = nullptr; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nul, nul, (int)ncounts, scope.ctx->stream)); }
    int rc = steps_block(scope, 256 + round256(ncounts * sizeof(uint32_t)) + round256(scan_bytes)); if (rc) return rc;
    char *p = (char *)scope.state().steps_scratch;
    *out = StepsScratch();
    out->total = (unsigned long long *)p; p += 256;
    out->counts = (uint32_t *)p; p += round256(ncounts * sizeof(uint32_t));
    out->scan = p; out->scan_bytes = scan_bytes;
    return CHROMA_OK;
}
static int check_media_call(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs, const int32_t *d_medium)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (media->ctx != ctx) return set_error(CHROMA_ERR_INVALID, "light media: made on another context");
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (segs->n && !d_medium) return set_error(CHROMA_ERR_INVALID, "segments: no medium array");
    return CHROMA_OK;
}

extern "C" {

int chroma_light_media_create(chroma_ctx *ctx, const chroma_light_media_desc *desc, chroma_light_media **media)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *media = nullptr;
    if (const char *why = steps::check_media(desc)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const size_t nm = desc->nmedia, wl_bytes = round256(nm * desc->wavelength_n * sizeof(float));
    const size_t t_bytes = round256(nm * std::max<size_t>(desc->time_n, 1) * sizeof(float)), m_bytes = round256(nm * sizeof(float));
    void *block = nullptr;
    int rc = chroma_malloc(ctx, 2 * wl_bytes + t_bytes + 3 * m_bytes, &block); if (rc) return rc;
    char *p = (char *)block;
    float *ri = (float *)p; p += wl_bytes;
    float *scint = (float *)p; p += wl_bytes;
    float *tcdf = (float *)p; p += t_bytes;
    float *yield = (float *)p; p += m_bytes;
    float *n_max = (float *)p; p += m_bytes;
    uint8_t *prompt = (uint8_t *)p;
    // one row at a time for the CDFs: a row that is ignored need not be readable, and is left as zeros
    std::vector<float> h_n_max(nm);
    steps::media_n_max(*desc, h_n_max.data());
    hipStream_t stream = ctx->stream;
    hipError_t e = hipMemsetAsync(scint, 0, wl_bytes + t_bytes, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ri, desc->refractive_index, nm * desc->wavelength_n * sizeof(float), hipMemcpyHostToDevice, stream);
    for (size_t m = 0; m < nm && e == hipSuccess; m++) {
        if (desc->light_yield[m] == 0.0f) continue;
        e = hipMemcpyAsync(scint + m * desc->wavelength_n, desc->scintillation_cdf + m * desc->wavelength_n, desc->wavelength_n * sizeof(float),
                           hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !desc->prompt[m])
            e = hipMemcpyAsync(tcdf + m * desc->time_n, desc->time_cdf + m * desc->time_n, desc->time_n * sizeof(float), hipMemcpyHostToDevice, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(yield, desc->light_yield, nm * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(n_max, h_n_max.data(), nm * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(prompt, desc->prompt, nm, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);          // (the caller's tables are his again when the call returns)
    if (e != hipSuccess) {
        chroma_free(ctx, block);
        return set_error((int)e, "light media: upload failed: %s", hipGetErrorString(e));
    }
    *media = new chroma_light_media{ctx, block, steps::make_media(*desc, ri, scint, tcdf, yield, prompt, n_max)};
    return CHROMA_OK;
}

int chroma_light_media_destroy(chroma_light_media *media)
{
    if (!media) return CHROMA_OK;
    const int rc = chroma_free(media->ctx, media->block);
    delete media;
    return rc;
}

int chroma_steps_count_media(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs, const int32_t *d_medium,
                             uint64_t seed, uint32_t *d_offsets, uint64_t *total)
{
    if (!d_offsets || !total) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_media_call(ctx, media, segs, d_medium); if (rc) return rc;
    const CallScope scope(ctx);
    *total = 0;
    if (segs->n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), ctx->stream));
        return CHROMA_OK;
    }
    StepsScratch sc;
    rc = media_scratch(scope, segs->n, &sc); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(sc.total, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_steps_count_media, dim3((unsigned)((segs->n + STEPS_BLOCK - 1) / STEPS_BLOCK)), dim3(STEPS_BLOCK), 0, ctx->stream,
                       media->view, *segs, d_medium, seed, sc.counts, sc.total);
    HIP_TRY(hipGetLastError());
    { size_t b = sc.scan_bytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc.scan, b, sc.counts, d_offsets, (int)(2 * segs->n + 1), ctx->stream)); }
    unsigned long long sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, sc.total, sizeof(sum), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *total = sum;
    if (sum > 0xffffffffull) return set_error(CHROMA_ERR_INVALID, "%llu photons in one call: more than 32-bit offsets hold, pass fewer segments", sum);
    return CHROMA_OK;
}

int chroma_steps_generate_media(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs, const int32_t *d_medium,
                                uint64_t seed, const uint32_t *d_offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (!d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_media_call(ctx, media, segs, d_medium); if (rc) return rc;
    if (segs->n == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_offsets + 2 * segs->n, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu photons, the segments emit %u", (unsigned long long)capacity, total);
    if (total == 0) return CHROMA_OK;
    rc = check_photons(photons, true); if (rc) return rc;
    hipLaunchKernelGGL(k_steps_generate_media, dim3((total + STEPS_BLOCK - 1) / STEPS_BLOCK), dim3(STEPS_BLOCK), 0, ctx->stream, media->view, *segs,
                       d_medium, seed, d_offsets, to_view(photons), total);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_steps_count(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                       uint32_t *d_offsets, uint64_t *total)
{
    if (!ctx || !d_offsets || !total) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = steps::check_source(src)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const CallScope scope(ctx);
    *total = 0;
    if (segs->n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), ctx->stream));
        return CHROMA_OK;
    }
    StepsScratch sc;
    int rc = steps_scratch(scope, src, segs->n, &sc); if (rc) return rc;
    const steps::Source s = steps::make_source(*src, sc.refractive_index, sc.scintillation_cdf, sc.time_cdf);
    HIP_TRY(hipMemsetAsync(sc.total, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_steps_count, dim3((unsigned)((segs->n + STEPS_BLOCK - 1) / STEPS_BLOCK)), dim3(STEPS_BLOCK), 0, ctx->stream, s, *segs, seed,
                       sc.counts, sc.total);
    HIP_TRY(hipGetLastError());
    { size_t b = sc.scan_bytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc.scan, b, sc.counts, d_offsets, (int)(2 * segs->n + 1), ctx->stream)); }
    unsigned long long sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, sc.total, sizeof(sum), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *total = sum;
    if (sum > 0xffffffffull) return set_error(CHROMA_ERR_INVALID, "%llu photons in one call: more than 32-bit offsets hold, pass fewer segments", sum);
    return CHROMA_OK;
}

int chroma_steps_generate(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                          const uint32_t *d_offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (!ctx || !d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = steps::check_source(src)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (segs->n == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_offsets + 2 * segs->n, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu photons, the segments emit %u", (unsigned long long)capacity, total);
    if (total == 0) return CHROMA_OK;
    int rc = check_photons(photons, true); if (rc) return rc;
    StepsScratch sc;
    rc = steps_scratch(scope, src, segs->n, &sc); if (rc) return rc;
    const steps::Source s = steps::make_source(*src, sc.refractive_index, sc.scintillation_cdf, sc.time_cdf);
    hipLaunchKernelGGL(k_steps_generate, dim3((total + STEPS_BLOCK - 1) / STEPS_BLOCK), dim3(STEPS_BLOCK), 0, ctx->stream, s, *segs, seed, d_offsets,
                       to_view(photons), total);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_photon_duplicate(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                            const chroma_photon_arrays *photons, int32_t copies, int32_t stride)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    int rc = check_photons(photons, false);
    if (rc) return rc;
    if (nthreads <= 0 || copies <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_photon_duplicate, dim3((nthreads + 255) / 256), dim3(256), 0, ctx->stream, to_view(photons),
                       first_photon, nthreads, copies, stride);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_count_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, uint32_t target_flag,
                         const uint32_t *d_flags, uint32_t *count)
{
    if (!ctx || !d_flags || !count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    return counted_launch(scope, nthreads > 0, count, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_count_photons, dim3((unsigned)std::min((nthreads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, d_flags, first_photon,
                           nthreads, target_flag, word);
    });
}

int chroma_copy_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, uint32_t target_flag,
                        const chroma_photon_arrays *src, const chroma_photon_arrays *dst, uint32_t *ncopied)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nthreads > 0, ncopied, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_copy_photons, dim3((unsigned)(((long long)nthreads + 16 * 256 - 1) / (16 * 256))), dim3(256), 0, ctx->stream, to_view(src), to_view(dst),
                           first_photon, nthreads, target_flag, word);
    });
}

int chroma_copy_photon_queue(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, const uint32_t *d_queue,
                             const chroma_photon_arrays *src, const chroma_photon_arrays *dst)
{
    if (!ctx || !d_queue) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    if (nthreads <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_copy_photon_queue, dim3((nthreads + 255) / 256), dim3(256), 0, ctx->stream, to_view(src), to_view(dst),
                       first_photon, nthreads, d_queue);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_count_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon, int32_t nphotons,
                             uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t *count)
{
    if (!ctx || !geom || !count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(photons, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nphotons > 0, count, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_count_hits, dim3((unsigned)std::min((nphotons + 255) / 256, 4096)), dim3(256), 0, ctx->stream, geom->view, photons->flags,
                           photons->last_hit_triangles, first_photon, nphotons, detection_state, word);
    });
}

int chroma_copy_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon, int32_t nphotons,
                            uint32_t detection_state, const chroma_photon_arrays *src, const chroma_photon_arrays *dst,
                            int32_t *d_channels, uint32_t *ncopied)
{
    if (!ctx || !geom || !d_channels) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nphotons > 0, ncopied, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_copy_hits, dim3((unsigned)(((long long)nphotons + COPY_ITEMS * 256 - 1) / (COPY_ITEMS * 256))), dim3(256), 0, ctx->stream, geom->view, to_view(src),
                           to_view(dst), d_channels, first_photon, nphotons, detection_state, word);
    });
}

int chroma_channel_hits(chroma_ctx *ctx, chroma_geometry *geom, uint64_t nphotons, uint32_t detection_state,
                        const chroma_photon_arrays *photons, uint32_t *d_hit_count, uint32_t *d_earliest_time_bits)
{
    if (!ctx || !geom || !d_hit_count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_channel_hits, dim3((unsigned)((nphotons + 255) / 256)), dim3(256), 0, ctx->stream, geom->view,
                       photons->flags, photons->last_hit_triangles, photons->t, (uint64_t)nphotons, detection_state,
                       d_hit_count, d_earliest_time_bits);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_reset(chroma_ctx *ctx, float maxtime, uint32_t nchannels, uint32_t *d_earliest_time_int,
                     uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nchannels == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_daq_reset, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, maxtime, nchannels,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, int32_t first_photon,
                       int32_t nphotons, uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng,
                       uint32_t acquisition, float global_weight, uint32_t *d_earliest_time_int,
                       uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (tables->time_cdf_len < 2 || tables->charge_cdf_len < 2 || !tables->d_time_cdf_x || !tables->d_time_cdf_y ||
        !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need two CDFs of at least 2 points and a positive charge unit");
    int rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_run_daq, dim3((nphotons + 255) / 256), dim3(256), 0, ctx->stream, geom->view, *tables, first_photon,
                       nphotons, detection_state, photons->t, photons->flags, photons->last_hit_triangles, photons->weights,
                       rng.seed, rng.photon_id_base, acquisition, global_weight, d_earliest_time_int, d_channel_q_int,
                       d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire_many(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, int32_t first_photon,
                            int32_t nphotons, uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng,
                            uint32_t acquisition, float global_weight, int32_t ndaq, int32_t channel_stride,
                            uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (ndaq < 1 || channel_stride < (int32_t)geom->view.nchannels)
        return set_error(CHROMA_ERR_INVALID, "ndaq must be positive and the channel stride at least the number of channels");
    if (tables->time_cdf_len < 2 || tables->charge_cdf_len < 2 || !tables->d_time_cdf_x || !tables->d_time_cdf_y ||
        !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need two CDFs of at least 2 points and a positive charge unit");
    int rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons <= 0) return CHROMA_OK;
    const long long total = (long long)nphotons * ndaq;
    hipLaunchKernelGGL(k_run_daq_many, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, geom->view, *tables,
                       first_photon, nphotons, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                       photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, ndaq, channel_stride,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire_events(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                              const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons,
                              uint32_t nphotons, chroma_rng rng, uint32_t acquisition, float global_weight,
                              uint32_t channel_stride, uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                              uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !bounds || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (nrows < 1 || channel_stride < geom->view.nchannels)
        return set_error(CHROMA_ERR_INVALID, "need at least one row and a channel stride of at least the number of channels");
    if ((uint64_t)nrows * channel_stride > 0xffffffffull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u words: more than 32-bit word indices hold, pass fewer rows", nrows, channel_stride);
    for (uint32_t r = 0; r < nrows; r++)
        if (bounds[r] > bounds[r + 1]) return set_error(CHROMA_ERR_INVALID, "event bounds: bound %u is below bound %u", r + 1, r);
    if (bounds[nrows] > nphotons || bounds[nrows] > 0x7fffffffu)
        return set_error(CHROMA_ERR_INVALID, "event bounds: the last bound %u is beyond the %u photons of the set", bounds[nrows], nphotons);
    if (tables->time_cdf_len < 2 || tables->charge_cdf_len < 2 || !tables->d_time_cdf_x || !tables->d_time_cdf_y ||
        !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need two CDFs of at least 2 points and a positive charge unit");
    int rc = check_photons(photons, false); if (rc) return rc;
    const uint32_t window = bounds[nrows] - bounds[0];
    if (window == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    rc = steps_block(scope, round256(((size_t)nrows + 1) * sizeof(uint32_t))); if (rc) return rc;
    uint32_t *d_bounds = (uint32_t *)scope.state().steps_scratch;
    HIP_TRY(hipMemcpyAsync(d_bounds, bounds, ((size_t)nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // (the caller's bounds are his again when the call returns)
    hipLaunchKernelGGL(k_run_daq_events, dim3((window + DAQ_EVENTS_BLOCK - 1) / DAQ_EVENTS_BLOCK), dim3(DAQ_EVENTS_BLOCK), 0, ctx->stream,
                       geom->view, *tables, nrows, d_bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                       photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, channel_stride,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_compact_events(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, uint32_t channel_stride, float charge_unit,
                              const uint32_t *d_earliest_time_int, const uint32_t *d_channel_q_int,
                              const uint32_t *d_channel_histories, uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel,
                              float *d_t, float *d_q, uint32_t *d_flags, uint64_t *ntouched)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories || !d_offsets || !ntouched ||
        (capacity && (!d_channel || !d_t || !d_q || !d_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    *ntouched = 0;
    if (nrows < 1 || nchannels < 1 || channel_stride < nchannels)
        return set_error(CHROMA_ERR_INVALID, "need at least one row, one channel and a channel stride of at least the number of channels");
    if ((uint64_t)nrows * channel_stride > 0xffffffffull || (uint64_t)nrows * nchannels >= 0x7fffffffull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u words: more than the scan's 31-bit count holds, pass fewer rows", nrows, channel_stride);
    const CallScope scope(ctx);
    const uint32_t nwords = nrows * nchannels, nflags = nwords + 1;
    size_t scan_bytes = 0;
    { uint32_t *nul = nullptr; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nul, nul, (int)nflags, ctx->stream)); }
    const size_t flag_bytes = round256((size_t)nflags * sizeof(uint32_t));
    int rc = steps_block(scope, flag_bytes + round256(scan_bytes)); if (rc) return rc;
    uint32_t *d_positions = (uint32_t *)scope.state().steps_scratch;          // the flags, then (in place) their exclusive sum
    void *d_scan = (char *)scope.state().steps_scratch + flag_bytes;
    const dim3 grid((nflags + 255) / 256), block(256);
    hipLaunchKernelGGL(k_daq_events_flag, grid, block, 0, ctx->stream, nwords, nchannels, channel_stride, d_channel_histories, d_positions);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_positions, d_positions, (int)nflags, ctx->stream));
    hipLaunchKernelGGL(k_daq_events_scatter, grid, block, 0, ctx->stream, nwords, nchannels, channel_stride, charge_unit,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories, d_positions, capacity, d_offsets, d_channel,
                       (uint32_t *)d_t, d_q, d_flags);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_positions + nwords, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *ntouched = total;
    if (total > capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu touched words, the state holds %u", (unsigned long long)capacity, total);
    return CHROMA_OK;
}

// ---- the time-binned DAQ (kernels_daq_pulses.h) ----
// what chroma_daq_acquire_events refuses, and the window's rules
static int check_pulses_call(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows, const uint32_t *bounds,
                             const chroma_photon_arrays *photons, uint32_t nphotons, const chroma_daq_window *window)
{
    if (!ctx || !geom || !tables || !bounds || !window) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids || !geom->view.nchannels) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (nrows < 1) return set_error(CHROMA_ERR_INVALID, "need at least one row");
    if (!(window->dt > 0.0f) || !std::isfinite(window->dt) || !std::isfinite(window->t0) || window->nbins < 1 || window->nbins > 65536)
        return set_error(CHROMA_ERR_INVALID, "DAQ window: need a finite t0, a finite positive dt and 1 .. 65536 bins");
    if ((uint64_t)nrows * geom->view.nchannels > 0x7fffffffffffffffull / window->nbins)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u channels of %u bins: more than 63-bit keys hold, pass fewer rows", nrows,
                         geom->view.nchannels, window->nbins);
    for (uint32_t r = 0; r < nrows; r++)
        if (bounds[r] > bounds[r + 1]) return set_error(CHROMA_ERR_INVALID, "event bounds: bound %u is below bound %u", r + 1, r);
    if (bounds[nrows] > nphotons || bounds[nrows] > 0x7fffffffu)
        return set_error(CHROMA_ERR_INVALID, "event bounds: the last bound %u is beyond the %u photons of the set", bounds[nrows], nphotons);
    if (tables->time_cdf_len < 2 || tables->charge_cdf_len < 2 || !tables->d_time_cdf_x || !tables->d_time_cdf_y ||
        !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need two CDFs of at least 2 points and a positive charge unit");
    return check_photons(photons, false);
}

// The pooled block of a pulses call: the bounds first, then 256 bytes of counters, then what the caller lays out.  Grows the block to
// `need` and puts the bounds there, unless this call has `placed` them already and the block need not grow.
static int pulses_block(const CallScope &scope, size_t need, uint32_t nrows, const uint32_t *bounds, bool placed)
{
    const bool keep = placed && scope.state().steps_scratch_bytes >= need;
    int rc = steps_block(scope, need); if (rc) return rc;
    if (keep) return CHROMA_OK;
    HIP_TRY(hipMemcpyAsync(scope.state().steps_scratch, bounds, ((size_t)nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, scope.ctx->stream));
    HIP_TRY(hipStreamSynchronize(scope.ctx->stream));          // (the caller's bounds are his again when the call returns)
    return CHROMA_OK;
}

// what the calls with noise refuse besides (noise NULL: nothing)
static int check_pulses_noise(const chroma_geometry *geom, uint32_t nrows, uint32_t nphotons, chroma_rng rng, const chroma_daq_noise *noise)
{
    if (!noise) return CHROMA_OK;
    if (const char *why = daq_noise::check(noise)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if ((uint64_t)nrows * geom->view.nchannels > 0xffffffffull)
        return set_error(CHROMA_ERR_INVALID, "DAQ noise: %u rows of %u channels: more than 32-bit word indices hold, pass fewer rows", nrows, geom->view.nchannels);
    const uint64_t last_id = rng.photon_id_base + (nphotons ? nphotons - 1u : 0u);
    if (nphotons && ((rng.photon_id_base >> 32) == daq_noise::ID_HIGH || (last_id >> 32) == daq_noise::ID_HIGH || last_id < rng.photon_id_base))
        return set_error(CHROMA_ERR_INVALID, "DAQ noise: the photon ids reach the high word 0xffffffff of the noise's pseudo-photons");
    return CHROMA_OK;
}

static DaqNoiseView noise_view(const chroma_daq_noise *noise)
{
    DaqNoiseView v;
    for (uint32_t j = 0; j < 64u; j++) v.count_cdf[j] = j < noise->ncount ? noise->count_cdf[j] : 0xffffffffu;
    v.ncount = noise->ncount;
    v.flag = noise->flag;
    v.accept = noise->d_accept;
    return v;
}

// The accepted in-window photons of the window (k_daq_pulses_count) and, with `noise`, the kept noise photoelectrons of the rows'
// words (k_daq_noise_count), with the bounds already in the block.  The counters: word 0 the photons, word 1 the emits' cursor,
// the 64-bit word behind them the noise.
static int pulses_count(const CallScope &scope, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows, uint32_t span,
                        uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng, uint32_t acquisition,
                        float global_weight, const chroma_daq_window *window, const chroma_daq_noise *noise, uint64_t *naccepted)
{
    hipStream_t stream = scope.ctx->stream;
    const uint32_t *d_bounds = (const uint32_t *)scope.state().steps_scratch;
    uint32_t *d_count = (uint32_t *)((char *)scope.state().steps_scratch + round256(((size_t)nrows + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(d_count, 0, 4 * sizeof(uint32_t), stream));
    if (span) {
        hipLaunchKernelGGL(k_daq_pulses_count, dim3((span + DAQ_PULSES_SPAN - 1) / DAQ_PULSES_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream, geom->view,
                           *tables, *window, nrows, d_bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                           photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, d_count);
        HIP_TRY(hipGetLastError());
    }
    if (noise) {
        const uint32_t nwords = nrows * geom->view.nchannels;
        hipLaunchKernelGGL(k_daq_noise_count, dim3((nwords + DAQ_NOISE_SPAN - 1) / DAQ_NOISE_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream,
                           noise_view(noise), geom->view.nchannels, nwords, rng.seed, acquisition, (unsigned long long *)(d_count + 2));
        HIP_TRY(hipGetLastError());
    }
    uint32_t counts[4] = {0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(counts, d_count, sizeof(counts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *naccepted = (uint64_t)counts[0] + (((uint64_t)counts[3] << 32) | counts[2]);
    return CHROMA_OK;
}

// chroma_daq_count_pulses and chroma_daq_count_pulses_noise
static int count_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows, const uint32_t *bounds,
                        uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                        uint32_t acquisition, float global_weight, const chroma_daq_window *window, const chroma_daq_noise *noise,
                        uint64_t *naccepted)
{
    if (!naccepted) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pulses_call(ctx, geom, tables, nrows, bounds, photons, nphotons, window); if (rc) return rc;
    rc = check_pulses_noise(geom, nrows, nphotons, rng, noise); if (rc) return rc;
    *naccepted = 0;
    const uint32_t span = bounds[nrows] - bounds[0];
    if (span == 0 && !noise) return CHROMA_OK;
    const CallScope scope(ctx);
    rc = pulses_block(scope, round256(((size_t)nrows + 1) * sizeof(uint32_t)) + 256, nrows, bounds, false); if (rc) return rc;
    return pulses_count(scope, geom, tables, nrows, span, detection_state, photons, rng, acquisition, global_weight, window, noise, naccepted);
}

int chroma_daq_count_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                            const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                            chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                            uint64_t *naccepted)
{
    return count_pulses(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight, window, nullptr,
                        naccepted);
}

int chroma_daq_count_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                                  const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                                  chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                  const chroma_daq_noise *noise, uint64_t *naccepted)
{
    return count_pulses(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight, window, noise,
                        naccepted);
}

// chroma_daq_acquire_pulses and chroma_daq_acquire_pulses_noise
static int acquire_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows, const uint32_t *bounds,
                          uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                          uint32_t acquisition, float global_weight, const chroma_daq_window *window, const chroma_daq_noise *noise,
                          uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel, uint32_t *d_bin, uint32_t *d_npe, uint32_t *d_q_int,
                          float *d_t_first, uint32_t *d_flags, uint32_t *d_outside, uint32_t *d_row_noise, uint64_t *npulses)
{
    if (!d_offsets || !d_outside || !npulses || (capacity && (!d_channel || !d_bin || !d_npe || !d_q_int || !d_t_first || !d_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pulses_call(ctx, geom, tables, nrows, bounds, photons, nphotons, window); if (rc) return rc;
    rc = check_pulses_noise(geom, nrows, nphotons, rng, noise); if (rc) return rc;
    *npulses = 0;
    hipStream_t stream = ctx->stream;
    const size_t offsets_bytes = ((size_t)nrows + 1) * sizeof(uint32_t), outside_bytes = 2 * (size_t)nrows * sizeof(uint32_t);
    const size_t row_noise_bytes = (size_t)nrows * sizeof(uint32_t);
    const uint32_t span = bounds[nrows] - bounds[0];
    if (span == 0 && !noise) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream));
        HIP_TRY(hipMemsetAsync(d_outside, 0, outside_bytes, stream));
        if (d_row_noise) HIP_TRY(hipMemsetAsync(d_row_noise, 0, row_noise_bytes, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return CHROMA_OK;
    }
    const CallScope scope(ctx);
    const size_t head_bytes = round256(offsets_bytes) + 256;          // the bounds and the counters (pulses_count)
    const size_t rows_bytes = round256(outside_bytes + row_noise_bytes);          // per row: early and late photons, then the noise
    rc = pulses_block(scope, head_bytes + rows_bytes, nrows, bounds, false); if (rc) return rc;
    uint64_t accepted = 0;
    rc = pulses_count(scope, geom, tables, nrows, span, detection_state, photons, rng, acquisition, global_weight, window, noise, &accepted);
    if (rc) return rc;
    if (accepted >= 0x7fffffffull)
        return set_error(CHROMA_ERR_INVALID, "%llu accepted photons and noise photoelectrons: more than the scan's 31-bit count holds, pass fewer rows",
                         (unsigned long long)accepted);
    const uint32_t n = (uint32_t)accepted;
    // the block: bounds, counters, the rows' early, late and noise counts; then, per accepted photon and noise photoelectron, the keys
    // and their positions before and behind the sort, charge count, time bits and history; the heads (n + 1); the workspaces of the
    // sort and of the scan
    const uint64_t nkeys = (uint64_t)nrows * geom->view.nchannels * window->nbins;
    int end_bit = 1;
    while (end_bit < 64 && ((nkeys - 1) >> end_bit)) end_bit++;
    size_t sort_bytes = 0, scan_bytes = 0;
    if (n) {
        uint64_t *k = nullptr; uint32_t *v = nullptr;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k, k, v, v, (int)n, 0, end_bit, stream));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, v, v, (int)(n + 1), stream));
    }
    const size_t key_bytes = round256((size_t)n * sizeof(uint64_t)), word_bytes = round256((size_t)n * sizeof(uint32_t));
    const size_t need = head_bytes + rows_bytes + 2 * key_bytes + 5 * word_bytes + round256(((size_t)n + 1) * sizeof(uint32_t)) +
                        round256(sort_bytes) + round256(scan_bytes);
    rc = pulses_block(scope, need, nrows, bounds, true); if (rc) return rc;
    char *p = (char *)scope.state().steps_scratch;
    const uint32_t *d_bounds = (const uint32_t *)p; p += round256(offsets_bytes);
    uint32_t *d_cursor = (uint32_t *)p + 1; p += 256;
    uint32_t *d_rows_outside = (uint32_t *)p, *d_rows_noise = d_rows_outside + 2 * (size_t)nrows; p += rows_bytes;
    uint64_t *d_keys = (uint64_t *)p; p += key_bytes;
    uint64_t *d_keys_sorted = (uint64_t *)p; p += key_bytes;
    uint32_t *d_order = (uint32_t *)p; p += word_bytes;
    uint32_t *d_order_sorted = (uint32_t *)p; p += word_bytes;
    uint32_t *d_charge = (uint32_t *)p; p += word_bytes;
    uint32_t *d_time = (uint32_t *)p; p += word_bytes;
    uint32_t *d_history = (uint32_t *)p; p += word_bytes;
    uint32_t *d_positions = (uint32_t *)p; p += round256(((size_t)n + 1) * sizeof(uint32_t));          // the heads, then (in place) their exclusive sum
    void *d_sort = p; p += round256(sort_bytes);
    void *d_scan = p;
    HIP_TRY(hipMemsetAsync(d_cursor, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(d_rows_outside, 0, outside_bytes + row_noise_bytes, stream));
    // both emits before the sort, onto one cursor: the photons' entries and the noise's lie among one another
    if (span) {
        hipLaunchKernelGGL(k_daq_pulses_emit, dim3((span + DAQ_PULSES_SPAN - 1) / DAQ_PULSES_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream, geom->view,
                           *tables, *window, nrows, d_bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                           photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, n, d_cursor, d_keys, d_order, d_charge,
                           d_time, d_history, d_rows_outside);
        HIP_TRY(hipGetLastError());
    }
    if (noise) {
        const uint32_t nwords = nrows * geom->view.nchannels;
        hipLaunchKernelGGL(k_daq_noise_emit, dim3((nwords + DAQ_NOISE_SPAN - 1) / DAQ_NOISE_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream,
                           noise_view(noise), *tables, *window, geom->view.nchannels, nwords, rng.seed, acquisition, n, d_cursor, d_keys, d_order,
                           d_charge, d_time, d_history, d_rows_noise);
        HIP_TRY(hipGetLastError());
    }
    uint32_t total = 0;
    if (n) {
        const dim3 grid((n + 1 + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), block(DAQ_PULSES_BLOCK);
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_sort, sort_bytes, d_keys, d_keys_sorted, d_order, d_order_sorted, (int)n, 0, end_bit, stream));
        hipLaunchKernelGGL(k_daq_pulses_heads, grid, block, 0, stream, n, d_keys_sorted, d_positions);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_positions, d_positions, (int)(n + 1), stream));
        HIP_TRY(hipMemcpyAsync(&total, d_positions + n, sizeof(total), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *npulses = total;
        if (total > capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu pulses, the rows hold %u", (unsigned long long)capacity, total);
        hipLaunchKernelGGL(k_daq_pulses_open, grid, block, 0, stream, n, geom->view.nchannels, window->nbins, d_keys_sorted, d_positions, d_channel,
                           d_bin, d_npe, d_q_int, (uint32_t *)d_t_first, d_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_reduce, dim3((n + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), dim3(DAQ_PULSES_BLOCK), 0, stream, n,
                           d_keys_sorted, d_positions, d_order_sorted, d_charge, d_time, d_history, d_npe, d_q_int, (uint32_t *)d_t_first, d_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_finish, dim3((std::max(total, nrows + 1) + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), block, 0, stream, n, total, nrows,
                           (uint64_t)geom->view.nchannels * window->nbins, d_keys_sorted, d_positions, (uint32_t *)d_t_first, d_offsets);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream));
    }
    HIP_TRY(hipMemcpyAsync(d_outside, d_rows_outside, outside_bytes, hipMemcpyDeviceToDevice, stream));
    if (d_row_noise) HIP_TRY(hipMemcpyAsync(d_row_noise, d_rows_noise, row_noise_bytes, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_daq_acquire_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                              const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                              chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                              uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel, uint32_t *d_bin, uint32_t *d_npe,
                              uint32_t *d_q_int, float *d_t_first, uint32_t *d_flags, uint32_t *d_outside, uint64_t *npulses)
{
    return acquire_pulses(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight, window, nullptr,
                          capacity, d_offsets, d_channel, d_bin, d_npe, d_q_int, d_t_first, d_flags, d_outside, nullptr, npulses);
}

int chroma_daq_acquire_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                                    const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                                    chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                    const chroma_daq_noise *noise, uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel,
                                    uint32_t *d_bin, uint32_t *d_npe, uint32_t *d_q_int, float *d_t_first, uint32_t *d_flags,
                                    uint32_t *d_outside, uint32_t *d_row_noise, uint64_t *npulses)
{
    return acquire_pulses(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight, window, noise,
                          capacity, d_offsets, d_channel, d_bin, d_npe, d_q_int, d_t_first, d_flags, d_outside, d_row_noise, npulses);
}

// ---- the trigger of the time-binned DAQ (kernels_daq_trigger.h) ----
int chroma_daq_trigger_pulses(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                              const chroma_daq_trigger *trigger, const uint32_t *d_offsets, const int32_t *d_channel, const uint32_t *d_bin,
                              const uint32_t *d_npe, const uint32_t *d_q_int, const float *d_t_first, const uint32_t *d_flags, uint64_t npulses,
                              uint64_t trigger_capacity, uint32_t *d_trig_offsets, uint32_t *d_trig_bin, uint32_t *d_trig_sum,
                              uint32_t *d_hit_offsets, uint64_t hit_capacity, int32_t *d_hit_channel, uint32_t *d_hit_npe, uint32_t *d_hit_q_int,
                              float *d_hit_t_first, uint32_t *d_hit_flags, uint32_t *d_pulse_trigger, uint64_t *ntriggers, uint64_t *nhits)
{
    if (!ctx || !window || !trigger || !d_offsets || !d_trig_offsets || !d_hit_offsets || !ntriggers || !nhits ||
        (npulses && (!d_channel || !d_bin || !d_npe || !d_q_int || !d_t_first || !d_flags)) || (trigger_capacity && (!d_trig_bin || !d_trig_sum)) ||
        (hit_capacity && (!d_hit_channel || !d_hit_npe || !d_hit_q_int || !d_hit_t_first || !d_hit_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nrows < 1 || nchannels < 1 || nchannels > 0x7fffffffu) return set_error(CHROMA_ERR_INVALID, "need at least one row and 1 .. 2^31 - 1 channels");
    if (!(window->dt > 0.0f) || !std::isfinite(window->dt) || !std::isfinite(window->t0) || window->nbins < 1 || window->nbins > 65536)
        return set_error(CHROMA_ERR_INVALID, "DAQ window: need a finite t0, a finite positive dt and 1 .. 65536 bins");
    const uint32_t nbins = window->nbins;
    if (trigger->kind != CHROMA_TRIGGER_NHIT && trigger->kind != CHROMA_TRIGGER_NPE) return set_error(CHROMA_ERR_INVALID, "DAQ trigger: unknown kind %u", trigger->kind);
    if (trigger->threshold < 1 || trigger->width < 1 || trigger->width > nbins || trigger->post < 1 ||
        trigger->holdoff < std::max<uint64_t>(1, (uint64_t)trigger->pre + trigger->post))
        return set_error(CHROMA_ERR_INVALID, "DAQ trigger: need a threshold of at least 1, a width of 1 .. %u bins, post >= 1 and holdoff >= max(1, pre + post)", nbins);
    if (npulses >= 0x7fffffffull) return set_error(CHROMA_ERR_INVALID, "%llu pulses: more than the scan's 31-bit count holds, pass fewer rows", (unsigned long long)npulses);
    if ((uint64_t)nrows * nbins >= 0x80000000ull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u bins: more than 31-bit (row, bin) indices hold, pass fewer rows", nrows, nbins);
    hipStream_t stream = ctx->stream;
    const size_t offsets_bytes = ((size_t)nrows + 1) * sizeof(uint32_t);
    if (npulses == 0) {
        *ntriggers = 0; *nhits = 0;
        HIP_TRY(hipMemsetAsync(d_trig_offsets, 0, offsets_bytes, stream));
        HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(uint32_t), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return CHROMA_OK;
    }
    // (what lies beyond the window changes nothing: a lockout, a gate or a reach of more than nbins bins is one of nbins)
    const uint32_t n = (uint32_t)npulses, holdoff = std::min(trigger->holdoff, nbins), pre = std::min(trigger->pre, nbins), post = std::min(trigger->post, nbins);
    const uint64_t per_row = (nbins + holdoff - 1) / holdoff, per_pulse = (trigger->width + holdoff - 1) / holdoff;
    const uint32_t room = (uint32_t)std::min<uint64_t>((uint64_t)nrows * per_row, (uint64_t)n * per_pulse);          // (<= nrows * nbins < 2^31)
    // The block, sized once from the bounds (growing it would lose what is in it): the sum per (row, bin); per pulse its row, its
    // trigger, the gated flags and their scan (n + 1), the keys and indices before and behind the sort, the heads (n + 1), the bin
    // that k_daq_pulses_open writes; per row the counts and their scan (nrows + 1); per trigger its bin and sum; the workspaces
    const CallScope scope(ctx);
    size_t sort_bytes = 0, scan_bytes = 0, scan_rows_bytes = 0;
    {
        uint64_t *k = nullptr; uint32_t *v = nullptr;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k, k, v, v, (int)n, 0, 64, stream));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, v, v, (int)(n + 1), stream));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_rows_bytes, v, v, (int)(nrows + 1), stream));
    }
    scan_bytes = std::max(scan_bytes, scan_rows_bytes);
    const size_t sum_bytes = round256((size_t)nrows * nbins * sizeof(uint32_t)), word_bytes = round256((size_t)n * sizeof(uint32_t)),
                 word1_bytes = round256(((size_t)n + 1) * sizeof(uint32_t)), key_bytes = round256((size_t)n * sizeof(uint64_t)),
                 trig_bytes = round256((size_t)room * sizeof(uint32_t));
    const size_t need = sum_bytes + 5 * word_bytes + 2 * word1_bytes + 2 * key_bytes + round256(offsets_bytes) + 2 * trig_bytes + round256(sort_bytes) +
                        round256(scan_bytes);
    int rc = steps_block(scope, need); if (rc) return rc;
    char *p = (char *)scope.state().steps_scratch;
    uint32_t *d_sum = (uint32_t *)p; p += sum_bytes;
    uint32_t *d_rows = (uint32_t *)p; p += word_bytes;
    uint32_t *d_of = (uint32_t *)p; p += word_bytes;          // the trigger of every pulse
    uint32_t *d_order = (uint32_t *)p; p += word_bytes;
    uint32_t *d_order_sorted = (uint32_t *)p; p += word_bytes;
    uint32_t *d_hit_bin = (uint32_t *)p; p += word_bytes;
    uint32_t *d_gated = (uint32_t *)p; p += word1_bytes;          // the flags, then (in place) their exclusive sum
    uint32_t *d_positions = (uint32_t *)p; p += word1_bytes;          // the heads, then (in place) their exclusive sum
    uint64_t *d_keys = (uint64_t *)p; p += key_bytes;
    uint64_t *d_keys_sorted = (uint64_t *)p; p += key_bytes;
    uint32_t *d_row_triggers = (uint32_t *)p; p += round256(offsets_bytes);          // the counts, then (in place) the rows' offsets
    uint32_t *d_bins = (uint32_t *)p; p += trig_bytes;
    uint32_t *d_sums = (uint32_t *)p; p += trig_bytes;
    void *d_sort = p; p += round256(sort_bytes);
    void *d_scan = p;
    const dim3 block(DAQ_TRIGGER_BLOCK), per_pulse_grid((n + DAQ_TRIGGER_BLOCK - 1) / DAQ_TRIGGER_BLOCK), per_pulse1_grid(n / DAQ_TRIGGER_BLOCK + 1);
    HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)nrows * nbins * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_daq_trigger_edges, per_pulse_grid, block, 0, stream, n, nrows, nchannels, nbins, trigger->kind, trigger->width, d_offsets, d_channel,
                       d_bin, d_npe, d_rows, d_sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_daq_trigger_count, dim3(nrows / DAQ_TRIGGER_WAVES + 1), block, 0, stream, nrows, nbins, trigger->threshold, holdoff, d_sum, d_row_triggers);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_row_triggers, d_row_triggers, (int)(nrows + 1), stream));
    uint32_t total = 0, ngated = 0, total_hits = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_row_triggers + nrows, sizeof(total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total > room) return set_error(CHROMA_ERR_INTERNAL, "DAQ trigger: %u firings, the bound is %u", total, room);
    int end_bit = 1;
    if (total) {
        hipLaunchKernelGGL(k_daq_trigger_fire, dim3((nrows + DAQ_TRIGGER_WAVES - 1) / DAQ_TRIGGER_WAVES), block, 0, stream, nrows, nbins, trigger->threshold,
                           holdoff, d_sum, d_row_triggers, room, d_bins, d_sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_trigger_gates, per_pulse1_grid, block, 0, stream, n, pre, post, d_rows, d_bin, d_row_triggers, d_bins, d_of, d_gated);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_gated, d_gated, (int)(n + 1), stream));
        hipLaunchKernelGGL(k_daq_trigger_compact, per_pulse_grid, block, 0, stream, n, nchannels, d_of, d_channel, d_gated, n, d_keys, d_order);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ngated, d_gated + n, sizeof(ngated), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ngated) {
        const uint64_t nkeys = (uint64_t)total * nchannels;
        while (end_bit < 64 && ((nkeys - 1) >> end_bit)) end_bit++;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_sort, sort_bytes, d_keys, d_keys_sorted, d_order, d_order_sorted, (int)ngated, 0, end_bit, stream));
        hipLaunchKernelGGL(k_daq_pulses_heads, dim3(ngated / DAQ_PULSES_BLOCK + 1), dim3(DAQ_PULSES_BLOCK), 0, stream, ngated, d_keys_sorted, d_positions);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_positions, d_positions, (int)(ngated + 1), stream));
        HIP_TRY(hipMemcpyAsync(&total_hits, d_positions + ngated, sizeof(total_hits), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *ntriggers = total; *nhits = total_hits;
    if (total > trigger_capacity || total_hits > hit_capacity)
        return set_error(CHROMA_ERR_INVALID, "room for %llu triggers and %llu hits, the rows hold %u and %u", (unsigned long long)trigger_capacity,
                         (unsigned long long)hit_capacity, total, total_hits);
    // nothing of the caller's was written so far
    HIP_TRY(hipMemcpyAsync(d_trig_offsets, d_row_triggers, offsets_bytes, hipMemcpyDeviceToDevice, stream));
    if (total) {
        HIP_TRY(hipMemcpyAsync(d_trig_bin, d_bins, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_trig_sum, d_sums, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
    if (d_pulse_trigger) {
        if (total) { HIP_TRY(hipMemcpyAsync(d_pulse_trigger, d_of, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream)); }
        else { HIP_TRY(hipMemsetAsync(d_pulse_trigger, 0xff, (size_t)n * sizeof(uint32_t), stream)); }
    }
    if (ngated) {
        const dim3 pulses_block(DAQ_PULSES_BLOCK);
        hipLaunchKernelGGL(k_daq_pulses_open, dim3((ngated + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), pulses_block, 0, stream, ngated, nchannels, 1u,
                           d_keys_sorted, d_positions, d_hit_channel, d_hit_bin, d_hit_npe, d_hit_q_int, (uint32_t *)d_hit_t_first, d_hit_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_trigger_reduce, dim3((ngated + DAQ_TRIGGER_BLOCK - 1) / DAQ_TRIGGER_BLOCK), block, 0, stream, ngated, d_keys_sorted,
                           d_positions, d_order_sorted, d_npe, d_q_int, (const uint32_t *)d_t_first, d_flags, d_hit_npe, d_hit_q_int,
                           (uint32_t *)d_hit_t_first, d_hit_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_finish, dim3(std::max(total_hits, total + 1) / DAQ_PULSES_BLOCK + 1), pulses_block, 0, stream, ngated, total_hits,
                           total, (uint64_t)nchannels, d_keys_sorted, d_positions, (uint32_t *)d_hit_t_first, d_hit_offsets);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, ((size_t)total + 1) * sizeof(uint32_t), stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_daq_convert(chroma_ctx *ctx, uint32_t nchannels, float charge_unit, const uint32_t *d_earliest_time_int,
                       const uint32_t *d_channel_q_int, float *d_earliest_time, float *d_channel_q)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_earliest_time || !d_channel_q)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nchannels == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_daq_convert, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, charge_unit,
                       d_earliest_time_int, d_channel_q_int, d_earliest_time, d_channel_q);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// ---- PDFs over DAQ output (kernels_pdf.h) ----
static int check_pdf_layout(uint32_t nchannels, int32_t ndaq, uint32_t stride)
{
    if (ndaq < 1 || stride < nchannels)
        return set_error(CHROMA_ERR_INVALID, "ndaq must be positive and the channel stride at least the number of channels");
    return CHROMA_OK;
}

int chroma_pdf_bin_hits(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride, const float *d_channel_q,
                        const float *d_channel_t, int32_t tbins, float tmin, float tmax, int32_t qbins, float qmin, float qmax,
                        uint32_t *d_hitcount, uint32_t *d_pdf)
{
    if (!ctx || !d_channel_q || !d_channel_t || !d_hitcount || !d_pdf) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (tbins < 1 || qbins < 1 || (int64_t)tbins * qbins > INT32_MAX)
        return set_error(CHROMA_ERR_INVALID, "need at least one time and one charge bin (and fewer than 2^31 per channel)");
    if (!(tmin < tmax) || !(qmin < qmax)) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_bin_hits, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, (int)ndaq, stride,
                       d_channel_q, d_channel_t, d_hitcount, (int)tbins, tmin, tmax, (int)qbins, qmin, qmax, d_pdf);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_eval_accumulate(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride, const uint32_t *d_event_hit,
                               const float *d_event_time, const float *d_mc_time, uint32_t nhit, const uint32_t *d_hit_channels,
                               float min_twidth, float tmin, float tmax, int32_t min_bin_content, uint32_t *d_hitcount,
                               uint32_t *d_bincount, float *d_nearest)
{
    if (!ctx || !d_event_hit || !d_event_time || !d_mc_time || !d_hitcount || !d_bincount || (nhit && (!d_hit_channels || !d_nearest)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (min_bin_content < 1 || min_bin_content > 1024) return set_error(CHROMA_ERR_INVALID, "min_bin_content must be in 1 .. 1024");
    if (!(tmin < tmax)) return set_error(CHROMA_ERR_INVALID, "empty or inverted time range");
    if (nhit > nchannels) return set_error(CHROMA_ERR_INVALID, "more hit channels than channels");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_eval_hitcount, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, (int)ndaq, stride,
                       d_event_hit, d_mc_time, tmin, tmax, d_hitcount);
    HIP_TRY(hipGetLastError());
    if (nhit == 0) return CHROMA_OK;          // an event with no hit channel: nothing to sort
    hipLaunchKernelGGL(k_pdf_eval_accumulate, dim3((nhit + PDF_EVAL_WAVES - 1) / PDF_EVAL_WAVES), dim3(64 * PDF_EVAL_WAVES), 0,
                       ctx->stream, nchannels, (int)ndaq, stride, nhit, d_hit_channels, d_event_hit, d_event_time, d_mc_time,
                       0.5f * min_twidth, tmin, tmax, (int)min_bin_content, d_hitcount, d_bincount, d_nearest);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_moments(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride, const float *d_mc_time,
                       const float *d_mc_charge, float tmin, float tmax, float qmin, float qmax, uint32_t *d_mom0, float *d_t_mom1,
                       float *d_t_mom2, float *d_q_mom1, float *d_q_mom2)
{
    if (!ctx || !d_mc_time || !d_mom0 || !d_t_mom1 || !d_t_mom2 || (!time_only && (!d_mc_charge || !d_q_mom1 || !d_q_mom2)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (!(tmin < tmax) || (!time_only && !(qmin < qmax))) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_moments, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, (int)(time_only != 0), nchannels,
                       (int)ndaq, stride, d_mc_time, d_mc_charge, tmin, tmax, qmin, qmax, d_mom0, d_t_mom1, d_t_mom2, d_q_mom1, d_q_mom2);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_kernel_eval(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                           const uint32_t *d_event_hit, const float *d_event_time, const float *d_event_charge, const float *d_mc_time,
                           const float *d_mc_charge, float tmin, float tmax, float qmin, float qmax, const float *d_inv_time_bandwidths,
                           const float *d_inv_charge_bandwidths, uint32_t *d_hitcount, float *d_time_pdf_values,
                           float *d_charge_pdf_values)
{
    if (!ctx || !d_event_hit || !d_event_time || !d_mc_time || !d_inv_time_bandwidths || !d_hitcount || !d_time_pdf_values ||
        (!time_only && (!d_event_charge || !d_mc_charge || !d_inv_charge_bandwidths || !d_charge_pdf_values)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (!(tmin < tmax) || (!time_only && !(qmin < qmax))) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_kernel_eval, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, (int)(time_only != 0), nchannels,
                       (int)ndaq, stride, d_event_hit, d_event_time, d_event_charge, d_mc_time, d_mc_charge, tmin, tmax, qmin, qmax,
                       d_inv_time_bandwidths, d_inv_charge_bandwidths, d_hitcount, d_time_pdf_values, d_charge_pdf_values);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_render(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const float *d_origin, const float *d_direction,
                  uint32_t alpha_depth, uint32_t *d_pixels, float *d_dx, uint32_t *d_dxlen, float *d_color, uint32_t bg_color)
{
    if (!ctx || !geom || !d_origin || !d_direction || !d_pixels || !d_dx || !d_dxlen || !d_color)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (alpha_depth < 1) return set_error(CHROMA_ERR_INVALID, "alpha_depth must be at least 1");
    if (nthreads <= 0) return CHROMA_OK;
    if (geom->stack_need > STACK_LDS + STACK_SCRATCH)
        return set_error(CHROMA_ERR_STACK, "BVH needs %u traversal stack entries, more than the %d supported", geom->stack_need, STACK_LDS + STACK_SCRATCH);
    const CallScope scope(ctx);          // (the render counts stack overflows into the context's counters)
    hipLaunchKernelGGL((k_render<STACK_LDS>), dim3((unsigned)((nthreads + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, ctx->stream,
                       geom->view, (const uint32_t *)geom->d_colors, (int)nthreads, d_origin, d_direction, alpha_depth, d_pixels, d_dx,
                       d_dxlen, (float4 *)d_color, bg_color, scope.state().d_counters);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_color_solids(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_triangle, int32_t ntriangles, const uint8_t *d_solid_hit,
                        const uint32_t *d_solid_colors, uint32_t nsolids)
{
    if (!ctx || !geom || !d_solid_hit || !d_solid_colors) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->d_colors || !geom->view.solid_id_map) return set_error(CHROMA_ERR_INVALID, "geometry was created without colors / solid_id_map");
    if (first_triangle < 0 || ntriangles < 0 || (uint64_t)first_triangle + (uint64_t)ntriangles > (uint64_t)geom->ntriangles)
        return set_error(CHROMA_ERR_INVALID, "triangles %d .. %lld of %llu", first_triangle, (long long)first_triangle + ntriangles, (unsigned long long)geom->ntriangles);
    if (ntriangles == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_color_solids, dim3((unsigned)((ntriangles + 255) / 256)), dim3(256), 0, ctx->stream, (int)first_triangle, (int)ntriangles,
                       geom->view.solid_id_map, d_solid_hit, d_solid_colors, nsolids, (uint32_t *)geom->d_colors);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

static int rays_transform(chroma_ctx *ctx, int32_t n, float *d_a, int mode, float phi, const float axis[3], const float point[3])
{
    if (!ctx || !d_a) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (n <= 0) return CHROMA_OK;
    const float zero[3] = {0.f, 0.f, 0.f};
    if (!axis) axis = zero;
    if (!point) point = zero;
    hipLaunchKernelGGL(k_rays_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, d_a, mode, phi,
                       axis[0], axis[1], axis[2], point[0], point[1], point[2]);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}
int chroma_points_translate(chroma_ctx *ctx, int32_t n, float *d_a, const float v[3]) { return rays_transform(ctx, n, d_a, 0, 0.f, nullptr, v); }
int chroma_points_rotate(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3]) { return rays_transform(ctx, n, d_a, 1, phi, axis, nullptr); }
int chroma_points_rotate_around_point(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3], const float point[3])
{ return rays_transform(ctx, n, d_a, 2, phi, axis, point); }

int chroma_probe(chroma_ctx *ctx, int32_t fn, uint64_t n, const float *d_x, const float *d_tab_x, const float *d_tab_f,
                 uint32_t ntab, float start, float step, float *d_out)
{
    if (!ctx || !d_x || !d_out || fn < 0 || fn > 4) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if ((fn == 0 && (!d_tab_f || ntab < 2)) || (fn == 1 && (!d_tab_x || ntab < 2)) || (fn == 2 && (!d_tab_x || !d_tab_f || ntab < 2)))
        return set_error(CHROMA_ERR_INVALID, "probe %d: table missing", fn);
    if (n == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)fn, n, d_x, d_tab_x, d_tab_f,
                       ntab, start, step, d_out);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_generate_bomb(chroma_ctx *ctx, const chroma_photon_arrays *photons, uint64_t nphotons, uint64_t seed,
                         uint64_t id_base, const float pos[3], float wavelength_lo, float wavelength_hi)
{
    if (!ctx || !pos) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(photons, true); if (rc) return rc;
    if (nphotons == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_generate_bomb, dim3((unsigned)((nphotons + 255) / 256)), dim3(256), 0, ctx->stream, to_view(photons),
                       (uint64_t)nphotons, seed, id_base, pos[0], pos[1], pos[2], wavelength_lo, wavelength_hi);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// ---- an exclusive sum in place for the other translation units (chroma_propagate_tracks: rows per photon -> offsets) ----
// Scratch from the context's pool, freed behind the stream's work.
int chroma_internal_exclusive_sum(chroma_ctx *ctx, uint32_t *d_counts, uint32_t n)
{
    if (n == 0) return CHROMA_OK;
    if (n >= 0x7fffffffu) return set_error(CHROMA_ERR_INVALID, "exclusive_sum: bad argument");
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_counts, d_counts, (int)n, ctx->stream));
    void *tmp = nullptr;
    int rc = chroma_malloc(ctx, std::max<size_t>(tmp_bytes, 4), &tmp);
    if (rc != CHROMA_OK) return rc;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_counts, d_counts, (int)n, ctx->stream);
    chroma_free(ctx, tmp);                 // (parked behind the scan)
    if (e != hipSuccess) return set_error((int)e, "exclusive_sum: %s", hipGetErrorString(e));
    return CHROMA_OK;
}

}  // extern "C"
