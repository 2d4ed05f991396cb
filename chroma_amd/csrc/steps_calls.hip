// steps_calls.hip -- photons from particle steps (kernels_steps.h): the device-resident light media and the count and generate calls,
// for one source or a medium per segment.  A count call is a pipeline -- the count kernel, an exclusive sum, the total read back --
// on the context's pooled scratch block.
#include <stdint.h>
#include <algorithm>

#include "chroma_internal.h"
#include "propagate_device.h"

#include "kernels_steps.h"
#include "kernels_particles.h"

// The calls' share of the context's scratch block, in this order: the 64-bit total, the source's three tables (the calls with a
// medium per segment have theirs in the chroma_light_media: `src` NULL, no tables), the 2 n + 1 counts, the scan's workspace.
struct StepsScratch {
    unsigned long long *total; float *refractive_index, *scintillation_cdf, *time_cdf; uint32_t *counts; void *scan; size_t scan_bytes;

    void lay(Carver &c, const chroma_light_source *src, size_t ncounts)
    {
        total = c.take<unsigned long long>(1);
        refractive_index = scintillation_cdf = time_cdf = nullptr;
        if (src) {          // (a table the source does not have: its room stays for the wavelengths', none for the times', and no pointer)
            refractive_index = c.take<float>(src->wavelength_n);
            float *scint = c.take<float>(src->wavelength_n), *time = c.take<float>(src->time_cdf ? src->time_n : 0);
            scintillation_cdf = src->scintillation_cdf ? scint : nullptr;
            time_cdf = src->time_cdf ? time : nullptr;
        }
        counts = c.take<uint32_t>(ncounts);
        scan = c.take<char>(scan_bytes);
    }
};
// A call grows the block when it has to and copies the source's tables up (they are host arrays of the caller's).
static int steps_scratch(const CallScope &scope, const chroma_light_source *src, uint64_t nsegments, StepsScratch *out)
{
    hipStream_t stream = scope.ctx->stream;
    const size_t ncounts = 2 * (size_t)nsegments + 1;
    int rc = scan_workspace_bytes(ncounts, stream, &out->scan_bytes); if (rc) return rc;
    rc = carve_call_scratch(scope, [&](Carver &c) { out->lay(c, src, ncounts); }); if (rc) return rc;
    if (!src) return CHROMA_OK;
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
struct MediaBlock {
    float *refractive_index, *scintillation_cdf, *time_cdf, *light_yield, *n_max; uint8_t *prompt;

    void lay(Carver &c, const chroma_light_media_desc &d)
    {
        const size_t nm = d.nmedia;
        refractive_index = c.take<float>(nm * d.wavelength_n); scintillation_cdf = c.take<float>(nm * d.wavelength_n);
        time_cdf = c.take<float>(nm * std::max<size_t>(d.time_n, 1));
        light_yield = c.take<float>(nm); n_max = c.take<float>(nm);
        prompt = c.take<uint8_t>(nm * sizeof(float));          // (a byte per medium, in the room of a word per medium)
    }
};
static int check_media_call(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs, const int32_t *d_medium)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (media->ctx != ctx) return set_error(CHROMA_ERR_INVALID, "light media: made on another context");
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (segs->n && !d_medium) return set_error(CHROMA_ERR_INVALID, "segments: no medium array");
    return CHROMA_OK;
}

// chroma_steps_count and chroma_steps_count_media behind their checks: the block (`src` NULL: a medium per segment), the count
// kernel that `launch` runs on it, the exclusive sum into the caller's offsets, the 64-bit total read back
template <class Launch>
static int steps_count(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint32_t *d_offsets, uint64_t *total,
                       Launch &&launch)
{
    const CallScope scope(ctx);
    *total = 0;
    if (segs->n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), ctx->stream));
        return CHROMA_OK;
    }
    StepsScratch sc;
    int rc = steps_scratch(scope, src, segs->n, &sc); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(sc.total, 0, sizeof(unsigned long long), ctx->stream));
    launch(dim3((unsigned)((segs->n + STEPS_BLOCK - 1) / STEPS_BLOCK)), sc);
    HIP_TRY(hipGetLastError());
    rc = exclusive_sum(sc.scan, sc.scan_bytes, sc.counts, d_offsets, 2 * segs->n + 1, ctx->stream); if (rc) return rc;
    unsigned long long sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, sc.total, sizeof(sum), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *total = sum;
    if (sum > 0xffffffffull) return set_error(CHROMA_ERR_INVALID, "%llu photons in one call: more than 32-bit offsets hold, pass fewer segments", sum);
    return CHROMA_OK;
}

// chroma_steps_generate and chroma_steps_generate_media behind their checks: the total the count call left behind the offsets
// against the room, then the generate kernel, which `launch` runs over that many photons (and says what kept it from it)
template <class Launch>
static int steps_generate(chroma_ctx *ctx, const chroma_step_segments *segs, const uint32_t *d_offsets, const chroma_photon_arrays *photons,
                          uint64_t capacity, Launch &&launch)
{
    if (segs->n == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_offsets + 2 * segs->n, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu photons, the segments emit %u", (unsigned long long)capacity, total);
    if (total == 0) return CHROMA_OK;
    int rc = check_photons(photons, true); if (rc) return rc;
    rc = launch(scope, dim3((total + STEPS_BLOCK - 1) / STEPS_BLOCK), total); if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

extern "C" {

int chroma_light_media_create(chroma_ctx *ctx, const chroma_light_media_desc *desc, chroma_light_media **media)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *media = nullptr;
    if (const char *why = steps::check_media(desc)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const size_t nm = desc->nmedia;
    MediaBlock b;
    Carver size, carver;
    b.lay(size, *desc);
    void *block = nullptr;
    int rc = chroma_malloc(ctx, size.offset, &block); if (rc) return rc;
    carver.base = (char *)block;
    b.lay(carver, *desc);
    float *const ri = b.refractive_index, *const scint = b.scintillation_cdf, *const tcdf = b.time_cdf;
    // one row at a time for the CDFs: a row that is ignored need not be readable, and is left as zeros
    std::vector<float> h_n_max(nm);
    steps::media_n_max(*desc, h_n_max.data());
    hipStream_t stream = ctx->stream;
    hipError_t e = hipMemsetAsync(scint, 0, (char *)b.light_yield - (char *)scint, stream);          // (both CDFs, the rounding behind them included)
    if (e == hipSuccess) e = hipMemcpyAsync(ri, desc->refractive_index, nm * desc->wavelength_n * sizeof(float), hipMemcpyHostToDevice, stream);
    for (size_t m = 0; m < nm && e == hipSuccess; m++) {
        if (desc->light_yield[m] == 0.0f) continue;
        e = hipMemcpyAsync(scint + m * desc->wavelength_n, desc->scintillation_cdf + m * desc->wavelength_n, desc->wavelength_n * sizeof(float),
                           hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !desc->prompt[m])
            e = hipMemcpyAsync(tcdf + m * desc->time_n, desc->time_cdf + m * desc->time_n, desc->time_n * sizeof(float), hipMemcpyHostToDevice, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(b.light_yield, desc->light_yield, nm * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.n_max, h_n_max.data(), nm * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.prompt, desc->prompt, nm, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);          // (the caller's tables are his again when the call returns)
    if (e != hipSuccess) {
        chroma_free(ctx, block);
        return set_error((int)e, "light media: upload failed: %s", hipGetErrorString(e));
    }
    *media = new chroma_light_media{ctx, block, steps::make_media(*desc, ri, scint, tcdf, b.light_yield, b.prompt, b.n_max)};
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
    return steps_count(ctx, nullptr, segs, d_offsets, total, [&](dim3 grid, const StepsScratch &sc) {
        hipLaunchKernelGGL(k_steps_count_media, grid, dim3(STEPS_BLOCK), 0, ctx->stream, media->view, *segs, d_medium, seed, sc.counts, sc.total);
    });
}

int chroma_steps_generate_media(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs, const int32_t *d_medium,
                                uint64_t seed, const uint32_t *d_offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (!d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_media_call(ctx, media, segs, d_medium); if (rc) return rc;
    return steps_generate(ctx, segs, d_offsets, photons, capacity, [&](const CallScope &, dim3 grid, uint32_t total) {
        hipLaunchKernelGGL(k_steps_generate_media, grid, dim3(STEPS_BLOCK), 0, ctx->stream, media->view, *segs, d_medium, seed, d_offsets,
                           to_view(photons), total);
        return CHROMA_OK;
    });
}

int chroma_steps_count(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                       uint32_t *d_offsets, uint64_t *total)
{
    if (!ctx || !d_offsets || !total) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = steps::check_source(src)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    return steps_count(ctx, src, segs, d_offsets, total, [&](dim3 grid, const StepsScratch &sc) {
        const steps::Source s = steps::make_source(*src, sc.refractive_index, sc.scintillation_cdf, sc.time_cdf);
        hipLaunchKernelGGL(k_steps_count, grid, dim3(STEPS_BLOCK), 0, ctx->stream, s, *segs, seed, sc.counts, sc.total);
    });
}

int chroma_steps_generate(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                          const uint32_t *d_offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (!ctx || !d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = steps::check_source(src)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (const char *why = steps::check_segments(segs)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    return steps_generate(ctx, segs, d_offsets, photons, capacity, [&](const CallScope &scope, dim3 grid, uint32_t total) {
        StepsScratch sc;          // (the source's tables, copied up again: the count call's may be gone)
        const int rc = steps_scratch(scope, src, segs->n, &sc); if (rc) return rc;
        const steps::Source s = steps::make_source(*src, sc.refractive_index, sc.scintillation_cdf, sc.time_cdf);
        hipLaunchKernelGGL(k_steps_generate, grid, dim3(STEPS_BLOCK), 0, ctx->stream, s, *segs, seed, d_offsets, to_view(photons), total);
        return CHROMA_OK;
    });
}

}  // extern "C"

// ---- charged particles stepped through the detector (kernels_particles.h) ----
// The device-resident table of chroma_stopping_media_create: ONE block of the context's pool, the stopping powers first, then
// the radiation lengths and the Birks constants.  Never written after it is made.
struct chroma_stopping_media {
    chroma_ctx *ctx;
    void *block;
    particles::Table view;
};
struct StoppingBlock {
    float *stopping_power, *radiation_length, *birks;

    void lay(Carver &c, const chroma_stopping_media_desc &d)
    {
        stopping_power = c.take<float>((size_t)d.nmedia * particles::NSPECIES * d.nke);
        radiation_length = c.take<float>(d.nmedia); birks = c.take<float>(d.nmedia);
    }
};

// chroma_particles_track's share of the context's scratch block, in this order: the matrix of step points (what the points and
// segments calls find again: the same n and max_steps lay the same block), the two queues (n + 1 words: the tail, then the
// ids), the live particles' rays and casts, the 64-bit total, the counts, the segments' offsets and the scan's workspace
struct ParticlesBlock {
    chroma_particle_points matrix;
    uint32_t *queue_a, *queue_b; float *origin, *direction, *distance; int32_t *last_hit, *triangle, *medium;
    unsigned long long *total; uint32_t *counts, *offsets; void *scan; size_t scan_bytes;

    void lay(Carver &c, size_t n, size_t max_steps)
    {
        const size_t rows = n * (max_steps + 1);
        matrix.pos = c.take<float>(3 * rows); matrix.t = c.take<float>(rows); matrix.dir = c.take<float>(3 * rows);
        matrix.ke = c.take<float>(rows); matrix.edep = c.take<float>(rows); matrix.qedep = c.take<float>(rows); matrix.medium = c.take<int32_t>(rows);
        queue_a = c.take<uint32_t>(n + 1); queue_b = c.take<uint32_t>(n + 1);
        origin = c.take<float>(3 * n); direction = c.take<float>(3 * n); distance = c.take<float>(n);
        last_hit = c.take<int32_t>(n); triangle = c.take<int32_t>(n); medium = c.take<int32_t>(n);
        total = c.take<unsigned long long>(1);
        counts = c.take<uint32_t>(n + 1); offsets = c.take<uint32_t>(n + 1);
        scan = c.take<char>(scan_bytes);
    }
};
static unsigned particle_blocks(uint64_t n) { return (unsigned)((n + PARTICLES_BLOCK - 1) / PARTICLES_BLOCK); }

static int check_particles_call(chroma_ctx *ctx, const chroma_stopping_media *media, const chroma_particle_arrays *p, const chroma_particle_options *o)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (media->ctx != ctx) return set_error(CHROMA_ERR_INVALID, "stopping media: made on another context");
    if (const char *why = particles::check_particles(p)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (const char *why = particles::check_options(o)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    return CHROMA_OK;
}

// The block of the last chroma_particles_track, laid again for the points and segments calls; refuses when there is none or
// when the context's scratch block is another one by now
static int particles_block_again(const CallScope &scope, ParticlesBlock *b)
{
    CallState &cs = scope.state();
    if (!cs.particles_have) return set_error(CHROMA_ERR_INVALID, "particles: no chroma_particles_track on this context before");
    if (cs.particles_run.n == 0) return CHROMA_OK;
    if (cs.call_scratch != cs.particles_block || cs.call_scratch_bytes != cs.particles_block_bytes)
        return set_error(CHROMA_ERR_INVALID, "particles: the points of the last chroma_particles_track are gone, another call has taken the context's scratch");
    int rc = scan_workspace_bytes((size_t)cs.particles_run.n + 1, scope.ctx->stream, &b->scan_bytes); if (rc) return rc;
    Carver c{(char *)cs.call_scratch};
    b->lay(c, (size_t)cs.particles_run.n, (size_t)cs.particles_max_steps);
    if (c.offset > cs.call_scratch_bytes) return set_error(CHROMA_ERR_INTERNAL, "particles: the block of the last track is too small");
    return CHROMA_OK;
}
// the counts of the run's particles (less 0: points, 1: segments) into b.counts and their 64-bit sum
static int particles_counts(const CallScope &scope, const ParticlesBlock &b, uint32_t less, uint64_t *total)
{
    const CallState &cs = scope.state();
    hipStream_t stream = scope.ctx->stream;
    HIP_TRY(hipMemsetAsync(b.total, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_particles_counts, dim3(particle_blocks(cs.particles_run.n + 1)), dim3(PARTICLES_BLOCK), 0, stream, cs.particles_run,
                       (uint32_t)cs.particles_max_steps, less, b.counts, b.total);
    HIP_TRY(hipGetLastError());
    unsigned long long sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, b.total, sizeof(sum), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *total = sum;
    return CHROMA_OK;
}

extern "C" {

int chroma_stopping_media_create(chroma_ctx *ctx, const chroma_stopping_media_desc *desc, chroma_stopping_media **media)
{
    if (!ctx || !media) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *media = nullptr;
    if (const char *why = particles::check_table(desc)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    StoppingBlock b;
    Carver size, carver;
    b.lay(size, *desc);
    void *block = nullptr;
    int rc = chroma_malloc(ctx, size.offset, &block); if (rc) return rc;
    carver.base = (char *)block;
    b.lay(carver, *desc);
    hipStream_t stream = ctx->stream;
    hipError_t e = hipMemcpyAsync(b.stopping_power, desc->stopping_power, (size_t)desc->nmedia * particles::NSPECIES * desc->nke * sizeof(float),
                                  hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.radiation_length, desc->radiation_length, desc->nmedia * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b.birks, desc->birks, desc->nmedia * sizeof(float), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);          // (the caller's tables are his again when the call returns)
    if (e != hipSuccess) {
        chroma_free(ctx, block);
        return set_error((int)e, "stopping media: upload failed: %s", hipGetErrorString(e));
    }
    *media = new chroma_stopping_media{ctx, block, particles::make_table(*desc, b.stopping_power, b.radiation_length, b.birks)};
    return CHROMA_OK;
}

int chroma_stopping_media_destroy(chroma_stopping_media *media)
{
    if (!media) return CHROMA_OK;
    const int rc = chroma_free(media->ctx, media->block);
    delete media;
    return rc;
}

int chroma_particles_advance(chroma_ctx *ctx, const chroma_stopping_media *media, const chroma_particle_arrays *p, const chroma_particle_options *options,
                             uint64_t seed, const float *d_distance, const int32_t *d_triangle, const int32_t *d_medium,
                             const chroma_particle_points *points)
{
    int rc = check_particles_call(ctx, media, p, options); if (rc) return rc;
    if (p->n == 0) return CHROMA_OK;
    if (const char *why = particles::check_points(points)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const CallScope scope(ctx);
    hipLaunchKernelGGL(k_particles_advance, dim3(particle_blocks(p->n)), dim3(PARTICLES_BLOCK), 0, ctx->stream, media->view, *options, seed, *p,
                       (const uint32_t *)nullptr, (uint32_t)p->n, d_distance, d_triangle, d_medium, *points, (uint32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_particles_track(chroma_ctx *ctx, chroma_geometry *geom, const chroma_stopping_media *media, const chroma_particle_arrays *p,
                           const chroma_particle_options *options, uint64_t seed, uint64_t *total_points)
{
    if (!total_points) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *total_points = 0;
    int rc = check_particles_call(ctx, media, p, options); if (rc) return rc;
    if (geom && geom->ctx != ctx) return set_error(CHROMA_ERR_INVALID, "geometry: made on another context");
    const size_t n = (size_t)p->n, max_steps = (size_t)options->max_steps;
    if (n * (max_steps + 1) > 0x7fffffffull)
        return set_error(CHROMA_ERR_INVALID, "particles: %zu particles of up to %zu points are more than 2^31 rows, pass fewer particles or steps", n, max_steps + 1);
    const CallScope scope(ctx);
    CallState &cs = scope.state();
    hipStream_t stream = ctx->stream;
    cs.particles_have = false;
    if (n == 0) {
        cs.particles_run = *p; cs.particles_max_steps = options->max_steps; cs.particles_have = true;
        return CHROMA_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    ParticlesBlock b;
    rc = scan_workspace_bytes(n + 1, stream, &b.scan_bytes); if (rc) return rc;
    rc = carve_call_scratch(scope, [&](Carver &c) { b.lay(c, n, max_steps); });
    if (rc) {
        Carver size;
        b.lay(size, n, max_steps);
        return set_error(CHROMA_ERR_INVALID, "particles: no room for the step points of %zu particles x %zu steps (%zu bytes), pass fewer particles or steps",
                         n, max_steps, size.offset);
    }
    const uint32_t *queue = nullptr;          // (the first iteration takes the particles as they stand)
    uint32_t *next = b.queue_a;
    long long nlive = (long long)n;
    for (size_t iteration = 0; nlive > 0; iteration++) {
        if (iteration > max_steps) return set_error(CHROMA_ERR_INTERNAL, "particles: %lld still alive after %zu iterations", nlive, iteration);
        const dim3 grid(particle_blocks((uint64_t)nlive)), block(PARTICLES_BLOCK);
        if (geom) {
            hipLaunchKernelGGL(k_particles_rays, grid, block, 0, stream, *p, queue, (uint32_t)nlive, b.origin, b.direction, b.last_hit);
            HIP_TRY(hipGetLastError());
            rc = intersect_mesh_in_scope(scope, geom, (int32_t)nlive, b.origin, b.direction, b.last_hit, b.distance, b.triangle); if (rc) return rc;
            hipLaunchKernelGGL(k_particles_medium, grid, block, 0, stream, geom->view, (uint32_t)nlive, b.triangle, b.direction, options->outside, b.medium);
        }
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)next, 1, 1, stream));          // (an empty queue: the tail alone)
        hipLaunchKernelGGL(k_particles_advance, grid, block, 0, stream, media->view, *options, seed, *p, queue, (uint32_t)nlive,
                           geom ? b.distance : nullptr, geom ? b.triangle : nullptr, geom ? b.medium : nullptr, b.matrix, next);
        HIP_TRY(hipGetLastError());
        rc = scope.read_survivors(next, &nlive); if (rc) return rc;
        queue = next;
        next = (next == b.queue_a) ? b.queue_b : b.queue_a;
    }
    cs.particles_run = *p; cs.particles_max_steps = options->max_steps;
    cs.particles_block = cs.call_scratch; cs.particles_block_bytes = cs.call_scratch_bytes;
    cs.particles_have = true;
    uint64_t total = 0;
    rc = particles_counts(scope, b, 0u, &total); if (rc) return rc;
    *total_points = total;
    return CHROMA_OK;
}

int chroma_particles_points(chroma_ctx *ctx, const chroma_particle_points *out, uint32_t *d_offsets, uint64_t capacity)
{
    if (!ctx || !d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    const CallState &cs = scope.state();
    ParticlesBlock b;
    int rc = particles_block_again(scope, &b); if (rc) return rc;
    const uint64_t n = cs.particles_run.n;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), ctx->stream));
        return CHROMA_OK;
    }
    uint64_t total = 0;
    rc = particles_counts(scope, b, 0u, &total); if (rc) return rc;
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu points, the tracks have %llu", (unsigned long long)capacity, (unsigned long long)total);
    if (const char *why = particles::check_points(out)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    rc = exclusive_sum(b.scan, b.scan_bytes, b.counts, d_offsets, n + 1, ctx->stream); if (rc) return rc;
    hipLaunchKernelGGL(k_particles_gather_points, dim3(particle_blocks(total)), dim3(PARTICLES_BLOCK), 0, ctx->stream, b.matrix, (uint32_t)n,
                       (uint32_t)cs.particles_max_steps, d_offsets, *out, (uint32_t)total);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_particles_segments(chroma_ctx *ctx, const chroma_step_segments *out, int32_t *d_medium, uint64_t capacity)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    const CallState &cs = scope.state();
    ParticlesBlock b;
    int rc = particles_block_again(scope, &b); if (rc) return rc;
    const uint64_t n = cs.particles_run.n;
    if (n == 0) return CHROMA_OK;
    uint64_t total = 0;
    rc = particles_counts(scope, b, 1u, &total); if (rc) return rc;
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu segments, the tracks have %llu", (unsigned long long)capacity, (unsigned long long)total);
    if (total == 0) return CHROMA_OK;
    if (!out || !out->a || !out->b || !out->t_a || !out->t_b || !out->beta || !out->z || !out->qedep || !out->evidx || !d_medium)
        return set_error(CHROMA_ERR_INVALID, "segments: null pointer");
    rc = exclusive_sum(b.scan, b.scan_bytes, b.counts, b.offsets, n + 1, ctx->stream); if (rc) return rc;
    const particles::SegmentsOut o = {(float *)out->a, (float *)out->b, (float *)out->t_a, (float *)out->t_b, (float *)out->beta, (float *)out->z,
                                      (float *)out->qedep, (uint32_t *)out->evidx, d_medium};
    hipLaunchKernelGGL(k_particles_gather_segments, dim3(particle_blocks(total)), dim3(PARTICLES_BLOCK), 0, ctx->stream, b.matrix, cs.particles_run,
                       (uint32_t)cs.particles_max_steps, b.offsets, o, (uint32_t)total);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

}  // extern "C"
