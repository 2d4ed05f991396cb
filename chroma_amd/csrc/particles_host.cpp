// particles_host.cpp -- the charged-particle stepper as plain loops on the host, over the same per-particle functions as the
// device kernels (particles_common.h): one iteration on the caller's casts (chroma_particles_advance_host), the whole loop in
// one medium (chroma_particles_track_host), and the flat points and segments of a matrix.  What the CPU tests run and what the
// GPU tests compare the kernels with bit for bit.
#include <stdint.h>

#include "particles_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

static const char *check_call(const chroma_stopping_media_desc *desc, const chroma_particle_arrays *particles, const chroma_particle_options *options,
                              const chroma_particle_points *points)
{
    if (const char *why = particles::check_table(desc)) return why;
    if (const char *why = particles::check_particles(particles)) return why;
    if (const char *why = particles::check_options(options)) return why;
    if (particles->n) if (const char *why = particles::check_points(points)) return why;
    return nullptr;
}

// the sum of the particles' point counts (or of their segments: a point less each)
static uint64_t count_rows(const chroma_particle_arrays &p, uint32_t max_steps, uint32_t less, uint32_t *offsets)
{
    uint64_t sum = 0;
    for (uint64_t i = 0; i < p.n; i++) {
        if (offsets) offsets[i] = (uint32_t)sum;
        sum += particles::points_of(p.nsteps[i], max_steps) - less;
    }
    if (offsets) offsets[p.n] = (uint32_t)sum;
    return sum;
}

extern "C" {

int chroma_particles_advance_host(const chroma_stopping_media_desc *desc, const chroma_particle_arrays *p, const chroma_particle_options *options,
                                  uint64_t seed, const float *distance, const int32_t *triangle, const int32_t *medium,
                                  const chroma_particle_points *points)
{
    if (const char *why = check_call(desc, p, options, points)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const particles::Table t = particles::make_table(*desc, desc->stopping_power, desc->radiation_length, desc->birks);
    for (uint64_t i = 0; i < p->n; i++)
        particles::advance_particle(t, *options, seed, *p, i, distance ? distance[i] : cm_inff(), triangle ? triangle[i] : -1,
                                    medium ? medium[i] : options->outside, *points);
    return CHROMA_OK;
}

int chroma_particles_track_host(const chroma_stopping_media_desc *desc, const chroma_particle_arrays *p, const chroma_particle_options *options,
                                uint64_t seed, const chroma_particle_points *points, uint64_t *total_points)
{
    if (!total_points) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *total_points = 0;
    if (const char *why = check_call(desc, p, options, points)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    const particles::Table t = particles::make_table(*desc, desc->stopping_power, desc->radiation_length, desc->birks);
    for (uint64_t i = 0; i < p->n; i++)          // (a particle ends after max_steps iterations at the latest)
        for (int32_t k = 0; k <= options->max_steps && p->status[i] == CHROMA_PARTICLE_ALIVE; k++)
            particles::advance_particle(t, *options, seed, *p, i, cm_inff(), -1, options->outside, *points);
    *total_points = count_rows(*p, (uint32_t)options->max_steps, 0u, nullptr);
    return CHROMA_OK;
}

int chroma_particles_points_host(const chroma_particle_arrays *p, int32_t max_steps, const chroma_particle_points *matrix,
                                 const chroma_particle_points *out, uint32_t *offsets, uint64_t capacity)
{
    if (const char *why = particles::check_particles(p)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (max_steps < 1 || !offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const uint64_t total = count_rows(*p, (uint32_t)max_steps, 0u, nullptr);
    if (total > 0xffffffffull) return set_error(CHROMA_ERR_INVALID, "%llu points: more than 32-bit offsets hold", (unsigned long long)total);
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu points, the tracks have %llu", (unsigned long long)capacity, (unsigned long long)total);
    count_rows(*p, (uint32_t)max_steps, 0u, offsets);
    if (!total) return CHROMA_OK;
    if (particles::check_points(matrix) || particles::check_points(out)) return set_error(CHROMA_ERR_INVALID, "particle points: null pointer");
    for (uint64_t i = 0; i < p->n; i++)
        for (uint32_t k = 0; k < offsets[i + 1] - offsets[i]; k++) particles::gather_point(*matrix, p->n, i, k, *out, (uint64_t)offsets[i] + k);
    return CHROMA_OK;
}

int chroma_particles_segments_host(const chroma_particle_arrays *p, int32_t max_steps, const chroma_particle_points *matrix,
                                   const chroma_step_segments *out, int32_t *medium, uint64_t capacity)
{
    if (const char *why = particles::check_particles(p)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (max_steps < 1 || !out) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const uint64_t total = count_rows(*p, (uint32_t)max_steps, 1u, nullptr);
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu segments, the tracks have %llu", (unsigned long long)capacity, (unsigned long long)total);
    if (!total) return CHROMA_OK;
    if (particles::check_points(matrix) || !out->a || !out->b || !out->t_a || !out->t_b || !out->beta || !out->z || !out->qedep || !out->evidx || !medium)
        return set_error(CHROMA_ERR_INVALID, "segments: null pointer");
    const particles::SegmentsOut o = {(float *)out->a, (float *)out->b, (float *)out->t_a, (float *)out->t_b, (float *)out->beta, (float *)out->z,
                                      (float *)out->qedep, (uint32_t *)out->evidx, medium};
    uint64_t j = 0;
    for (uint64_t i = 0; i < p->n; i++)
        for (uint32_t k = 0; k + 1u < particles::points_of(p->nsteps[i], (uint32_t)max_steps); k++) particles::gather_segment(*matrix, *p, i, k, o, j++);
    return CHROMA_OK;
}

}  // extern "C"
