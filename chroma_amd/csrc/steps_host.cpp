// steps_host.cpp -- chroma_steps_count_host / chroma_steps_generate_host: photons from charged-particle steps as plain loops
// on the host, over the same per-segment and per-photon functions as the device kernels (steps_common.h).  What the CPU tests
// run, what the GPU tests compare the kernels with bit for bit, and the generator of a machine without a GPU.
#include <stdint.h>

#include "steps_common.h"

static bool photons_ok(const chroma_photon_arrays *a)
{
    return a && a->pos && a->dir && a->pol && a->wavelengths && a->t && a->flags && a->last_hit_triangles && a->weights &&
           a->evidx && a->rng_counters;
}

extern "C" {

int chroma_steps_count_host(const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                            uint32_t *offsets, uint64_t *total)
{
    if (steps::check_source(src) || steps::check_segments(segs) || !offsets || !total) return CHROMA_ERR_INVALID;
    const steps::Source s = steps::make_source(*src, src->refractive_index, src->scintillation_cdf, src->time_cdf);
    uint64_t sum = 0;
    for (uint64_t k = 0; k < segs->n; k++) {
        uint32_t n_ch, n_sc;
        steps::segment_counts(s, steps::load_segment(*segs, k), seed, segs->segment_base + k, &n_ch, &n_sc);
        offsets[2 * k] = (uint32_t)sum;
        offsets[2 * k + 1] = (uint32_t)(sum + n_ch);
        sum += (uint64_t)n_ch + n_sc;
    }
    offsets[2 * segs->n] = (uint32_t)sum;
    *total = sum;
    return sum > 0xffffffffull ? CHROMA_ERR_INVALID : CHROMA_OK;
}

int chroma_steps_generate_host(const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                               const uint32_t *offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (steps::check_source(src) || steps::check_segments(segs) || !offsets) return CHROMA_ERR_INVALID;
    if (capacity < offsets[2 * segs->n]) return CHROMA_ERR_INVALID;
    if (offsets[2 * segs->n] == 0) return CHROMA_OK;
    if (!photons_ok(photons)) return CHROMA_ERR_INVALID;
    const steps::Source s = steps::make_source(*src, src->refractive_index, src->scintillation_cdf, src->time_cdf);
    for (uint64_t k = 0; k < segs->n; k++) {
        const steps::Segment g = steps::load_segment(*segs, k);
        const uint32_t first = offsets[2 * k], n_ch = offsets[2 * k + 1] - first, n = offsets[2 * k + 2] - first;
        for (uint32_t j = 0; j < n; j++) {
            const steps::PhotonOut p = steps::make_photon(s, g, seed, segs->segment_base + k, j, n_ch);
            const size_t i = (size_t)first + j;
            photons->pos[3 * i] = p.pos.x; photons->pos[3 * i + 1] = p.pos.y; photons->pos[3 * i + 2] = p.pos.z;
            photons->dir[3 * i] = p.dir.x; photons->dir[3 * i + 1] = p.dir.y; photons->dir[3 * i + 2] = p.dir.z;
            photons->pol[3 * i] = p.pol.x; photons->pol[3 * i + 1] = p.pol.y; photons->pol[3 * i + 2] = p.pol.z;
            photons->wavelengths[i] = p.wavelength;
            photons->t[i] = p.t;
            photons->flags[i] = p.flags;
            photons->last_hit_triangles[i] = -1;
            photons->weights[i] = 1.0f;
            photons->evidx[i] = g.evidx;
            photons->rng_counters[i] = 0u;
        }
    }
    return CHROMA_OK;
}

}  // extern "C"
