// steps_host.cpp -- chroma_steps_count_host / chroma_steps_generate_host: photons from charged-particle steps as plain loops
// on the host, over the same per-segment and per-photon functions as the device kernels (steps_common.h).  What the CPU tests
// run, what the GPU tests compare the kernels with bit for bit, and the generator of a machine without a GPU.
#include <stdint.h>

#include <vector>

#include "steps_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

// A chroma_light_media_desc as the table the per-segment functions read, over the caller's own arrays.  A table no row of
// which is read may be NULL in the desc: the refractive indices stand in for it, so that a row's address can be formed.
struct HostMedia {
    std::vector<float> n_max;
    steps::Media view;
    explicit HostMedia(const chroma_light_media_desc &d) : n_max(d.nmedia)
    {
        steps::media_n_max(d, n_max.data());
        view = steps::make_media(d, d.refractive_index, d.scintillation_cdf ? d.scintillation_cdf : d.refractive_index,
                                 d.time_cdf ? d.time_cdf : d.refractive_index, d.light_yield, d.prompt, n_max.data());
    }
};
static const char *check_media_call(const chroma_light_media_desc *desc, const chroma_step_segments *segs, const int32_t *medium)
{
    if (const char *why = steps::check_media(desc)) return why;
    if (const char *why = steps::check_segments(segs)) return why;
    if (segs->n && !medium) return "segments: no medium array";
    return nullptr;
}

static bool photons_ok(const chroma_photon_arrays *a)
{
    return a && a->pos && a->dir && a->pol && a->wavelengths && a->t && a->flags && a->last_hit_triangles && a->weights &&
           a->evidx && a->rng_counters;
}

static void store_photon(const chroma_photon_arrays *photons, size_t i, const steps::PhotonOut &p, uint32_t evidx)
{
    photons->pos[3 * i] = p.pos.x; photons->pos[3 * i + 1] = p.pos.y; photons->pos[3 * i + 2] = p.pos.z;
    photons->dir[3 * i] = p.dir.x; photons->dir[3 * i + 1] = p.dir.y; photons->dir[3 * i + 2] = p.dir.z;
    photons->pol[3 * i] = p.pol.x; photons->pol[3 * i + 1] = p.pol.y; photons->pol[3 * i + 2] = p.pol.z;
    photons->wavelengths[i] = p.wavelength;
    photons->t[i] = p.t;
    photons->flags[i] = p.flags;
    photons->last_hit_triangles[i] = -1;
    photons->weights[i] = 1.0f;
    photons->evidx[i] = evidx;
    photons->rng_counters[i] = 0u;
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
        for (uint32_t j = 0; j < n; j++)
            store_photon(photons, (size_t)first + j, steps::make_photon(s, g, seed, segs->segment_base + k, j, n_ch), g.evidx);
    }
    return CHROMA_OK;
}

int chroma_steps_count_media_host(const chroma_light_media_desc *desc, const chroma_step_segments *segs, const int32_t *medium,
                                  uint64_t seed, uint32_t *offsets, uint64_t *total)
{
    if (const char *why = check_media_call(desc, segs, medium)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (!offsets || !total) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const HostMedia media(*desc);
    uint64_t sum = 0;
    for (uint64_t k = 0; k < segs->n; k++) {
        uint32_t n_ch = 0, n_sc = 0;
        if (steps::medium_ok(media.view, medium[k]))
            steps::segment_counts(steps::media_source(media.view, (uint32_t)medium[k]), steps::load_segment(*segs, k), seed,
                                  segs->segment_base + k, &n_ch, &n_sc);
        offsets[2 * k] = (uint32_t)sum;
        offsets[2 * k + 1] = (uint32_t)(sum + n_ch);
        sum += (uint64_t)n_ch + n_sc;
    }
    offsets[2 * segs->n] = (uint32_t)sum;
    *total = sum;
    if (sum > 0xffffffffull) return set_error(CHROMA_ERR_INVALID, "%llu photons in one call: more than 32-bit offsets hold, pass fewer segments", (unsigned long long)sum);
    return CHROMA_OK;
}

int chroma_steps_generate_media_host(const chroma_light_media_desc *desc, const chroma_step_segments *segs, const int32_t *medium,
                                     uint64_t seed, const uint32_t *offsets, const chroma_photon_arrays *photons, uint64_t capacity)
{
    if (const char *why = check_media_call(desc, segs, medium)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (!offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const uint32_t total = offsets[2 * segs->n];
    if (capacity < total) return set_error(CHROMA_ERR_INVALID, "room for %llu photons, the segments emit %u", (unsigned long long)capacity, total);
    if (total == 0) return CHROMA_OK;
    if (!photons_ok(photons)) return set_error(CHROMA_ERR_INVALID, "photon arrays: null pointer");
    const HostMedia media(*desc);
    for (uint64_t k = 0; k < segs->n; k++) {
        const uint32_t first = offsets[2 * k], n_ch = offsets[2 * k + 1] - first, n = offsets[2 * k + 2] - first;
        if (!n) continue;
        if (!steps::medium_ok(media.view, medium[k])) return set_error(CHROMA_ERR_INVALID, "segment %llu has photons and no medium: offsets of another call", (unsigned long long)k);
        const steps::Source s = steps::media_source(media.view, (uint32_t)medium[k]);
        const steps::Segment g = steps::load_segment(*segs, k);
        for (uint32_t j = 0; j < n; j++) store_photon(photons, (size_t)first + j, steps::make_photon(s, g, seed, segs->segment_base + k, j, n_ch), g.evidx);
    }
    return CHROMA_OK;
}

}  // extern "C"
