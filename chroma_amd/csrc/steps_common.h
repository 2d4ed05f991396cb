// steps_common.h -- photons from charged-particle steps: what ONE segment and ONE photon compute, written once for the
// device kernels (kernels_steps.h) and for the host loops (steps_host.cpp).  Like include/chroma_math.h it is plain
// arithmetic under CM_FN: every operation is a single IEEE single-precision +, -, *, /, sqrt or one of cm_expf, cm_logf,
// cm_sincosf, and both sides are compiled with -ffp-contract=off, so the two produce the same bits.
//
// The small helpers the propagate path has as __device__ functions (interp_property, uniform_sphere, sample_cdf_uniform,
// rotate: propagate_device.h) are restated here in namespace steps with the same operation order, because the host side
// cannot include them.
#pragma once

#include <stdint.h>

#include "../../include/chroma_math.h"
#include "../../include/chroma_hip.h"

namespace steps {

constexpr uint64_t ID_BASE = 0x57E9000000000000ull;       // Philox id of segment g: ID_BASE + g
constexpr float POISSON_MAX_MEAN = 16.0f;                 // Knuth's product up to here, a rounded normal above
constexpr int REJECT_ROUNDS = 1000;                       // cap of the wavelength rejection loop
// 2 pi alpha x 1e6: positions are in mm, wavelengths in nm (alpha = 7.2973525693e-3, CODATA 2018)
constexpr float FRANK_TAMM = 45850.6183f;

struct v3 { float x, y, z; };
CM_FN v3 mk3(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
CM_FN v3 add(v3 a, v3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
CM_FN v3 sub(v3 a, v3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
CM_FN v3 mul(v3 a, float c) { return mk3(a.x * c, a.y * c, a.z * c); }
CM_FN v3 div(v3 a, float c) { return mk3(a.x / c, a.y / c, a.z / c); }
CM_FN float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
CM_FN v3 cross(v3 a, v3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
CM_FN float norm(v3 a) { return cm_sqrtf(dot(a, a)); }

// rotate (propagate_device.h; rotate.h:22-28): a about the unit vector n
CM_FN v3 rotate(v3 a, float phi, v3 n)
{
    float sin_phi, cos_phi;
    cm_sincosf(phi, &sin_phi, &cos_phi);
    return add(add(mul(a, cos_phi), mul(mul(n, dot(a, n)), 1.0f - cos_phi)), mul(cross(a, n), sin_phi));
}

CM_FN float uniform(cm_rng *r, float low, float high) { return low + cm_rng_uniform(r) * (high - low); }
// uniform_sphere (propagate_device.h; random.h:15-23)
CM_FN v3 uniform_sphere(cm_rng *r)
{
    float theta = uniform(r, 0.0f, 2 * CM_PI_F);
    float u = uniform(r, -1.0f, 1.0f);
    float c = cm_sqrtf(1.0f - u * u);
    float st, ct;
    cm_sincosf(theta, &st, &ct);
    return mk3(c * ct, c * st, u);
}
// sample_cdf_uniform (propagate_device.h; random.h:35-55).  A bracket over which the CDF does not rise (u == 1 at the flat
// end of a time CDF) gives the bracket's lower node where the original divides 0 by 0.
CM_FN float sample_cdf(cm_rng *r, int ncdf, float x0, float delta, const float *cdf_y)
{
    float u = cm_rng_uniform(r);
    int lower = 0;
    int upper = ncdf - 1;
    while (lower < upper - 1) {
        int half = (lower + upper) / 2;
        if (u < cdf_y[half]) upper = half; else lower = half;
    }
    float delta_cdf_y = cdf_y[upper] - cdf_y[lower];
    if (!(delta_cdf_y > 0.0f)) return x0 + delta * (float)lower;
    return x0 + delta * (float)lower + delta * (u - cdf_y[lower]) / delta_cdf_y;
}

// A chroma_light_source whose table pointers the caller of these functions can read (device copies in the kernels), with what
// is the same for every segment worked out once
struct Source {
    const float *refractive_index, *scintillation_cdf, *time_cdf;
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    float light_yield;
    uint32_t node_lo, node_hi;        // the Cherenkov range in grid nodes
    float wl_lo, wl_hi;               // ... and in nm
    float n_max;                      // largest n over those nodes (linear interpolation stays below it)
};

CM_FN float node_wavelength(const Source &s, uint32_t j) { return s.wavelength_start + (float)j * s.wavelength_step; }

// interp_property (propagate_device.h; geometry.h:64-75)
CM_FN float interp_property(const Source &s, float x, const float *fp)
{
    float start = s.wavelength_start, step = s.wavelength_step;
    uint32_t n = s.wavelength_n;
    if (x < start) return fp[0];
    if (x > (start + (float)(n - 1) * step)) return fp[n - 1];
    int jl = cm_f2i((x - start) / step);
    int ju = (jl + 1 < (int)n) ? jl + 1 : (int)n - 1;
    return fp[jl] + (x - (start + (float)jl * step)) * (fp[ju] - fp[jl]) / step;
}

// what chroma_light_source must satisfy before anything indexes its tables (host side; NULL: fine)
static inline const char *check_source(const chroma_light_source *s)
{
    if (!s || !s->refractive_index) return "light source: null pointer";
    if (s->wavelength_n < 2 || !(s->wavelength_step > 0.0f) || !(s->wavelength_start > 0.0f)) return "light source: need a rising wavelength grid of at least 2 nodes above 0";
    if (!(s->cherenkov_lo < s->cherenkov_hi) || s->cherenkov_hi >= s->wavelength_n) return "light source: Cherenkov range must be two different grid nodes, lo < hi";
    if (s->time_cdf && (s->time_n < 2 || !(s->time_step > 0.0f))) return "light source: a time CDF needs a rising grid of at least 2 nodes";
    if (!(s->light_yield >= 0.0f) || !cm_isfinite(s->light_yield)) return "light source: light_yield must be finite and not negative";
    return nullptr;
}
static inline const char *check_segments(const chroma_step_segments *g)
{
    if (!g) return "segments: null pointer";
    if (g->n > 0x3fffffffull) return "segments: more than 2^30 in one call";
    if (g->n && (!g->a || !g->b || !g->t_a || !g->t_b || !g->beta || !g->z || !g->qedep)) return "segments: null pointer";
    return nullptr;
}
// (host side: `ri` the refractive-index table where the HOST can read it; the three pointers where the callee can)
static inline Source make_source(const chroma_light_source &s, const float *ri, const float *scint_cdf, const float *time_cdf)
{
    Source o;
    o.refractive_index = ri; o.scintillation_cdf = scint_cdf; o.time_cdf = time_cdf;
    o.wavelength_n = s.wavelength_n; o.wavelength_start = s.wavelength_start; o.wavelength_step = s.wavelength_step;
    o.time_n = s.time_n; o.time_start = s.time_start; o.time_step = s.time_step;
    o.light_yield = s.scintillation_cdf ? s.light_yield : 0.0f;
    o.node_lo = s.cherenkov_lo; o.node_hi = s.cherenkov_hi;
    o.wl_lo = node_wavelength(o, o.node_lo); o.wl_hi = node_wavelength(o, o.node_hi);
    o.n_max = s.refractive_index[o.node_lo];
    for (uint32_t j = o.node_lo; j <= o.node_hi; j++) if (s.refractive_index[j] > o.n_max) o.n_max = s.refractive_index[j];
    return o;
}

// A chroma_light_media as the callee reads it: the three tables one row per medium, and per medium what make_source works out
// for one source -- the yield (0: no scintillation light), whether the emission is prompt, the largest n of the Cherenkov
// range.  What is the same for every row is here once.
struct Media {
    const float *refractive_index, *scintillation_cdf, *time_cdf;      // [nmedia][wavelength_n], ditto, [nmedia][time_n]
    const float *light_yield, *n_max;                                  // [nmedia]
    const uint8_t *prompt;                                             // [nmedia]
    uint32_t nmedia;
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    uint32_t node_lo, node_hi;
    float wl_lo, wl_hi;
};

// the Source of row m (m < nmedia): what make_source gives for that medium's chroma_light_source, field for field
CM_FN Source media_source(const Media &t, uint32_t m)
{
    Source o;
    o.refractive_index = t.refractive_index + (size_t)m * t.wavelength_n;
    o.scintillation_cdf = t.scintillation_cdf + (size_t)m * t.wavelength_n;
    o.time_cdf = t.prompt[m] ? nullptr : t.time_cdf + (size_t)m * t.time_n;
    o.wavelength_n = t.wavelength_n; o.wavelength_start = t.wavelength_start; o.wavelength_step = t.wavelength_step;
    o.time_n = t.time_n; o.time_start = t.time_start; o.time_step = t.time_step;
    o.light_yield = t.light_yield[m];
    o.node_lo = t.node_lo; o.node_hi = t.node_hi;
    o.wl_lo = t.wl_lo; o.wl_hi = t.wl_hi;
    o.n_max = t.n_max[m];
    return o;
}
// the row of a segment: a medium outside the table emits nothing
CM_FN bool medium_ok(const Media &t, int32_t m) { return m >= 0 && (uint32_t)m < t.nmedia; }

// what chroma_light_media_desc must satisfy (host side; NULL: fine): check_source's conditions for every row, and CDF rows
// that rise from their first node to their last, which sample_cdf's bisection takes for granted
static inline const char *check_cdf_row(const float *row, uint32_t n)
{
    for (uint32_t j = 0; j < n; j++) {
        if (!cm_isfinite(row[j])) return "not finite";
        if (j && row[j] < row[j - 1]) return "falls";
    }
    return nullptr;
}
static inline const char *check_media(const chroma_light_media_desc *d)
{
    if (!d || !d->refractive_index || !d->light_yield || !d->prompt) return "light media: null pointer";
    if (d->nmedia < 1 || d->nmedia > 256) return "light media: need 1 to 256 media";
    if (d->wavelength_n < 2 || !(d->wavelength_step > 0.0f) || !(d->wavelength_start > 0.0f)) return "light media: need a rising wavelength grid of at least 2 nodes above 0";
    if (!(d->cherenkov_lo < d->cherenkov_hi) || d->cherenkov_hi >= d->wavelength_n) return "light media: Cherenkov range must be two different grid nodes, lo < hi";
    for (uint32_t m = 0; m < d->nmedia; m++) {
        if (!(d->light_yield[m] >= 0.0f) || !cm_isfinite(d->light_yield[m])) return "light media: light_yield must be finite and not negative";
        if (d->light_yield[m] == 0.0f) continue;
        if (!d->scintillation_cdf) return "light media: a medium with a light yield needs a scintillation CDF";
        if (check_cdf_row(d->scintillation_cdf + (size_t)m * d->wavelength_n, d->wavelength_n)) return "light media: a scintillation CDF row is not finite or does not rise";
        if (d->prompt[m]) continue;
        if (!d->time_cdf || d->time_n < 2 || !(d->time_step > 0.0f)) return "light media: a time CDF needs a rising grid of at least 2 nodes";
        if (check_cdf_row(d->time_cdf + (size_t)m * d->time_n, d->time_n)) return "light media: a time CDF row is not finite or does not rise";
    }
    return nullptr;
}
// n_max[m], the largest n of row m over the Cherenkov range, as make_source finds it (host side)
static inline void media_n_max(const chroma_light_media_desc &d, float *n_max)
{
    for (uint32_t m = 0; m < d.nmedia; m++) {
        const float *row = d.refractive_index + (size_t)m * d.wavelength_n;
        n_max[m] = row[d.cherenkov_lo];
        for (uint32_t j = d.cherenkov_lo; j <= d.cherenkov_hi; j++) if (row[j] > n_max[m]) n_max[m] = row[j];
    }
}
// (host side: the seven pointers where the callee can read them)
static inline Media make_media(const chroma_light_media_desc &d, const float *ri, const float *scint_cdf, const float *time_cdf,
                               const float *light_yield, const uint8_t *prompt, const float *n_max)
{
    Media o;
    o.refractive_index = ri; o.scintillation_cdf = scint_cdf; o.time_cdf = time_cdf;
    o.light_yield = light_yield; o.n_max = n_max; o.prompt = prompt;
    o.nmedia = d.nmedia;
    o.wavelength_n = d.wavelength_n; o.wavelength_start = d.wavelength_start; o.wavelength_step = d.wavelength_step;
    o.time_n = d.time_n; o.time_start = d.time_start; o.time_step = d.time_step;
    o.node_lo = d.cherenkov_lo; o.node_hi = d.cherenkov_hi;
    o.wl_lo = o.wavelength_start + (float)o.node_lo * o.wavelength_step;          // (node_wavelength's expression)
    o.wl_hi = o.wavelength_start + (float)o.node_hi * o.wavelength_step;
    return o;
}

struct Segment { v3 a, b; float t_a, t_b, beta, z, qedep; uint32_t evidx; };
CM_FN Segment load_segment(const chroma_step_segments &g, uint64_t s)
{
    Segment o;
    o.a = mk3(g.a[3 * s], g.a[3 * s + 1], g.a[3 * s + 2]);
    o.b = mk3(g.b[3 * s], g.b[3 * s + 1], g.b[3 * s + 2]);
    o.t_a = g.t_a[s]; o.t_b = g.t_b[s]; o.beta = g.beta[s]; o.z = g.z[s]; o.qedep = g.qedep[s];
    o.evidx = g.evidx ? g.evidx[s] : 0u;
    return o;
}

CM_FN cm_rng stream(uint64_t seed, uint64_t segment, uint32_t word)
{
    cm_rng r;
    cm_rng_init(&r, seed, ID_BASE + segment, 0);
    r.stream = word;
    return r;
}

// 1 - 1/(beta^2 n^2): the Frank-Tamm factor (negative below threshold)
CM_FN float cherenkov_factor(float beta2, float n) { return 1.0f - 1.0f / (beta2 * (n * n)); }

// mean number of Cherenkov photons of a segment of length L (mm)
CM_FN float cherenkov_mean(const Source &s, float L, float beta, float z)
{
    if (!(L > 0.0f) || !(beta > 0.0f) || z == 0.0f) return 0.0f;
    const float beta2 = beta * beta;
    float sum = 0.0f, f_prev = 0.0f;
    for (uint32_t j = s.node_lo; j <= s.node_hi; j++) {
        const float wl = node_wavelength(s, j);
        float f = cherenkov_factor(beta2, s.refractive_index[j]);
        f = (f > 0.0f) ? f / (wl * wl) : 0.0f;
        if (j > s.node_lo) sum = sum + 0.5f * (f_prev + f) * s.wavelength_step;
        f_prev = f;
    }
    return ((FRANK_TAMM * (z * z)) * L) * sum;
}

CM_FN float scintillation_mean(const Source &s, float qedep) { return (qedep > 0.0f) ? s.light_yield * qedep : 0.0f; }

// a count of the given mean; a mean that is not positive draws nothing
CM_FN uint32_t draw_count(cm_rng *r, float mean)
{
    if (!(mean > 0.0f)) return 0u;
    if (mean <= POISSON_MAX_MEAN) {
        const float limit = cm_expf(-mean);
        float p = 1.0f;
        uint32_t k = 0;
        do { p = p * cm_rng_uniform(r); k++; } while (p > limit);
        return k - 1u;
    }
    const float x = cm_roundf(mean + cm_sqrtf(mean) * cm_rng_normal(r));
    return (x < 2147483648.0f) ? cm_f2u32(x) : 0x7fffffffu;
}

CM_FN void segment_counts(const Source &s, const Segment &g, uint64_t seed, uint64_t segment, uint32_t *n_cherenkov, uint32_t *n_scintillation)
{
    cm_rng r = stream(seed, segment, 0u);
    *n_cherenkov = draw_count(&r, cherenkov_mean(s, norm(sub(g.b, g.a)), g.beta, g.z));
    *n_scintillation = draw_count(&r, scintillation_mean(s, g.qedep));
}

struct PhotonOut { v3 pos, dir, pol; float wavelength, t; uint32_t flags; };

// photon j of a segment that emits n_cherenkov Cherenkov photons (j below that: one of them)
CM_FN PhotonOut make_photon(const Source &s, const Segment &g, uint64_t seed, uint64_t segment, uint32_t j, uint32_t n_cherenkov)
{
    cm_rng r = stream(seed, segment, 1u + j);
    const v3 ab = sub(g.b, g.a);
    PhotonOut o;
    if (j < n_cherenkov) {
        const v3 u = div(ab, norm(ab));                  // (a segment of no length emits no Cherenkov light)
        const float beta2 = g.beta * g.beta;
        const float f_max = cherenkov_factor(beta2, s.n_max);
        const float inv_lo = 1.0f / s.wl_hi, inv_hi = 1.0f / s.wl_lo;
        float wl = s.wl_lo, n = s.n_max;
        for (int round = 0; round < REJECT_ROUNDS; round++) {
            wl = 1.0f / uniform(&r, inv_lo, inv_hi);
            n = interp_property(s, wl, s.refractive_index);
            if (cm_rng_uniform(&r) * f_max <= cherenkov_factor(beta2, n)) break;
        }
        float cos_theta = 1.0f / (g.beta * n);
        if (cos_theta > 1.0f) cos_theta = 1.0f;          // (only a photon the capped loop gave up on)
        const float sin_theta = cm_sqrtf(1.0f - cos_theta * cos_theta);
        const float phi = uniform(&r, 0.0f, 2 * CM_PI_F);
        // e: a unit vector perpendicular to u, from the axis u has least of
        const float ax = cm_fabsf(u.x), ay = cm_fabsf(u.y), az = cm_fabsf(u.z);
        v3 e = cross(u, (ax <= ay && ax <= az) ? mk3(1.0f, 0.0f, 0.0f) : (ay <= az) ? mk3(0.0f, 1.0f, 0.0f) : mk3(0.0f, 0.0f, 1.0f));
        e = div(e, norm(e));
        // on the cone around u, and the unit vector of the (u, dir) plane at a right angle to it, both turned by phi about u
        o.dir = rotate(add(mul(u, cos_theta), mul(e, sin_theta)), phi, u);
        o.pol = rotate(sub(mul(u, sin_theta), mul(e, cos_theta)), phi, u);
        const float frac = cm_rng_uniform(&r);
        o.pos = add(g.a, mul(ab, frac));
        o.t = g.t_a + frac * (g.t_b - g.t_a);
        o.wavelength = wl;
        o.flags = CHROMA_CHERENKOV;
    } else {
        const float frac = cm_rng_uniform(&r);
        o.pos = add(g.a, mul(ab, frac));
        o.t = g.t_a + frac * (g.t_b - g.t_a);
        if (s.time_cdf) o.t = o.t + sample_cdf(&r, (int)s.time_n, s.time_start, s.time_step, s.time_cdf);
        o.wavelength = sample_cdf(&r, (int)s.wavelength_n, s.wavelength_start, s.wavelength_step, s.scintillation_cdf);
        o.dir = uniform_sphere(&r);
        const v3 aux = uniform_sphere(&r);
        const v3 pol = cross(aux, o.dir);
        o.pol = div(pol, norm(pol));
        o.flags = CHROMA_SCINTILLATION;
    }
    return o;
}

// the run (2 * segment + kind) photon i falls in: the largest k with offsets[k] <= i, among offsets[0 .. nruns] with
// offsets[0] == 0 and offsets[nruns] > i -- runs of no photons in front of it are stepped over
CM_FN uint32_t find_run(const uint32_t *offsets, uint32_t nruns, uint32_t i)
{
    uint32_t lo = 0, hi = nruns;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace steps
