// particles_common.h -- the charged-particle stepper (continuous slowing down): what ONE particle computes in ONE iteration,
// written once for the device kernels (kernels_particles.h) and for the host loops (particles_host.cpp), as steps_common.h
// is for the light source: single IEEE operations and chroma_math.h's functions under CM_FN, both sides compiled with
// -ffp-contract=off, so the two produce the same bits.
//
// Units: MeV, mm, ns.  The model: mean stopping power from a table (linear in log ke), every step limited by max_step, by a
// fraction max_loss of ke and by the next volume boundary, Highland multiple scattering of the direction at the end of the step.
// No secondaries, no straggling, no lateral displacement.
#pragma once

#include "steps_common.h"

namespace particles {

using steps::v3; using steps::mk3; using steps::add; using steps::mul; using steps::div; using steps::dot; using steps::cross; using steps::norm;

constexpr uint64_t STREAM_BASE = 0x9A27000000000000ull;   // Philox id of particle p: STREAM_BASE + p (the segments': steps::ID_BASE)
constexpr int NSPECIES = CHROMA_PARTICLE_SPECIES;         // e, mu, pi, K, p, alpha: the rows of a medium's table
constexpr float ELECTRON_MASS = 0.51099895f;

// the table of chroma_stopping_media_desc where the callee can read it
struct Table {
    const float *stopping_power;      // [nmedia][NSPECIES][nke] MeV/mm at ke_min exp(j log_step)
    const float *radiation_length;    // [nmedia] mm; +inf: none
    const float *birks;               // [nmedia] mm/MeV
    uint32_t nmedia, nke;
    float ke_min, log_step;
};

// one particle's chroma_particle_arrays entry in registers
struct State {
    v3 pos, dir;
    float ke, t;
    int32_t last_hit, species;
    float z, mass;
    uint32_t nsteps, rng_counter, status;
};

// one step point: the columns of chroma_particle_points
struct Point { v3 pos; float t; v3 dir; float ke, edep, qedep; int32_t medium; };

// what advance() wrote: the vertex (row 0) and / or the post-step point (row State::nsteps, after the call)
enum : uint32_t { WROTE_VERTEX = 1u, WROTE_STEP = 2u };

static inline const char *check_table(const chroma_stopping_media_desc *d)
{
    if (!d || !d->stopping_power || !d->radiation_length || !d->birks) return "stopping media: null pointer";
    if (d->nmedia < 1 || d->nmedia > 256) return "stopping media: need 1 to 256 media";
    if (d->nke < 2 || d->nke > (1u << 20)) return "stopping media: need 2 to 2^20 energy nodes";
    if (!(d->ke_min > 0.0f) || !cm_isfinite(d->ke_min) || !(d->log_step > 0.0f) || !cm_isfinite(d->log_step)) return "stopping media: need ke_min > 0 and a rising energy grid";
    const size_t count = (size_t)d->nmedia * NSPECIES * d->nke;
    for (size_t k = 0; k < count; k++)
        if (!cm_isfinite(d->stopping_power[k]) || d->stopping_power[k] < 0.0f) return "stopping media: a stopping power is negative or not finite";
    for (uint32_t m = 0; m < d->nmedia; m++) {
        if (!(d->radiation_length[m] > 0.0f)) return "stopping media: a radiation length is not above 0";          // (NaN too; +inf is fine)
        if (!(d->birks[m] >= 0.0f) || !cm_isfinite(d->birks[m])) return "stopping media: a Birks constant is negative or not finite";
    }
    return nullptr;
}
static inline const char *check_options(const chroma_particle_options *o)
{
    if (!o) return "particle options: null pointer";
    if (o->max_steps < 1 || o->max_steps > (1 << 20)) return "particle options: max_steps must be 1 to 2^20";
    if (!(o->max_step > 0.0f) || !cm_isfinite(o->max_step)) return "particle options: max_step must be finite and above 0";
    if (!(o->max_loss > 0.0f) || !(o->max_loss <= 1.0f)) return "particle options: max_loss must be in (0, 1]";
    if (!(o->ke_cut >= 0.0f) || !cm_isfinite(o->ke_cut)) return "particle options: ke_cut must be finite and not negative";
    if (o->outside < -1) return "particle options: outside must be a medium row or -1";
    return nullptr;
}
static inline const char *check_particles(const chroma_particle_arrays *p)
{
    if (!p) return "particles: null pointer";
    if (p->n > 0x3fffffffull) return "particles: more than 2^30 in one call";
    if (p->n && (!p->pos || !p->dir || !p->ke || !p->t || !p->last_hit || !p->species || !p->z || !p->mass || !p->evidx || !p->nsteps ||
                 !p->rng_counter || !p->status)) return "particles: null pointer";
    return nullptr;
}
static inline const char *check_points(const chroma_particle_points *q)
{
    if (!q || !q->pos || !q->t || !q->dir || !q->ke || !q->edep || !q->qedep || !q->medium) return "particle points: null pointer";
    return nullptr;
}
static inline Table make_table(const chroma_stopping_media_desc &d, const float *stopping_power, const float *radiation_length, const float *birks)
{
    Table t;
    t.stopping_power = stopping_power; t.radiation_length = radiation_length; t.birks = birks;
    t.nmedia = d.nmedia; t.nke = d.nke; t.ke_min = d.ke_min; t.log_step = d.log_step;
    return t;
}

CM_FN State load_state(const chroma_particle_arrays &p, uint64_t i)
{
    State s;
    s.pos = mk3(p.pos[3 * i], p.pos[3 * i + 1], p.pos[3 * i + 2]);
    s.dir = mk3(p.dir[3 * i], p.dir[3 * i + 1], p.dir[3 * i + 2]);
    s.ke = p.ke[i]; s.t = p.t[i]; s.last_hit = p.last_hit[i]; s.species = p.species[i]; s.z = p.z[i]; s.mass = p.mass[i];
    s.nsteps = p.nsteps[i]; s.rng_counter = p.rng_counter[i]; s.status = p.status[i];
    return s;
}
CM_FN void store_state(const chroma_particle_arrays &p, uint64_t i, const State &s)
{
    p.pos[3 * i] = s.pos.x; p.pos[3 * i + 1] = s.pos.y; p.pos[3 * i + 2] = s.pos.z;
    p.dir[3 * i] = s.dir.x; p.dir[3 * i + 1] = s.dir.y; p.dir[3 * i + 2] = s.dir.z;
    p.ke[i] = s.ke; p.t[i] = s.t; p.last_hit[i] = s.last_hit;
    p.nsteps[i] = s.nsteps; p.rng_counter[i] = s.rng_counter; p.status[i] = s.status;
}
CM_FN Point load_point(const chroma_particle_points &q, uint64_t row)
{
    Point o;
    o.pos = mk3(q.pos[3 * row], q.pos[3 * row + 1], q.pos[3 * row + 2]);
    o.dir = mk3(q.dir[3 * row], q.dir[3 * row + 1], q.dir[3 * row + 2]);
    o.t = q.t[row]; o.ke = q.ke[row]; o.edep = q.edep[row]; o.qedep = q.qedep[row]; o.medium = q.medium[row];
    return o;
}
CM_FN void store_point(const chroma_particle_points &q, uint64_t row, const Point &o)
{
    q.pos[3 * row] = o.pos.x; q.pos[3 * row + 1] = o.pos.y; q.pos[3 * row + 2] = o.pos.z;
    q.dir[3 * row] = o.dir.x; q.dir[3 * row + 1] = o.dir.y; q.dir[3 * row + 2] = o.dir.z;
    q.t[row] = o.t; q.ke[row] = o.ke; q.edep[row] = o.edep; q.qedep[row] = o.qedep; q.medium[row] = o.medium;
}
// the row of point k of particle i in the step-major matrix of n particles
CM_FN uint64_t matrix_row(uint64_t n, uint64_t i, uint32_t k) { return (uint64_t)k * n + i; }

// beta of a kinetic energy: sqrt(1 - 1/gamma^2) with gamma = 1 + ke/mass (0 at rest)
CM_FN float beta_of(float ke, float mass)
{
    const float gamma = 1.0f + ke / mass;
    return cm_sqrtf(1.0f - 1.0f / (gamma * gamma));
}

// S of (medium, species) at ke: linear in x = log(ke/ke_min)/log_step between the nodes, the end nodes' values beyond them
CM_FN float stopping_power(const Table &t, uint32_t medium, uint32_t species, float ke)
{
    const float *row = t.stopping_power + ((size_t)medium * NSPECIES + species) * t.nke;
    const float x = cm_logf(ke / t.ke_min) / t.log_step;
    if (!(x > 0.0f)) return row[0];
    if (x >= (float)(t.nke - 1u)) return row[t.nke - 1u];
    const int j = cm_f2i(x);
    return row[j] + (x - (float)j) * (row[j + 1] - row[j]);
}

// The Highland width of a step of length s (> 0) in a medium of radiation length x0 (finite)
CM_FN float highland_theta0(float s, float x0, float beta, float ke, float mass, float z)
{
    const float p = cm_sqrtf(ke * (ke + 2.0f * mass));
    const float ratio = s / x0;
    float bracket = 1.0f + 0.038f * cm_logf((ratio * (z * z)) / (beta * beta));
    if (!(bracket > 0.0f)) bracket = 0.0f;
    return ((13.6f / (beta * p)) * cm_fabsf(z)) * cm_sqrtf(ratio) * bracket;
}

// (u, v): the orthonormal pair at a right angle to the unit vector d -- u = normalize(d x e) with e the axis d has least of
// (x before y before z on a tie), v = d x u
CM_FN void perpendicular_pair(v3 d, v3 *u, v3 *v)
{
    const float ax = cm_fabsf(d.x), ay = cm_fabsf(d.y), az = cm_fabsf(d.z);
    v3 e = cross(d, (ax <= ay && ax <= az) ? mk3(1.0f, 0.0f, 0.0f) : (ay <= az) ? mk3(0.0f, 1.0f, 0.0f) : mk3(0.0f, 0.0f, 1.0f));
    *u = div(e, norm(e));
    *v = cross(d, *u);
}

CM_FN int has_nan(v3 a) { return cm_isnan(a.x) || cm_isnan(a.y) || cm_isnan(a.z); }

// One iteration of particle `particle` (its global index: the random stream).  `distance`, `triangle`: the nearest triangle
// along s.dir (triangle < 0 or a distance that is not finite: none); `medium`: the row on the particle's side of it.
// Returns WROTE_*: out[0] the vertex, out[1] the post-step point.
CM_FN uint32_t advance(const Table &t, const chroma_particle_options &o, uint64_t seed, uint64_t particle, State &s, float distance,
                       int32_t triangle, int32_t medium, Point *out)
{
    if (s.status != CHROMA_PARTICLE_ALIVE) return 0u;
    uint32_t wrote = 0u;
    if (s.nsteps == 0u) {
        out[0].pos = s.pos; out[0].t = s.t; out[0].dir = s.dir; out[0].ke = s.ke; out[0].edep = 0.0f; out[0].qedep = 0.0f; out[0].medium = -1;
        wrote = WROTE_VERTEX;
    }
    if (s.species < 0 || s.species >= NSPECIES || s.z == 0.0f || !(s.mass > 0.0f) || !(s.ke > 0.0f)) { s.status = CHROMA_PARTICLE_UNTRACKED; return wrote; }
    // 1. the medium
    if (medium < 0 || (uint32_t)medium >= t.nmedia) { s.status = CHROMA_PARTICLE_LEFT; return wrote; }
    // 2. the stopping power
    const float S = stopping_power(t, (uint32_t)medium, (uint32_t)s.species, s.ke);
    // 3. nothing ahead and nothing to lose
    const bool hit = triangle >= 0 && cm_isfinite(distance);
    if (!hit && S == 0.0f) { s.status = CHROMA_PARTICLE_LEFT; return wrote; }
    // 4. the physics step
    float s_phys = o.max_step;
    if (S > 0.0f) {
        const float by_loss = (o.max_loss * s.ke) / S;
        if (by_loss < s_phys) s_phys = by_loss;
    }
    // 5. the boundary
    float len = s_phys;
    if (hit && distance <= s_phys) { len = distance; s.last_hit = triangle; } else s.last_hit = -1;
    // 6. the loss
    const float ke0 = s.ke;
    float edep = S * len;
    if (edep > ke0) edep = ke0;
    float ke1 = ke0 - edep;
    if (ke1 < o.ke_cut) { edep = ke0; ke1 = 0.0f; }
    const float qedep = edep / (1.0f + t.birks[medium] * S);
    // 7. the move
    const float beta = beta_of(ke0, s.mass);
    s.pos = add(s.pos, mul(s.dir, len));
    if (beta > 0.0f) s.t = s.t + len / (beta * CM_SPEED_OF_LIGHT);
    s.ke = ke1;
    // 8. the scatter
    const float x0 = t.radiation_length[medium];
    if (o.scatter && len > 0.0f && cm_isfinite(x0) && beta > 0.0f) {
        const float theta0 = highland_theta0(len, x0, beta, ke0, s.mass, s.z);
        cm_rng r;
        cm_rng_init(&r, seed, STREAM_BASE + particle, s.rng_counter);
        const float g1 = cm_rng_normal(&r), g2 = cm_rng_normal(&r);
        s.rng_counter = r.counter;
        v3 u, v;
        perpendicular_pair(s.dir, &u, &v);
        const v3 d = add(add(s.dir, mul(u, theta0 * g1)), mul(v, theta0 * g2));
        s.dir = div(d, norm(d));
    }
    // 9. the point
    s.nsteps = s.nsteps + 1u;
    out[1].pos = s.pos; out[1].t = s.t; out[1].dir = s.dir; out[1].ke = ke1; out[1].edep = edep; out[1].qedep = qedep; out[1].medium = medium;
    if (has_nan(s.pos) || has_nan(s.dir)) s.status = CHROMA_PARTICLE_NAN_ABORT;
    else if (ke1 == 0.0f) s.status = CHROMA_PARTICLE_STOPPED;
    else if (s.nsteps >= (uint32_t)o.max_steps) s.status = CHROMA_PARTICLE_TRUNCATED;
    return wrote | WROTE_STEP;
}

// advance() for particle i of `p`, its points into the step-major matrix `q`
CM_FN void advance_particle(const Table &t, const chroma_particle_options &o, uint64_t seed, const chroma_particle_arrays &p, uint64_t i,
                            float distance, int32_t triangle, int32_t medium, const chroma_particle_points &q)
{
    State s = load_state(p, i);
    if (s.status != CHROMA_PARTICLE_ALIVE) return;
    if (s.nsteps >= (uint32_t)o.max_steps) { p.status[i] = CHROMA_PARTICLE_TRUNCATED; return; }      // (no row left: a caller's own nsteps)
    Point out[2];
    const uint32_t wrote = advance(t, o, seed, p.particle_base + i, s, distance, triangle, medium, out);
    if (wrote & WROTE_VERTEX) store_point(q, matrix_row(p.n, i, 0u), out[0]);
    if (wrote & WROTE_STEP) store_point(q, matrix_row(p.n, i, s.nsteps), out[1]);
    store_state(p, i, s);
}

// points of a particle, with a count the matrix cannot hold cut down to it
CM_FN uint32_t points_of(uint32_t nsteps, uint32_t max_steps) { return (nsteps < max_steps ? nsteps : max_steps) + 1u; }

// Flat point j = point k of particle i, from the matrix (gather of chroma_particles_points)
CM_FN void gather_point(const chroma_particle_points &matrix, uint64_t n, uint64_t i, uint32_t k, const chroma_particle_points &flat, uint64_t j)
{
    store_point(flat, j, load_point(matrix, matrix_row(n, i, k)));
}

// Flat segment j = points k -> k + 1 of particle i (chroma_particles_segments): the arrays of a chroma_step_segments and its medium
struct SegmentsOut { float *a, *b, *t_a, *t_b, *beta, *z, *qedep; uint32_t *evidx; int32_t *medium; };
CM_FN void gather_segment(const chroma_particle_points &matrix, const chroma_particle_arrays &p, uint64_t i, uint32_t k, const SegmentsOut &out, uint64_t j)
{
    const Point a = load_point(matrix, matrix_row(p.n, i, k)), b = load_point(matrix, matrix_row(p.n, i, k + 1u));
    const float mass = p.mass[i];
    out.a[3 * j] = a.pos.x; out.a[3 * j + 1] = a.pos.y; out.a[3 * j + 2] = a.pos.z;
    out.b[3 * j] = b.pos.x; out.b[3 * j + 1] = b.pos.y; out.b[3 * j + 2] = b.pos.z;
    out.t_a[j] = a.t; out.t_b[j] = b.t;
    out.beta[j] = 0.5f * (beta_of(a.ke, mass) + beta_of(b.ke, mass));
    out.z[j] = p.z[i];
    out.qedep[j] = b.qedep;
    out.evidx[j] = p.evidx[i];
    out.medium[j] = b.medium;
}

}  // namespace particles
