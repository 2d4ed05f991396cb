// kernels_hybrid_render.h -- the hybrid photon-mapped render (chroma/cuda/hybrid_render.cu): k_hybrid_lookup
// (update_xyz_lookup), k_hybrid_image (update_xyz_image), k_hybrid_pixels (process_image), and k_hybrid_reduce, the
// deterministic replacement of the reference's fAtomicAdd.
// One of the kernel families of libchroma_hip.so; included by chroma_hip.hip after kernel_propagate_fused.h (it runs the
// same step functions as k_propagate, one lane per sample).
#pragma once

// apply_hit (propagate_device.h) that also gives the side of the triangle the photon arrives at: the reference's
// State::inside_to_outside (photon.h:114,122), by apply_hit_normal's own sign test on the incoming direction.
// (Kept here, not in State: the shared State and apply_hit stay as the other kernels compile them.)
__device__ inline bool hybrid_apply_hit(State &s, Photon &p, const GeoView &g, int triangle, float distance)
{
    p.last_hit_triangle = triangle;
    s.distance_to_boundary = distance;
    if (triangle == -1) {
        p.history |= CHROMA_NO_HIT;
        return false;
    }
    const float4 *t = g.tri + TRI_STRIDE * (size_t)g.tri_to_dev[triangle];
    const float4 a = t[0], b = t[1], c = t[2];
    const v3 normal = triangle_normal(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z));
    const bool inside_to_outside = !(dot(normal, -p.direction) > 0.0f);
    apply_hit_normal(s, p, g, distance, normal, __float_as_uint(a.w));
    return inside_to_outside;
}

// to_diffuse (hybrid_render.cu:20-58): k_propagate's step loop for one lane (all-models physics, no weights, no
// scatter-first, the NaN abort) that also stops after the first step which sets CHROMA_REFLECT_DIFFUSE.  A sample's
// outcome is therefore the propagate loop's, stepped one step at a time and stopped at the first diffuse reflection.
// Wave-uniform like intersect_mesh: every lane of the wave calls it, a lane without a photon with live = false.
// Returns the side (inside to outside) of the last triangle hit.
template <int LDS_N>
__device__ inline bool to_diffuse(Photon &p, cm_rng &rng, const GeoView &g, int max_steps, bool live, uint32_t *lds,
                                  LaneCounters &cnt)
{
    State s;
    bool inside_to_outside = false;
    int steps = 0;
    while (__any(live && steps < max_steps)) {
        bool stepping = live && steps < max_steps;
        if (stepping) {
            steps++;
            if (cm_isnan(p.direction.x * p.direction.y * p.direction.z * p.position.x * p.position.y * p.position.z)) {
                p.history |= CHROMA_NO_HIT | CHROMA_NAN_ABORT;
                live = false;
                stepping = false;
            }
        }
        float distance;
        int triangle = intersect_mesh<LDS_N, PROP_BLOCK, false>(g, p.position, p.direction, distance, p.last_hit_triangle,
                                                                lds, cnt, stepping);
        if (stepping) {
            inside_to_outside = hybrid_apply_hit(s, p, g, triangle, distance);
            if (triangle == -1)
                live = false;
            else
                live = step_after_hit(p, s, rng, g, false, 0) && !(p.history & CHROMA_REFLECT_DIFFUSE);
        }
    }
    return inside_to_outside;
}

// update_xyz_lookup (hybrid_render.cu:63-131): thread k samples a point of triangle offset + k (k < nthreads; the host
// caps offset + nthreads at the triangle count), casts the ray from the source at it, and, when that ray's first hit is
// the triangle itself, follows the photon to its first diffuse reflection.  Instead of adding cos_theta * xyz to the
// diffusing triangle's lookup entry with an atomic, it writes the record (key = 2 * triangle + side, value): key_none
// for a sample that contributes nothing.  k_hybrid_reduce adds the records up after a stable sort by key.
// Random stream of thread k: (seed, id_base + k), from rng_counters[k], written back.
// Sample outputs (s_tri, s_side, s_history, s_cos: all or none): diffusing triangle or -1, side (1 = inside to outside),
// final history (0 when the ray missed the triangle), cos_theta (0 when it missed).
template <int LDS_N>
__global__ __launch_bounds__(PROP_BLOCK) void
k_hybrid_lookup(GeoView g, int nthreads, int offset, float px, float py, float pz, uint64_t seed, uint64_t id_base,
                uint32_t *rng_counters, float wavelength, float xr, float xg, float xb, int max_steps, uint32_t key_none,
                uint32_t *keys, uint32_t *ids, float *values, int32_t *s_tri, uint32_t *s_side, uint32_t *s_history,
                float *s_cos, DeviceCounters *counters)
{
    __shared__ uint32_t s_lds[TRAV_LDS_WORDS(LDS_N, PROP_BLOCK)];
    uint32_t *lds = s_lds + threadIdx.x;

    const int k = blockIdx.x * PROP_BLOCK + threadIdx.x;
    const bool on = k < nthreads;
    const int id = k + offset;
    LaneCounters cnt = {0, 0, 0, 0, 0};
    const v3 position = mk3(px, py, pz);
    cm_rng rng;
    v3 v0, v1, v2, direction = mk3(0.0f, 0.0f, 1.0f);
    if (on) {
        cm_rng_init(&rng, seed, id_base + (uint64_t)k, rng_counters[k]);
        const float4 *t = g.tri + TRI_STRIDE * (size_t)g.tri_to_dev[id];
        const float4 a4 = t[0], b4 = t[1], c4 = t[2];
        v0 = mk3(a4.x, a4.y, a4.z);
        v1 = mk3(b4.x, b4.y, b4.z);
        v2 = mk3(c4.x, c4.y, c4.z);
        float a = rng_u(rng);
        float b = uniform(rng, 0.0f, 1.0f - a);
        float c = 1.0f - a - b;
        direction = a * v0 + b * v1 + c * v2 - position;
        direction = direction / norm(direction);
    }
    float distance;
    const int first = intersect_mesh<LDS_N, PROP_BLOCK, false>(g, position, direction, distance, -1, lds, cnt, on);
    const bool mine = on && first == id;

    Photon p;
    float cos_theta = 0.0f;
    if (mine) {
        const v3 surface_normal = triangle_normal(v0, v1, v2);
        cos_theta = dot(surface_normal, -direction);
        if (cos_theta < 0.0f) cos_theta = dot(-surface_normal, -direction);
        p.position = position;
        p.direction = direction;
        p.wavelength = wavelength;
        p.polarization = uniform_sphere(rng);
        p.last_hit_triangle = -1;
        p.time = 0.0f;
        p.history = 0;
        p.weight = 1.0f;
        p.evidx = 0;
    }
    const bool inside_to_outside = to_diffuse<LDS_N>(p, rng, g, max_steps, mine, lds, cnt);

    if (on) {
        rng_counters[k] = rng.counter;
        const bool diffuse = mine && (p.history & CHROMA_REFLECT_DIFFUSE);
        const uint32_t side = inside_to_outside ? 1u : 0u;
        keys[k] = diffuse ? 2u * (uint32_t)p.last_hit_triangle + side : key_none;
        ids[k] = (uint32_t)k;
        store3(values, (size_t)k, mk3(cos_theta * xr, cos_theta * xg, cos_theta * xb));
        if (s_tri) {
            s_tri[k] = diffuse ? p.last_hit_triangle : -1;
            s_side[k] = diffuse ? side : 0u;
            s_history[k] = mine ? p.history : 0u;
            s_cos[k] = cos_theta;
        }
    }
    flush_counters<false, FLUSH_OVERFLOWS>(cnt, counters, lane_id());
}

// The lookup records of one k_hybrid_lookup launch, stably sorted by key (sample order within a key): the first record
// of each key sums its key's values in sample order in f32, then adds the sum once to the entry (key & 1: lookup1,
// inside to outside, else lookup2; triangle key >> 1).  The same bits on every run.
__global__ __launch_bounds__(256) void
k_hybrid_reduce(int n, const uint32_t *sorted_keys, const uint32_t *order, const float *values, uint32_t key_none,
                float *lookup1, float *lookup2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = sorted_keys[i];
    if (key >= key_none || (i > 0 && sorted_keys[i - 1] == key)) return;
    v3 sum = load3(values, order[i]);
    for (int m = i + 1; m < n && sorted_keys[m] == key; m++) sum = sum + load3(values, order[m]);
    float *lookup = (key & 1u) ? lookup1 : lookup2;
    const size_t t = key >> 1;
    store3(lookup, t, load3(lookup, t) + sum);
}

// update_xyz_image (hybrid_render.cu:133-168): ray k from the camera to its first diffuse reflection, then
// image[k] += xyz * lookup[triangle] / nlookup_calls in the reference's float3 order.  One thread per ray: no contention.
// Random stream and sample outputs as k_hybrid_lookup's.
template <int LDS_N>
__global__ __launch_bounds__(PROP_BLOCK) void
k_hybrid_image(GeoView g, int nthreads, uint64_t seed, uint64_t id_base, uint32_t *rng_counters, const float *positions,
               const float *directions, float wavelength, float xr, float xg, float xb, const float *lookup1,
               const float *lookup2, float *image, int nlookup_calls, int max_steps, int32_t *s_tri, uint32_t *s_side,
               uint32_t *s_history, DeviceCounters *counters)
{
    __shared__ uint32_t s_lds[TRAV_LDS_WORDS(LDS_N, PROP_BLOCK)];
    uint32_t *lds = s_lds + threadIdx.x;

    const int k = blockIdx.x * PROP_BLOCK + threadIdx.x;
    const bool on = k < nthreads;
    LaneCounters cnt = {0, 0, 0, 0, 0};
    cm_rng rng;
    Photon p;
    if (on) {
        cm_rng_init(&rng, seed, id_base + (uint64_t)k, rng_counters[k]);
        p.position = load3(positions, (size_t)k);
        p.direction = load3(directions, (size_t)k);
        p.direction = p.direction / norm(p.direction);
        p.wavelength = wavelength;
        p.polarization = uniform_sphere(rng);
        p.last_hit_triangle = -1;
        p.time = 0.0f;
        p.history = 0;
        p.weight = 1.0f;
        p.evidx = 0;
    }
    const bool inside_to_outside = to_diffuse<LDS_N>(p, rng, g, max_steps, on, lds, cnt);

    if (on) {
        rng_counters[k] = rng.counter;
        const bool diffuse = (p.history & CHROMA_REFLECT_DIFFUSE) != 0;
        if (diffuse) {
            const v3 l = load3(inside_to_outside ? lookup1 : lookup2, (size_t)p.last_hit_triangle);
            const float n = (float)nlookup_calls;
            store3(image, (size_t)k, load3(image, (size_t)k) + mk3(xr * l.x, xg * l.y, xb * l.z) / n);
        }
        if (s_tri) {
            s_tri[k] = diffuse ? p.last_hit_triangle : -1;
            s_side[k] = diffuse ? (inside_to_outside ? 1u : 0u) : 0u;
            s_history[k] = p.history;
        }
    }
    flush_counters<false, FLUSH_OVERFLOWS>(cnt, counters, lane_id());
}

// process_image (hybrid_render.cu:170-201): image / nimages, clamped to [0, 1] (NaN to 0), floorf(x * 255), packed
// 0xFF << 24 | r << 16 | g << 8 | b.
__device__ inline uint32_t hybrid_channel(float x)
{
    if (!(x >= 0.0f)) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    return (uint32_t)floorf(x * 255.0f);
}
__global__ __launch_bounds__(256) void
k_hybrid_pixels(int nthreads, const float *image, uint32_t *pixels, int nimages)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nthreads) return;
    const v3 rgb = load3(image, (size_t)k) / (float)nimages;
    pixels[k] = 0xFFu << 24 | hybrid_channel(rgb.x) << 16 | hybrid_channel(rgb.y) << 8 | hybrid_channel(rgb.z);
}
