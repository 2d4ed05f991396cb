// kernels_distance.h -- the kernels of chroma_intersect_mesh / chroma_distance_to_mesh: the lane-per-ray reference walk, and the
// fast path through k_raycast_quad (ray records from the caller's arrays, the check of its results, the strict walk for the rest).
// One of the kernel families of libchroma_hip.so; included by chroma_hip.hip alone, so that each kernel is compiled once.
#pragma once

// distance_to_mesh (chroma/cuda/mesh.h:124-151)
template <int LDS_N, bool COUNT>
__global__ __launch_bounds__(PROP_BLOCK) void
k_distance_to_mesh(GeoView g, int nthreads, const float *origin, const float *direction, const int32_t *last_hit_in,
                   float *distance_out, int32_t *triangle_out, DeviceCounters *counters)
{
    __shared__ uint32_t s_lds[TRAV_LDS_WORDS(LDS_N, PROP_BLOCK)];
    int id = blockIdx.x * PROP_BLOCK + threadIdx.x;
    LaneCounters cnt = {0, 0, 0, 0};
    bool on = id < nthreads;
    v3 o = mk3(0.f, 0.f, 0.f), d = mk3(0.f, 0.f, 1.f);
    if (on) {
        o = load3(origin, id);
        d = load3(direction, id);
        d = d / norm(d);
    }
    float dist;
    int last_hit = (on && last_hit_in) ? last_hit_in[id] : -1;
    if ((uint32_t)last_hit >= g.ntriangles) last_hit = -1;   // an id outside the mesh excludes nothing (as k_rays_from_arrays)
    int tri = intersect_mesh<LDS_N, PROP_BLOCK, COUNT>(g, o, d, dist, last_hit, s_lds + threadIdx.x, cnt, on);
    if (on) {
        if (tri != -1) distance_out[id] = dist;
        if (triangle_out) triangle_out[id] = tri;
    }
    flush_counters<COUNT, FLUSH_OVERFLOWS>(cnt, counters, lane_id());
}

// ---- distance_to_mesh through the fast ray cast --------------------------------------------------------
// mesh.h:124-151 asks for the nearest triangle along free rays.  Same pipeline as a propagation step:
// ray records, k_raycast_quad, the check that the reference tests the winner (record_hit_is_regular),
// the literal reference walk for the rays that fail it or that the fast walk cannot take.
__global__ void k_rays_from_arrays(GeoView g, int n, const float *origin_in, const float *direction_in, const int32_t *last_hit_in,
                                   float4 *rays, int32_t *hit_triangle, float *hit_distance, uint32_t *retry_list, StepState *st)
{
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    int last_hit = last_hit_in ? last_hit_in[slot] : -1;          // a triangle id (mesh.h:82) -> its record
    last_hit = (last_hit >= 0 && (uint32_t)last_hit < g.ntriangles) ? (int)g.tri_to_dev[last_hit] : -1;
    v3 origin = load3(origin_in, slot), direction = load3(direction_in, slot);
    direction = direction / norm(direction);
    v3 noid = (-origin) / direction;
    v3 inv_dir = 1.0f / direction;
    bool moderate = cm_fabsf(inv_dir.x) < 1e30f && cm_fabsf(inv_dir.y) < 1e30f && cm_fabsf(inv_dir.z) < 1e30f &&
                    cm_fabsf(noid.x) < 1e30f && cm_fabsf(noid.y) < 1e30f && cm_fabsf(noid.z) < 1e30f;
    int status = moderate ? 0 : HIT_RETRY;                 // (a NaN ray is not moderate: the literal walk answers)
    v3 a = mk3(0.f, 0.f, 0.f), b = mk3(0.f, 0.f, 0.f);
    if (moderate) {
        a = ray_fast(g, noid, inv_dir, 1.0f).a;
        b = mk3(cm_fmaf(g.world_origin[0], inv_dir.x, noid.x), cm_fmaf(g.world_origin[1], inv_dir.y, noid.y),
                cm_fmaf(g.world_origin[2], inv_dir.z, noid.z));
    }
    RayRecord(origin, last_hit, direction, status, a, ray_growth(g, origin), b).store(rays + 4 * (size_t)slot);
    if (status != 0) settle_ray(status, slot, hit_triangle, hit_distance, retry_list, &st->retry);
}
__global__ void k_step_set(StepState *st, uint32_t n) { st->n = n; st->renorm = 0u; st->in_tail = 0u; st->launches = 0u; st->work = 0u; st->retry = 0u; }

// results of the fast cast: checked, translated to triangle ids, or handed to the literal walk
__global__ void k_distance_finish(GeoView g, int n, const float4 *rays, const int32_t *hit_triangle, const float *hit_distance,
                                  float *distance_out, int32_t *triangle_out, uint32_t *retry_list, StepState *st)
{
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    int rec = hit_triangle[slot];
    if (rec == HIT_RETRY) return;                          // already listed
    if (rec >= 0) {
        const float4 *r = rays + 4 * (size_t)slot;
        const float4 r0 = r[0], r1 = r[1];
        const float4 *t = g.tri + TRI_STRIDE * (size_t)rec;
        const float4 a = t[0], b = t[1], c = t[2];
        const float dist = hit_distance[slot];
        if (!record_hit_is_regular(g, a, b, c, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), dist)) {
            retry_list[atomicAdd(&st->retry, 1u)] = (uint32_t)slot;
            return;
        }
        distance_out[slot] = dist;
        if (triangle_out) triangle_out[slot] = (int32_t)__float_as_uint(b.w);
    } else if (triangle_out) {
        triangle_out[slot] = -1;                           // a miss leaves the distance untouched (mesh.h:145-148)
    }
}
template <bool COUNT>
__global__ __launch_bounds__(PROP_BLOCK) void
k_distance_retry(GeoView g, const float4 *rays, const StepState *st, const uint32_t *retry_list, float *distance_out,
                 int32_t *triangle_out, DeviceCounters *counters)
{
    __shared__ uint32_t s_lds[TRAV_LDS_WORDS(STACK_LDS, PROP_BLOCK)];
    const int nretry = (int)st->retry;
    LaneCounters cnt = {0, 0, 0, 0};
    for (int k = blockIdx.x * PROP_BLOCK + threadIdx.x; k < nretry; k += gridDim.x * PROP_BLOCK) {
        const int slot = (int)retry_list[k];
        const float4 *r = rays + 4 * (size_t)slot;
        const float4 r0 = r[0], r1 = r[1];
        float dist;
        int rec = intersect_mesh_dev<STACK_LDS, PROP_BLOCK, COUNT>(g, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), dist,
                                                                   __float_as_int(r0.w), s_lds + threadIdx.x, cnt, true);
        if (rec >= 0) distance_out[slot] = dist;
        if (triangle_out) triangle_out[slot] = rec >= 0 ? (int32_t)g.dev_to_tri[rec] : -1;
    }
    flush_counters<COUNT, FLUSH_OVERFLOWS>(cnt, counters, lane_id());
}
