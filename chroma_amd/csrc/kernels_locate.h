// kernels_locate.h -- the kernels of chroma_locate_materials around the ray cast of chroma_intersect_mesh (kernels_distance.h):
// the ray records of n points that share ONE probe direction, and the material each point lies in from its ray's hit.
// One of the kernel families of libchroma_hip.so; included by chroma_hip.hip alone, so that each kernel is compiled once.
#pragma once

// k_rays_from_arrays with the direction as a kernel argument and no last hit: the record chroma_intersect_mesh forms for the
// ray (points[slot], direction), operation for operation, so that the cast and its triangle are that call's.  No [n][3]
// direction array exists anywhere.
__global__ void k_locate_rays(GeoView g, int n, const float *points, float dx, float dy, float dz, float4 *rays, int32_t *hit_triangle,
                              float *hit_distance, uint32_t *retry_list, StepState *st)
{
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    v3 origin = load3(points, slot), direction = mk3(dx, dy, dz);
    direction = direction / norm(direction);
    v3 noid = (-origin) / direction;
    v3 inv_dir = 1.0f / direction;
    bool moderate = cm_fabsf(inv_dir.x) < 1e30f && cm_fabsf(inv_dir.y) < 1e30f && cm_fabsf(inv_dir.z) < 1e30f &&
                    cm_fabsf(noid.x) < 1e30f && cm_fabsf(noid.y) < 1e30f && cm_fabsf(noid.z) < 1e30f;
    int status = moderate ? 0 : HIT_RETRY;                 // (an axis-parallel probe, the default one: the literal walk answers)
    v3 a = mk3(0.f, 0.f, 0.f), b = mk3(0.f, 0.f, 0.f);
    if (moderate) {
        a = ray_fast(g, noid, inv_dir, 1.0f).a;
        b = mk3(cm_fmaf(g.world_origin[0], inv_dir.x, noid.x), cm_fmaf(g.world_origin[1], inv_dir.y, noid.y),
                cm_fmaf(g.world_origin[2], inv_dir.z, noid.z));
    }
    RayRecord(origin, -1, direction, status, a, ray_growth(g, origin), b).store(rays + 4 * (size_t)slot);
    if (status != 0) settle_ray(status, slot, hit_triangle, hit_distance, retry_list, &st->retry);
}

// The lane-per-ray walk (k_distance_to_mesh) for a context whose walk does not go through the ray records
template <int LDS_N, bool COUNT>
__global__ __launch_bounds__(PROP_BLOCK) void
k_locate_walk(GeoView g, int n, const float *points, float dx, float dy, float dz, int32_t *triangle_out, DeviceCounters *counters)
{
    __shared__ uint32_t s_lds[TRAV_LDS_WORDS(LDS_N, PROP_BLOCK)];
    int id = blockIdx.x * PROP_BLOCK + threadIdx.x;
    LaneCounters cnt = {0, 0, 0, 0};
    bool on = id < n;
    v3 o = on ? load3(points, id) : mk3(0.f, 0.f, 0.f), d = mk3(dx, dy, dz);
    d = d / norm(d);
    float dist;
    int tri = intersect_mesh<LDS_N, PROP_BLOCK, COUNT>(g, o, d, dist, -1, s_lds + threadIdx.x, cnt, on);
    if (on) triangle_out[id] = tri;
    flush_counters<COUNT, FLUSH_OVERFLOWS>(cnt, counters, lane_id());
}

// fill_state's choice of material1 (photon.h:99-120; apply_hit_normal, propagate_device.h) for the triangle the cast found:
// the stored unit normal and the material code come from the triangle's 32-byte physics record, one aligned sector.
__global__ void k_locate_material(GeoView g, int n, const int32_t *triangle, float dx, float dy, float dz, int32_t outside,
                                  int32_t *material)
{
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const int tri = triangle[slot];
    if (tri < 0 || (uint32_t)tri >= g.ntriangles) { material[slot] = outside; return; }
    v3 direction = mk3(dx, dy, dz);
    direction = direction / norm(direction);
    const TriPhys r = load_tri_phys(g, (size_t)g.tri_to_dev[tri]);
    const uint32_t inner = 0xFF & (r.code >> 24), outer = 0xFF & (r.code >> 16);
    material[slot] = (int32_t)((dot(r.normal, -direction) > 0.0f) ? outer : inner);
}
