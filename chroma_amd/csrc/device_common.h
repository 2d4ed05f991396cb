// device_common.h -- device-side types shared by the HIP kernels of libchroma_hip.so: float3 algebra, the geometry and photon
// views, the 64-byte photon record (PhotonRecord) and what stores a photon back (store_photon), wave and block helpers.
//
// Written for gfx950 (CDNA4) only: 64-wide wavefronts, one photon per lane.
// Arithmetic follows include/chroma_math.h (the numeric contract) and is compiled with
// -ffp-contract=off so that the CPU oracle reproduces every result bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define CM_FN __host__ __device__ static inline
#include "../../include/chroma_math.h"
#include "../../include/chroma_hip.h"

#define WAVE 64

// two floats in one register pair: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 do the same IEEE operation on each half
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- float3 algebra (operation order as chroma/cuda/linalg.h) -------------------------
struct v3 { float x, y, z; };
__device__ inline v3 mk3(float x, float y, float z) { return v3{x, y, z}; }
__device__ inline v3 operator-(v3 a) { return mk3(-a.x, -a.y, -a.z); }
__device__ inline v3 operator+(v3 a, v3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline v3 operator-(v3 a, v3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline v3 operator*(v3 a, float c) { return mk3(a.x * c, a.y * c, a.z * c); }
__device__ inline v3 operator*(float c, v3 a) { return mk3(c * a.x, c * a.y, c * a.z); }
__device__ inline v3 operator/(v3 a, float c) { return mk3(a.x / c, a.y / c, a.z / c); }
__device__ inline v3 operator/(v3 a, v3 b) { return mk3(a.x / b.x, a.y / b.y, a.z / b.z); }
__device__ inline v3 operator/(float c, v3 a) { return mk3(c / a.x, c / a.y, c / a.z); }
__device__ inline float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline v3 cross(v3 a, v3 b)
{ return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ inline float norm(v3 a) { return cm_sqrtf(dot(a, a)); }
__device__ inline v3 normalize(v3 a) { return a / norm(a); }

__device__ inline v3 load3(const float *p, size_t i) { return mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ inline void store3(float *p, size_t i, v3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

// interp (interpolate.h:32-57) as used by sample_cdf(rng, n, cdf_x, cdf_y) (random.h:26-31): the DAQ kernels' draws (kernels_daq.h,
// kernels_daq_pulses.h) and k_probe (kernels_render.h)
__device__ inline float interp_table(float x, int n, const float *xp, const float *fp)
{
    int lower = 0;
    int upper = n - 1;
    if (x <= xp[lower]) return fp[lower];
    if (x >= xp[upper]) return fp[upper];
    while (lower < upper - 1) {
        int half = (lower + upper) / 2;
        if (x < xp[half]) upper = half; else lower = half;
    }
    float df = fp[upper] - fp[lower];
    float dx = xp[upper] - xp[lower];
    return fp[lower] + df * (x - xp[lower]) / dx;
}

// ---- device view of an uploaded geometry ------------------------------------------------
// Layout in HBM (see DESIGN.md "Data layout"):
//   nodes   uint4[nnodes]            16 B packed node, as chroma/cuda/geometry_types.h:57-67
//   wnodes  uint4[nwide][8]          128 B wide node = one L2 line: eight child entries in the node
//                                    format above, w = child wide node | 0x80000000+device triangle
//                                    | 0xFFFFFFFF (empty); derived from `nodes` (csrc/wide_build.cpp)
//   tri     float4[nrecords][3]      48 B record: v0.xyz|material_code, v1.xyz|triangle id, v2.xyz|rank
//                                    (one aligned 48-B gather instead of the reference's
//                                     12-B index fetch + three 12-B vertex gathers).  `rank` is the
//                                    triangle's position in the reference's test order (tie-break of
//                                    the wide walk).  Records are stored in the order the wide tree
//                                    lists its triangles, not in triangle-id order: the triangles of
//                                    one wide node -- tested together -- sit in adjacent 128-B lines.
//                                    Both trees hold that "device" index in their leaves;
//                                    tri_to_dev / dev_to_tri translate at ray start and end.
//   tri_isect float4[nrecords][3]    48 B intersection record, in record order: {e1.x, e2.x, e1.y, e2.y}
//                                    {e1.z, e2.z, v0.x, v0.y} {v0.z, rank, 0, 0} with e1 = v1 - v0, e2 = v2 - v0.
//                                    What the fast walks' Moeller-Trumbore reads (intersect_triangle_edges): the
//                                    edges computed once instead of in every test, and every packed operand of
//                                    the test an aligned register pair straight from the three 16-B loads
//   tri_phys uint4[nrecords][2]      32 B physics record, in record order: {unit normal.xyz, material code}
//                                    {triangle id, leaf words x, y, z}.  What k_physics needs of the winning
//                                    triangle -- one aligned 32-B sector instead of the 48-B record, and the
//                                    normal and leaf box computed once instead of on every step (TriPhys)
//   tables  float[...]               optics tables, row-major [row][wavelength_n]
struct SurfaceInfo { uint32_t model; uint32_t transmissive; float thickness; int32_t dichroic_index; };

// float4s per triangle record: {v0, material code} {v1, triangle id} {v2, rank}.  4 pads a record to
// 64 bytes, so that none straddles two 128-byte lines (a quarter of the 48-byte ones do).
#ifndef TRI_STRIDE
#define TRI_STRIDE 3
#endif
struct GeoView {
    const uint4  *nodes;             // traversal copy: leaf child = device triangle index
    const uint4  *wnodes;            // derived 8-wide tree, 8 entries (128 B) per node
    const float4 *tri;               // [device triangle index][3]
    const float4 *tri_isect;         // [device triangle index][3]: the intersection record (intersect_triangle_edges)
    const uint4  *tri_phys;          // [device triangle index][2]: the physics record (TriPhys)
    const uint32_t *tri_to_dev, *dev_to_tri;
    // materials
    const float *mat_refractive_index, *mat_absorption_length, *mat_scattering_length;
    const uint32_t *mat_num_comp, *mat_comp_offset;
    const float *comp_reemission_prob, *comp_reemission_wvl_cdf, *comp_absorption_length, *comp_reemission_time_cdf;
    // surfaces
    const float *surf_detect, *surf_absorb, *surf_reemit, *surf_reflect_diffuse, *surf_reflect_specular,
                *surf_eta, *surf_k, *surf_reemission_cdf;
    const SurfaceInfo *surf_info;
    const uint32_t *dichroic_nangles, *dichroic_offset;
    const float *dichroic_angles, *dichroic_reflect, *dichroic_transmit;
    // hits
    const uint32_t *solid_id_map;
    const int32_t  *solid_id_to_channel_index;
    float world_origin[3];
    float world_scale;
    float suspect_margin;            // see record_hit_is_regular (propagate_device.h)
    float slab_grow;                 // quanta by which the fast slab test grows a box on every side (ray_growth, propagate_device.h)
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    uint32_t nnodes, ntriangles, nsolids, nchannels, nwide;
    uint32_t plain_optics;           // no re-emitting material component, every surface of the default model
};

// the physics record of a triangle, as k_physics reads it: normalize(cross(v1 - v0, v2 - v1)) (fill_state's
// expression), the material code, the triangle id, and the leaf box by the reference's rule (leaf_words,
// propagate_device.h); written by k_triangle_phys at geometry creation
struct TriPhys { v3 normal; uint32_t code, id, bx, by, bz; };
__device__ inline TriPhys load_tri_phys(const GeoView &g, size_t record)
{
    const uint4 *r = g.tri_phys + 2 * record;
    const uint4 a = r[0], b = r[1];
    return TriPhys{mk3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)), a.w, b.x, b.y, b.z, b.w};
}

struct PhotonView {   // device pointers of chroma_photon_arrays
    float *pos, *dir, *pol, *wavelengths, *t;
    uint32_t *flags; int32_t *last_hit_triangles; float *weights; uint32_t *evidx; uint32_t *rng_counters;
};

struct DeviceCounters {   // accumulated with one atomic per wave
    unsigned long long photon_steps, nodes_visited, triangles_tested, stack_overflows;
    unsigned long long stack_spills;   // stack entries a fast walk pushed beyond its LDS part (counting builds)
    unsigned long long packet_rays, packet_nodes, packet_tris;      // k_raycast_packet's share of the two counts above (counting builds)
};

// the device-side step control block of chroma_propagate (k_step_begin, kernel_step_control.h)
struct StepState {
    uint32_t n;          // photons queued for this step
    uint32_t renorm;     // this step opens a launch in the reference's sense: re-normalise dir/pol on load
    uint32_t in_tail;    // the reference's last launch (all remaining steps) has begun
    uint32_t launches;   // launches in the reference's sense so far
    uint32_t work;       // next unclaimed ray of the persistent ray cast
    uint32_t retry;      // rays left for k_raycast_retry
    uint32_t pad[2];
};

// ---- hits ---------------------------------------------------------------------------------------------------------
// the channel a photon was detected on, or -1 (propagate.cu:157-171: the flag, a last hit triangle, a solid with a channel)
__device__ inline int hit_channel(const GeoView &g, uint32_t history, int triangle_id, uint32_t detection_state)
{
    if (!(history & detection_state)) return -1;
    if (triangle_id <= -1) return -1;
    uint32_t solid_id = g.solid_id_map[triangle_id];
    return g.solid_id_to_channel_index[solid_id];
}

// where the hits of a chroma_propagate_hits call go (k_finalize_hits, and k_tail_coop for the photons it finishes)
struct HitsOut {
    PhotonView dst; int32_t *channels; uint32_t capacity;
    uint32_t *hit_count, *earliest;
    uint32_t detection_state; int want;
};

// a photon in registers (chroma/cuda/photon.h:12-27)
struct Photon {
    v3 position, direction, polarization;
    float wavelength, time, weight;
    uint32_t history;
    int last_hit_triangle;
    uint32_t evidx;
};

// ---- the photon record --------------------------------------------------------------------------------------------
// A photon outside the caller's arrays: 64 bytes, four float4 rows ("working set" and "final records")
//   {position, wavelength} {direction, time} {polarization, weight} {flags, draw counter, last hit, tag}
// The LAST HIT word (row 3, .z) is
//   - the index of a triangle RECORD (GeoView::tri, -1: none) in a working-set record: what the next ray cast skips;
//   - a triangle ID (-1: none) in a final record: what the caller's last_hit_triangles gets.
// The TAG (row 3, .w) is
//   - the photon id, in a working-set record (the record sits at its queue slot);
//   - the call's epoch, in a final record (the record sits at its photon id; k_physics, chroma_propagate_hits only);
//   - photon_tail_stamp(epoch) = epoch | 0x80000000, on the final-record slot of a photon k_tail_coop is about to finish
//     (k_mark_tail): k_finalize_hits, which runs beside the tail kernel, leaves such a photon to it.
// Used by k_load_working, k_ray_setup and k_mark_tail.  k_physics, k_physics_deal, k_tail_coop, k_store_working and
// k_finalize_hits still pick the rows apart by hand, in this layout: taken through the struct they compile to other
// registers, scratch or occupancy (profiles/r09/INDEX.md).
CM_FN uint32_t photon_tail_stamp(uint32_t epoch) { return epoch | 0x80000000u; }

struct PhotonRecord {
    float4 row[4];

    PhotonRecord() = default;
    __device__ inline PhotonRecord(const Photon &p, uint32_t draw_counter, int last_hit, uint32_t tag)
    {
        row[0] = make_float4(p.position.x, p.position.y, p.position.z, p.wavelength);
        row[1] = make_float4(p.direction.x, p.direction.y, p.direction.z, p.time);
        row[2] = make_float4(p.polarization.x, p.polarization.y, p.polarization.z, p.weight);
        row[3] = make_float4(__uint_as_float(p.history), __uint_as_float(draw_counter), __int_as_float(last_hit), __uint_as_float(tag));
    }
    __device__ static inline PhotonRecord load(const float4 *r) { PhotonRecord rec; rec.row[0] = r[0]; rec.row[1] = r[1]; rec.row[2] = r[2]; rec.row[3] = r[3]; return rec; }
    __device__ inline void store(float4 *r) const { r[0] = row[0]; r[1] = row[1]; r[2] = row[2]; r[3] = row[3]; }
    // row 3 of a record nothing else is known of: the stamp of k_mark_tail
    __device__ static inline void store_tag(float4 *r, uint32_t tag) { r[3] = make_float4(0.f, 0.f, 0.f, __uint_as_float(tag)); }

    // (accessors for what a caller reads today; the other words get theirs with the first kernel that reads them through the struct)
    __device__ inline v3 position() const { return mk3(row[0].x, row[0].y, row[0].z); }
    __device__ inline v3 direction() const { return mk3(row[1].x, row[1].y, row[1].z); }
    __device__ inline int last_hit() const { return __float_as_int(row[3].z); }
};

// a photon goes back to the caller's arrays (evidx is the caller's own: no kernel of a step changes it)
__device__ inline void store_photon(const PhotonView &pv, size_t id, const Photon &p, uint32_t draw_counter)
{
    pv.rng_counters[id] = draw_counter;
    store3(pv.pos, id, p.position);
    store3(pv.dir, id, p.direction);
    store3(pv.pol, id, p.polarization);
    pv.wavelengths[id] = p.wavelength;
    pv.t[id] = p.time;
    pv.flags[id] = p.history;
    pv.last_hit_triangles[id] = p.last_hit_triangle;
    pv.weights[id] = p.weight;
}

__device__ inline void copy_photon(const PhotonView &src, size_t i, const PhotonView &dst, size_t o)
{
    store3(dst.pos, o, load3(src.pos, i));
    store3(dst.dir, o, load3(src.dir, i));
    store3(dst.pol, o, load3(src.pol, i));
    dst.wavelengths[o] = src.wavelengths[i];
    dst.t[o] = src.t[i];
    dst.flags[o] = src.flags[i];
    dst.last_hit_triangles[o] = src.last_hit_triangles[i];
    dst.weights[o] = src.weights[i];
    dst.evidx[o] = src.evidx[i];
    if (dst.rng_counters && src.rng_counters) dst.rng_counters[o] = src.rng_counters[i];
}

// photons a thread of k_copy_hits / k_finalize_hits looks at (blocks of 256 threads)
#define COPY_ITEMS 16

// ---- wave-level helpers --------------------------------------------------------------------
__device__ inline unsigned lane_id() { return __lane_id(); }

// Append `value` for every lane with pred set: one atomic per wave, lanes keep their order.
// queue[0] is the tail index (initially 1), as chroma/cuda/propagate.cu:315-318.
__device__ inline void wave_queue_append(uint32_t *queue, bool pred, uint32_t value)
{
    unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return;
    unsigned lane = lane_id();
    unsigned leader = (unsigned)__ffsll((long long)mask) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(queue, (uint32_t)__popcll(mask));
    base = __shfl(base, (int)leader);
    if (pred) {
        unsigned rank = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
        queue[base + rank] = value;
    }
}

// Block-level variant: one atomic per BLOCK (a hot word takes only ~88 atomics/us, so one per
// wave is too many for 1e8 photons).  Waves publish their counts in LDS, wave 0 reserves the
// block's span, every lane then writes at its own offset.  All threads of the block must call it.
template <int MAX_WAVES>
__device__ inline uint32_t block_queue_append(uint32_t *queue, bool pred, uint32_t value, uint32_t *s_counts /* [MAX_WAVES+1] */)
{
    unsigned long long mask = __ballot(pred);
    unsigned lane = lane_id();
    unsigned wave = threadIdx.x / WAVE, nwaves = (blockDim.x + WAVE - 1) / WAVE;
    if (lane == 0) s_counts[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (unsigned w = 0; w < nwaves; w++) { uint32_t c = s_counts[w]; s_counts[w] = total; total += c; }
        s_counts[MAX_WAVES] = total ? atomicAdd(queue, total) : 0u;
    }
    __syncthreads();
    uint32_t at = 0;                       // position in the queue (>= 1) of this lane's entry, 0 if none
    if (pred) {
        at = s_counts[MAX_WAVES] + s_counts[wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        queue[at] = value;
    }
    return at;
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
