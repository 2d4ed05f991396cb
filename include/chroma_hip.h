/* chroma_hip.h -- C ABI of libchroma_hip.so, the MI355X (gfx950) photon-propagation engine.
 *
 * This is the drop-in boundary for chroma's propagate path.  In the reference the
 * boundary is PyCUDA: Python JIT-compiles the .cu files under chroma/cuda and launches kernels by
 * name (chroma/gpu/tools.py:14-54).  Every entry point below names the reference
 * kernel or host routine it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C: opaque handles, raw device/host pointers, sizes; no C++ or torch types.
 *   - every function returns 0 (CHROMA_OK) or a negative chroma error / positive
 *     hipError_t; chroma_last_error() returns a thread-local message.
 *   - "d_" arguments are device pointers obtained from chroma_malloc(); all other
 *     pointers are host pointers.
 *   - all work is issued on the context's stream; entry points that return values
 *     to the host synchronise that stream, the others are asynchronous.
 *   - photon arrays are structure-of-arrays exactly as chroma/cuda/propagate.cu:217-226
 *     takes them: float3 arrays are packed [n][3] floats (12-byte stride).
 */
#ifndef CHROMA_HIP_H
#define CHROMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHROMA_OK                 0
#define CHROMA_ERR_INVALID       -1   /* bad argument / shape mismatch             */
#define CHROMA_ERR_NO_DEVICE     -2   /* no usable HIP device                      */
#define CHROMA_ERR_STACK         -3   /* BVH needs a deeper traversal stack        */
#define CHROMA_ERR_INTERNAL      -4

/* History bits: chroma/cuda/photon.h:49-64 == chroma/event.py:5-17 */
#define CHROMA_NO_HIT            (1u << 0)
#define CHROMA_BULK_ABSORB       (1u << 1)
#define CHROMA_SURFACE_DETECT    (1u << 2)
#define CHROMA_SURFACE_ABSORB    (1u << 3)
#define CHROMA_RAYLEIGH_SCATTER  (1u << 4)
#define CHROMA_REFLECT_DIFFUSE   (1u << 5)
#define CHROMA_REFLECT_SPECULAR  (1u << 6)
#define CHROMA_SURFACE_REEMIT    (1u << 7)
#define CHROMA_SURFACE_TRANSMIT  (1u << 8)
#define CHROMA_BULK_REEMIT       (1u << 9)
#define CHROMA_CHERENKOV         (1u << 10)
#define CHROMA_SCINTILLATION     (1u << 11)
#define CHROMA_NAN_ABORT         (1u << 31)
/* chroma/cuda/propagate.cu:258,315 */
#define CHROMA_TERMINAL_MASK (CHROMA_NO_HIT | CHROMA_BULK_ABSORB | CHROMA_SURFACE_DETECT | \
                              CHROMA_SURFACE_ABSORB | CHROMA_NAN_ABORT)

/* surface models: chroma/cuda/geometry_types.h:22 */
#define CHROMA_SURFACE_DEFAULT  0
#define CHROMA_SURFACE_COMPLEX  1
#define CHROMA_SURFACE_WLS      2
#define CHROMA_SURFACE_DICHROIC 3

/* packed BVH node: chroma/cuda/geometry_types.h:57-59 */
#define CHROMA_CHILD_BITS  28
#define CHROMA_NCHILD_MASK 0xF0000000u

typedef struct chroma_ctx chroma_ctx;
typedef struct chroma_geometry chroma_geometry;

/* Flat, pointer-free description of a flattened geometry + BVH + optics tables.
 * Replaces the pointer-linked Material/Surface/DichroicProps/Geometry/Detector
 * structs assembled byte-by-byte by chroma/gpu/geometry.py:47-253 and
 * chroma/gpu/detector.py:17-40 (struct layouts chroma/cuda/geometry_types.h:4-82,
 * chroma/cuda/detector.h:4-22).  All pointers are HOST pointers; the library
 * copies what it needs.  Tables are row-major [index][wavelength_n]. */
typedef struct chroma_geometry_desc {
    /* mesh (chroma/gpu/geometry.py:191-209) */
    const float    *vertices;        /* [nvertices][3]                               */
    const uint32_t *triangles;       /* [ntriangles][3] vertex indices               */
    const uint32_t *material_codes;  /* [ntriangles] inner<<24|outer<<16|surface<<8  */
    const uint32_t *solid_id_map;    /* [ntriangles]                                 */
    const uint32_t *colors;          /* [ntriangles] or NULL                         */
    uint32_t nvertices, ntriangles;
    /* BVH (chroma/bvh/bvh.py, chroma/cuda/geometry.h:31-47) */
    const uint32_t *nodes;           /* [nnodes][4] packed x,y,z,w                   */
    uint32_t nnodes;
    float world_origin[3];
    float world_scale;
    /* common grids (chroma/gpu/geometry.py:15-30) */
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    /* materials (chroma/gpu/geometry.py:47-103) */
    uint32_t nmaterials;
    const float    *mat_refractive_index;   /* [nmaterials][wavelength_n] */
    const float    *mat_absorption_length;
    const float    *mat_scattering_length;
    const uint32_t *mat_num_comp;           /* [nmaterials]                          */
    const uint32_t *mat_comp_offset;        /* [nmaterials] first row in comp tables */
    uint32_t ncomp_total;
    const float    *comp_reemission_prob;     /* [ncomp_total][wavelength_n] */
    const float    *comp_reemission_wvl_cdf;  /* [ncomp_total][wavelength_n] */
    const float    *comp_absorption_length;   /* [ncomp_total][wavelength_n] */
    const float    *comp_reemission_time_cdf; /* [ncomp_total][time_n]       */
    /* surfaces (chroma/gpu/geometry.py:108-189); a None surface keeps its slot, zero-filled */
    uint32_t nsurfaces;
    const float    *surf_detect;            /* [nsurfaces][wavelength_n] each */
    const float    *surf_absorb;
    const float    *surf_reemit;
    const float    *surf_reflect_diffuse;
    const float    *surf_reflect_specular;
    const float    *surf_eta;
    const float    *surf_k;
    const float    *surf_reemission_cdf;
    const uint32_t *surf_model;             /* [nsurfaces] */
    const uint32_t *surf_transmissive;
    const float    *surf_thickness;
    const int32_t  *surf_dichroic_index;    /* [nsurfaces] index into dichroic tables or -1 */
    uint32_t ndichroic;
    const uint32_t *dichroic_nangles;       /* [ndichroic]                 */
    const uint32_t *dichroic_offset;        /* [ndichroic] first angle row */
    uint32_t ndichroic_angles_total;
    const float    *dichroic_angles;        /* [ndichroic_angles_total]                */
    const float    *dichroic_reflect;       /* [ndichroic_angles_total][wavelength_n]  */
    const float    *dichroic_transmit;      /* [ndichroic_angles_total][wavelength_n]  */
    /* detector part (chroma/gpu/detector.py:17-40); nsolids == 0 for a plain Geometry */
    const int32_t  *solid_id_to_channel_index; /* [nsolids] */
    uint32_t nsolids, nchannels;
    /* OPTIONAL: the derived traversal tree of `nodes`, as chroma_wide_build returned it for exactly
     * these nodes (a cache, or one process of a node building it for the others).  wide_nodes == NULL:
     * chroma_geometry_create derives it (16 s of all-core work at 170 M triangles).  A supplied tree goes
     * through the same index checks (chroma_wide_validate) before anything is uploaded. */
    const uint32_t *wide_nodes;             /* [nwide][8][4] */
    const uint32_t *wide_tri_to_record;     /* [ntriangles]  */
    const uint32_t *wide_record_to_tri;     /* [nrecords]    */
    const uint32_t *wide_rank;              /* [ntriangles]  */
    uint64_t nwide, nrecords;
} chroma_geometry_desc;

/* The nine photon arrays of chroma/cuda/propagate.cu:220-225 plus the per-photon
 * Philox draw counter that replaces curandState (propagate.cu:219,241,303). */
typedef struct chroma_photon_arrays {
    float    *pos;                 /* [n][3] mm          */
    float    *dir;                 /* [n][3]             */
    float    *pol;                 /* [n][3]             */
    float    *wavelengths;         /* [n] nm             */
    float    *t;                   /* [n] ns             */
    uint32_t *flags;               /* [n] history bits   */
    int32_t  *last_hit_triangles;  /* [n]                */
    float    *weights;             /* [n]                */
    uint32_t *evidx;               /* [n]                */
    uint32_t *rng_counters;        /* [n] uniforms already drawn by each photon */
} chroma_photon_arrays;

/* Replaces the curandState array from get_rng_states (chroma/gpu/tools.py:75-84):
 * the stream of photon i is Philox4x32-10 keyed by `seed`, indexed by
 * `photon_id_base + i` (see include/chroma_math.h). */
typedef struct chroma_rng {
    uint64_t seed;
    uint64_t photon_id_base;
} chroma_rng;

typedef struct chroma_propagate_stats {
    uint64_t photon_steps;       /* loop iterations that ran a ray cast (propagate.cu:264-275)  */
    uint64_t nodes_visited;      /* get_node calls in the child loop (cuda/mesh.h:75-76)        */
    uint64_t triangles_tested;   /* intersect_triangle calls (cuda/mesh.h:84-86)                */
    uint64_t launches;           /* propagate kernel launches                                   */
    uint64_t stack_overflows;    /* rays whose traversal stack overflowed (must be 0)           */
    double   kernel_ms;          /* HIP-event time of the propagate kernel launches, if timed   */
    double   raycast_ms;         /* of which: the ray-cast kernel (k_raycast_persistent)         */
    uint64_t raycast_launches;   /* number of ray-cast launches timed in raycast_ms              */
    uint64_t stack_spills;       /* stack entries pushed beyond the LDS part of a fast walk's stack
                                    (counting mode only; the deep-stack path of the 4- and 8-lane walks) */
    double   physics_ms;         /* HIP-event time of the main k_physics pass of every timed step            */
    uint64_t physics_launches;
    double   packet_ms;          /* HIP-event time of k_raycast_packet (the first step of a call with coherent photons);
                                    raycast_ms / raycast_launches then are k_raycast_quad's alone               */
    uint64_t packet_launches;
    uint64_t packet_rays, packet_nodes_visited, packet_triangles_tested;   /* counting mode: the packet kernel's share */
    uint64_t reordered;          /* photons of calls that took them up in direction order (chroma_set_autosort) */
} chroma_propagate_stats;

const char *chroma_last_error(void);
const char *chroma_version(void);

/* ---- context: replaces create_cuda_context (chroma/gpu/tools.py:121-142) ---- */
int chroma_device_count(int *count);
int chroma_init(int device, chroma_ctx **ctx);
int chroma_shutdown(chroma_ctx *ctx);
int chroma_synchronize(chroma_ctx *ctx);
int chroma_mem_info(chroma_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
int chroma_device_name(chroma_ctx *ctx, char *buf, size_t buflen);

/* ---- device memory: replaces pycuda.gpuarray allocation / get / set ---- */
int chroma_malloc(chroma_ctx *ctx, size_t nbytes, void **d_ptr);
int chroma_free(chroma_ctx *ctx, void *d_ptr);
/* (chroma_free parks the block in a pool and chroma_malloc reuses a parked block of the same size once the work that
 *  was queued when it was freed has completed: a GPUPhotons per event batch costs no hipMalloc / hipFree after the
 *  first.  chroma_pool_trim gives everything parked back to the device; chroma_pool_stats: bytes parked, allocations
 *  served from the pool, allocations that went to hipMalloc.) */
int chroma_pool_trim(chroma_ctx *ctx);
int chroma_pool_stats(chroma_ctx *ctx, uint64_t *parked_bytes, uint64_t *reused, uint64_t *allocated);
/* (copies of 8 MB and more are staged through pinned buffers by all host threads, piece by piece, DMA overlapping the
 *  staging of the next piece.)  Synchronous: ordered after the work queued on the context's stream. */
int chroma_memcpy_htod(chroma_ctx *ctx, void *d_dst, const void *h_src, size_t nbytes);
/* The same on the context's second stream -- NOT ordered with the queued work, so that the next event batch can be
 * uploaded (by another host thread) while the current one propagates: replaces the copies of GPUPhotons.__init__
 * (chroma/gpu/photon.py:13-94) in Simulation's batch loop (chroma/sim.py:58-139).  d_dst must not be in use by queued
 * work (a block fresh from chroma_malloc is not).  Returns when the data is on the device. */
int chroma_upload(chroma_ctx *ctx, void *d_dst, const void *h_src, size_t nbytes);
int chroma_memcpy_dtoh(chroma_ctx *ctx, void *h_dst, const void *d_src, size_t nbytes);
int chroma_memcpy_dtod(chroma_ctx *ctx, void *d_dst, const void *d_src, size_t nbytes);
int chroma_memset32(chroma_ctx *ctx, void *d_dst, uint32_t value, size_t count);

/* ---- geometry: replaces GPUGeometry.__init__ / GPUDetector.__init__ ---- */
int chroma_geometry_create(chroma_ctx *ctx, const chroma_geometry_desc *desc, chroma_geometry **geom);
int chroma_geometry_destroy(chroma_geometry *geom);
/* device pointers of the uploaded arrays, for the GPUGeometry attributes
 * (vertices, triangles, nodes, material_codes, colors, solid_id_map; gpu/geometry.py:191-209) */
int chroma_geometry_device_ptr(chroma_geometry *geom, const char *name, void **d_ptr, size_t *nbytes);
/* worst-case traversal stack entries this BVH can need (host-side tree walk) */
int chroma_geometry_stack_need(chroma_geometry *geom, uint32_t *entries);

/* ---- kernel-level entry points (one per reference kernel) ---- */

/* `propagate` (chroma/cuda/propagate.cu:217-319): up to max_steps steps for the photons
 * input_queue[first_photon .. first_photon+nthreads); survivors are appended to
 * d_output_queue (slot 0 = tail index, initial value 1, propagate.cu:315-318).
 * Asynchronous.  `stats` may be NULL; if given it is ACCUMULATED into on the next
 * synchronising call (chroma_propagate_stats_read). */
int chroma_propagate_step(chroma_ctx *ctx, chroma_geometry *geom,
                          int32_t first_photon, int32_t nthreads,
                          const uint32_t *d_input_queue, uint32_t *d_output_queue,
                          chroma_rng rng, const chroma_photon_arrays *photons,
                          int32_t max_steps, int32_t use_weights, int32_t scatter_first);

/* `photon_duplicate` (chroma/cuda/propagate.cu:13-52) */
int chroma_photon_duplicate(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                            const chroma_photon_arrays *photons, int32_t copies, int32_t stride);

/* `count_photons` + `copy_photons` (chroma/cuda/propagate.cu:54-114) */
int chroma_count_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                         uint32_t target_flag, const uint32_t *d_flags, uint32_t *count);
int chroma_copy_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                        uint32_t target_flag, const chroma_photon_arrays *src,
                        const chroma_photon_arrays *dst, uint32_t *ncopied);

/* `copy_photon_queue` (chroma/cuda/propagate.cu:116-144) */
int chroma_copy_photon_queue(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                             const uint32_t *d_queue, const chroma_photon_arrays *src,
                             const chroma_photon_arrays *dst);

/* `count_photon_hits` + `copy_photon_hits` (chroma/cuda/propagate.cu:147-214) */
int chroma_count_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon,
                             int32_t nphotons, uint32_t detection_state,
                             const chroma_photon_arrays *photons, uint32_t *count);
int chroma_copy_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon,
                            int32_t nphotons, uint32_t detection_state,
                            const chroma_photon_arrays *src, const chroma_photon_arrays *dst,
                            int32_t *d_channels, uint32_t *ncopied);

/* `distance_to_mesh` (chroma/cuda/mesh.h:124-151); d_triangle may be NULL.
 * Rays that miss leave d_distance untouched, as in the reference. */
int chroma_distance_to_mesh(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads,
                            const float *d_origin, const float *d_direction,
                            float *d_distance, int32_t *d_triangle);
/* The device function `intersect_mesh` (chroma/cuda/mesh.h:42-118) over a ray bundle, with its
 * `last_hit_triangle` argument: ray i never hits triangle d_last_hit[i] (mesh.h:82; NULL or -1: no
 * exclusion).  An id outside the mesh -- negative, or >= the number of triangles -- names no triangle and excludes
 * nothing, under every walk.  chroma_distance_to_mesh is this call with d_last_hit = NULL.  Same fast walk, check and
 * literal-walk fallback as a propagation step. */
int chroma_intersect_mesh(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads,
                          const float *d_origin, const float *d_direction, const int32_t *d_last_hit,
                          float *d_distance, int32_t *d_triangle);

/* Which material each point lies in, by the rule of the reference's `fill_state` (chroma/cuda/photon.h:99-120) for a photon
 * that would start at the point along `direction` (one probe direction for all points; NULL: (0, 0, 1)): the nearest
 * triangle along the ray, no last-hit exclusion; with normal = normalize(cross(v1 - v0, v2 - v1)), the point is in the
 * triangle's OUTER material ((code >> 16) & 0xFF) when dot(normal, -d) > 0 and in its INNER material ((code >> 24) & 0xFF)
 * otherwise -- the engine's own float arithmetic and strict comparison.  A point whose ray hits nothing gets `outside`.
 * d_triangle (may be NULL) receives the deciding triangle, -1 for none: exactly what chroma_intersect_mesh returns for the
 * same rays (the same ray-cast pipeline).  n == 0 does nothing; n < 0, a null pointer or a direction of no length is
 * CHROMA_ERR_INVALID.  Queued on the context's stream. */
int chroma_locate_materials(chroma_ctx *ctx, chroma_geometry *geom, int32_t n, const float *d_points,
                            const float direction[3], int32_t outside, int32_t *d_material, int32_t *d_triangle);

/* ---- fused host loops ---- */

/* GPUPhotons.propagate (chroma/gpu/photon.py:193-259) for n photons, whole loop on the
 * device side: queue ping-pong, survivor compaction, no per-step host copy of the photon
 * arrays.  ncopies/true_nphotons give the interleaved initial queue order of
 * photon.py:209-212.  Synchronises.  `stats` may be NULL.  `aborted` (may be NULL)
 * receives 1 if any photon carries NAN_ABORT afterwards (photon.py:254-255). */
int chroma_propagate(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons,
                     uint64_t nphotons, uint32_t ncopies, chroma_rng rng,
                     int32_t max_steps, int32_t use_weights, int32_t scatter_first,
                     int32_t time_kernels, chroma_propagate_stats *stats, int32_t *aborted);

/* propagate_hit in ONE call: chroma_propagate followed -- in the same pass that finishes the propagation -- by what the
 * reference does afterwards in separate kernels: the abort-flag reduction (chroma/gpu/photon.py:254-255), `count_photon_hits`
 * + `copy_photon_hits` (chroma/cuda/propagate.cu:147-214, GPUPhotons.get_flat_hits, chroma/gpu/photon.py:96-175) and the
 * per-channel hit count / earliest time of chroma_channel_hits.  Photons that end during the call travel as one 64-byte
 * record each and a single streaming kernel fills the caller's arrays from them while it extracts the hits; the arrays end up
 * exactly as chroma_propagate leaves them, and the flat hits are the SET chroma_copy_photon_hits would copy afterwards (their order
 * is unspecified, as in the reference: blocks of 4096 photons land in the order their atomics do) -- tests/test_gpu_hits.py.
 *   dst / d_channels   device arrays for up to `capacity` flat hits and their channels (both or neither)
 *   d_hit_count, d_earliest_time_bits   per-channel arrays (device, nchannels), ACCUMULATED into as by chroma_channel_hits;
 *                      d_hit_count may be NULL (then neither is touched), d_earliest_time_bits may be NULL
 *   nhits (out)        detected photons that belong to a channel; if it exceeds `capacity` only `capacity` of them were
 *                      written -- the photon arrays are final, chroma_copy_photon_hits with larger buffers gets all
 * A hits request is honoured for max_steps <= 0 too: no step is taken, the photon arrays stay as they are, and the photons detected
 * before the call are its hits (chroma_propagate followed by chroma_copy_photon_hits, for every max_steps).  Every flat hit carries
 * its photon's draw counter in dst->rng_counters when that array is given -- tests/test_gpu_hits_oracle.py. */
typedef struct chroma_hits_request {
    uint32_t detection_state;
    uint32_t capacity;
    const chroma_photon_arrays *dst;
    int32_t *d_channels;
    uint32_t *d_hit_count;
    uint32_t *d_earliest_time_bits;
    uint32_t nhits;
} chroma_hits_request;
int chroma_propagate_hits(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons,
                          uint64_t nphotons, uint32_t ncopies, chroma_rng rng,
                          int32_t max_steps, int32_t use_weights, int32_t scatter_first,
                          int32_t time_kernels, chroma_propagate_stats *stats, int32_t *aborted,
                          chroma_hits_request *hits);

/* The general form of the two calls above: what a call does is an ARGUMENT, not a setting of the context -- which walk the ray
 * cast takes (GPUPhotons.propagate(exact=True) passes CHROMA_WALK_LITERAL here), how the tail runs, whether the kernels count
 * their work.  A field of -1 takes the context's setting (chroma_set_walk / chroma_set_tail / chroma_set_counting or the CHROMA_*
 * environment) as it is when the call starts; nothing a concurrent call or setter does changes a call under way.  Every call
 * that uses the context's scratch (queues, working sets, result words, counters, settings) runs one at a time per context: two
 * threads may share a handle.
 * `hits` may be NULL (then this is chroma_propagate).  Zero the structure, then set what you need: reserved fields must be 0. */
typedef struct chroma_propagate_options {
    int32_t max_steps, use_weights, scatter_first, time_kernels;      /* as the arguments of chroma_propagate */
    int32_t walk;          /* CHROMA_WALK_* or -1 */
    int32_t tail;          /* CHROMA_TAIL_* or -1 */
    int32_t counting;      /* 0, 1 or -1 */
    int32_t reserved[5];
} chroma_propagate_options;
int chroma_propagate_opt(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons,
                         uint64_t nphotons, uint32_t ncopies, chroma_rng rng,
                         const chroma_propagate_options *options,
                         chroma_propagate_stats *stats, int32_t *aborted, chroma_hits_request *hits);

/* chroma_propagate_opt that also records every photon's TRACK, on the device (the reference's tracking mode,
 * chroma/gpu/photon.py:218-238 and chroma/sim.py:102-114): row 0 of a photon is its state before the first step, and every step
 * whose input queue holds it adds one row, its state after that step.  A photon that is terminal when the call starts is in the
 * first step's queue and left untouched: two equal rows (one when max_steps <= 0).  Rows carry pos, dir, pol, wavelengths, t,
 * flags, last_hit_triangles (a triangle id), weights and evidx.
 * As in the reference's tracking mode every step is a launch of its own, also with use_weights, so dir and pol are
 * re-normalised at every step (propagate.cu:248,250): the photons end as chroma_propagate_step driven with max_steps = 1 once
 * per step leaves them -- which is NOT what chroma_propagate gives for the last < 8192 photons of a call, whose steps share
 * one launch in the reference.  The call runs the split step loop (options->tail is taken as CHROMA_TAIL_SPLIT;
 * CHROMA_TAIL_FUSED, in the options or as the context's setting, is CHROMA_ERR_INVALID), with any walk, without final records,
 * and reads the survivor count after every step.
 * Refused before anything is launched: nphotons * (max_steps + 1) above 2^32-1 rows, nphotons * 2 rows (the least a call
 * with a step records) above $CHROMA_TRACKS_MAX_ROWS (CHROMA_ERR_INVALID), and no memory for rows 0, the row counts and the
 * first step's rows (64 bytes per photon each, from the pool of chroma_malloc).  How many rows the LATER steps add is known
 * only as they run: the rows of step k >= 1 are allocated when its photon count is known (64 bytes each), so a call can also
 * fail BETWEEN two steps, for lack of memory or because the rows would exceed $CHROMA_TRACKS_MAX_ROWS (default: 2^32-1; read
 * at every call).  It then stores the live photons back, returns the error and no tracks, and leaves the photon arrays
 * and draw counters exactly as the steps taken so far left them (the message says how many): a caller may go on from there.
 * *tracks: the rows, on the device, to hand to chroma_tracks_gather and chroma_tracks_destroy (NULL when the call fails);
 * *nrows: how many there are.  Returns when the photon arrays and the rows are complete. */
typedef struct chroma_tracks chroma_tracks;
int chroma_propagate_tracks(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons,
                            uint64_t nphotons, uint32_t ncopies, chroma_rng rng,
                            const chroma_propagate_options *options,
                            chroma_propagate_stats *stats, int32_t *aborted, chroma_tracks **tracks, uint64_t *nrows);
/* The rows per photon (CSR): d_offsets[0 .. nphotons] (device), and rows d_offsets[i] .. d_offsets[i + 1] of the arrays of `dst`
 * (device, *nrows entries each; rng_counters is not written and may be NULL) are the track of photon i -- the index in the
 * arrays of the call, copies included -- in step order.  Queued on the context's stream; may be called more than once. */
int chroma_tracks_gather(chroma_ctx *ctx, chroma_tracks *tracks, const chroma_photon_arrays *dst, uint64_t *d_offsets);
/* gives the rows back to the pool (behind the work queued on the context's stream); `tracks` may be NULL */
int chroma_tracks_destroy(chroma_ctx *ctx, chroma_tracks *tracks);

/* Per-channel reduction of detected photons: hit count and earliest hit time
 * (float bits, valid for t >= 0 as in chroma/cuda/daq.cu:5-20).  The arrays
 * (length nchannels, device) are ACCUMULATED into: zero / 0x7f800000-fill them first.
 * This is the quantity all-reduced across GPUs. */
int chroma_channel_hits(chroma_ctx *ctx, chroma_geometry *geom, uint64_t nphotons,
                        uint32_t detection_state, const chroma_photon_arrays *photons,
                        uint32_t *d_hit_count, uint32_t *d_earliest_time_bits);

/* ---- DAQ --------------------------------------------------------
 * `run_daq` (chroma/cuda/daq.cu:35-86) for photons [first_photon, first_photon + nphotons): a
 * photon with `detection_state` set whose last hit triangle belongs to a channel contributes, with
 * probability weight * global_weight, a hit time (photon time + a draw from the time CDF) and a
 * charge (a draw from the charge CDF, quantised to charge_unit) to its channel: atomicMin on the
 * time bits, atomicAdd on the integer charge, atomicOr on the history.  The three draws come from
 * the photon's Philox stream number 1 + acquisition (include/chroma_math.h), not from per-thread
 * curandStates.  The CDF tables are DEVICE arrays of cdf_len floats each (chroma/cuda/detector.h).
 * The channel arrays are accumulated into: reset them first (chroma_daq_reset). */
typedef struct chroma_daq_tables {
    const float *d_time_cdf_x, *d_time_cdf_y;      int32_t time_cdf_len;
    const float *d_charge_cdf_x, *d_charge_cdf_y;  int32_t charge_cdf_len;
    float charge_unit;
} chroma_daq_tables;
/* `reset_earliest_time_int` (daq.cu:25-33) + zeroing of charge and history */
int chroma_daq_reset(chroma_ctx *ctx, float maxtime, uint32_t nchannels, uint32_t *d_earliest_time_int,
                     uint32_t *d_channel_q_int, uint32_t *d_channel_histories);
int chroma_daq_acquire(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                       int32_t first_photon, int32_t nphotons, uint32_t detection_state,
                       const chroma_photon_arrays *photons, chroma_rng rng, uint32_t acquisition,
                       float global_weight, uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                       uint32_t *d_channel_histories);
/* `run_daq_many` (chroma/cuda/daq.cu:88-150; GPUDaq(ndaq > 1), chroma/gpu/daq.py:85-99): `ndaq`
 * independent acquisitions of the same photons side by side -- copy i accumulates into channels
 * [i * channel_stride, (i + 1) * channel_stride) of arrays of ndaq * channel_stride entries -- each
 * adding a unit normal jitter to the hit time (the reference's curand_normal; here Box-Muller on the
 * photon's stream, include/chroma_math.h).  Copy i of a photon draws from words 8 i ... of Philox
 * stream 1 + acquisition of that photon. */
int chroma_daq_acquire_many(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                            int32_t first_photon, int32_t nphotons, uint32_t detection_state,
                            const chroma_photon_arrays *photons, chroma_rng rng, uint32_t acquisition,
                            float global_weight, int32_t ndaq, int32_t channel_stride,
                            uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int, uint32_t *d_channel_histories);
/* The per-event acquisitions of a batch as ONE launch: `nrows` events given as nrows + 1 ascending photon
 * bounds (a HOST array; row r is the photons [bounds[r], bounds[r + 1]), empty rows allowed, bounds[0]
 * need not be 0 nor bounds[nrows] the end of the set of `nphotons` photons).  A photon of row r does what
 * chroma_daq_acquire does for it in the acquisition numbered `acquisition + r` -- the same rejects, the
 * same three draws from Philox stream 1 + acquisition + r, no jitter -- into word r * channel_stride +
 * channel of the three arrays (nrows * channel_stride words each, accumulated into: reset them first).
 * Word for word what nrows chroma_daq_acquire calls onto nrows separate states leave.  Bounds that
 * descend or end beyond `nphotons`, nrows < 1 and channel_stride < nchannels are CHROMA_ERR_INVALID before
 * anything is launched. */
int chroma_daq_acquire_events(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                              uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                              const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                              uint32_t acquisition, float global_weight, uint32_t channel_stride,
                              uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                              uint32_t *d_channel_histories);
/* The touched words of such a state -- history != 0: an accepted photon always carries the detection
 * flag, so these are exactly the (row, channel) pairs any accepted photon reached, those whose time is
 * still the reset value included -- in (row, channel) order: row r is the entries [d_offsets[r],
 * d_offsets[r + 1]) (d_offsets: nrows + 1 words) of d_channel, d_t (the time bits as they are), d_q
 * (charge count * charge_unit, as chroma_daq_convert) and d_flags, arrays of `capacity` entries.  The
 * order comes from a scan, not from an atomic: the output is deterministic.  *ntouched: the number of
 * touched words (never more than the photons acquired, nor than nrows * nchannels); beyond `capacity`
 * nothing is written and the call is CHROMA_ERR_INVALID.  Returns when the arrays are written. */
int chroma_daq_compact_events(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, uint32_t channel_stride,
                              float charge_unit, const uint32_t *d_earliest_time_int,
                              const uint32_t *d_channel_q_int, const uint32_t *d_channel_histories,
                              uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel, float *d_t,
                              float *d_q, uint32_t *d_flags, uint64_t *ntouched);
/* ---- the time-binned DAQ: per-channel pulse histograms, kept sparse ---------------------------
 * A second view of the very photoelectrons chroma_daq_acquire_events accumulates: per (row, channel,
 * time bin) instead of per (row, channel), and only the bins that hold something.
 *
 * A photon of row r is treated exactly as chroma_daq_acquire_events treats it: the same rejects (no
 * triangle, no channel, detection flag not set), the same three draws in the same order from Philox
 * stream 1 + acquisition + r of photon photon_id_base + photon index -- the weight gate, the time smear
 * through the time CDF, the charge through the charge CDF -- time = photon time + smear and charge_int =
 * cm_f2u32(cm_roundf(charge / charge_unit)): toward zero after rounding; NaN and negatives give 0;
 * saturating; as cvt.rzi.u32.f32 / v_cvt_u32_f32 (a charge CDF may start below zero).  A pulse
 * acquisition with the `acquisition` of a chroma_daq_acquire_events call therefore describes the same
 * accepted photons.
 *
 * The window: dt > 0 and finite, t0 finite, 1 <= nbins <= 65536.  In float32, with IEEE subtract and
 * divide: x = (time - t0) / dt; the photon is in the window iff x >= 0.0f && x < (float)nbins, and its bin
 * is (uint32)cm_floorf(x).  An accepted photon outside the window is EARLY if time < t0 and LATE otherwise
 * (a NaN time is late).  Times are compared as floats, so negative times bin like any other (the unsigned
 * minimum of chroma_daq_acquire, which ranks them above the reset value, has no part here).
 *
 * A pulse is a (row, channel, bin) with at least one accepted in-window photon: npe, the number of them;
 * q_int, the sum of their charge_int (wrapping, as the accumulator of chroma_daq_acquire does); t_first,
 * the smallest of their times as floats (-0 ranks below +0); flags, the OR of their histories.  Pulses
 * come in ascending (row, channel, bin) order, row r the entries [d_offsets[r], d_offsets[r + 1]).  The
 * order comes from a sort and a scan and every reduction is of integers: the output is deterministic. */
typedef struct chroma_daq_window {
    float t0;           /* the lower edge of bin 0 */
    float dt;           /* the width of a bin */
    uint32_t nbins;
} chroma_daq_window;
/* *naccepted: the accepted in-window photons of the rows -- an upper bound on the number of pulses, by
 * which a caller sizes the arrays of chroma_daq_acquire_pulses.  Writes nothing else.  Arguments and
 * refusals as chroma_daq_acquire_events (there is no channel stride) and the window rules above; also
 * refused: nrows * nchannels * nbins of 2^63 or more.  All CHROMA_ERR_INVALID before anything is
 * launched. */
int chroma_daq_count_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                            uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                            const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                            uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                            uint64_t *naccepted);
/* The pulses: d_offsets (nrows + 1 words), and `capacity` entries each of d_channel, d_bin, d_npe,
 * d_q_int, d_t_first and d_flags (these six may be NULL when capacity is 0); d_outside, 2 * nrows words:
 * the early and the late photons of row r in words 2 r and 2 r + 1 -- written, not accumulated.
 * *npulses: the number of pulses; beyond `capacity` NOTHING is written (d_offsets and d_outside
 * neither), *npulses still holds the number needed and the call is CHROMA_ERR_INVALID.  An empty photon
 * window is CHROMA_OK with no pulse and d_offsets and d_outside all zero.  Returns when the arrays are
 * written.  Scratch is the context's pooled per-call block, grown to what the accepted photons need
 * (some 50 bytes each), never to photons of the window or to rows x channels x bins. */
int chroma_daq_acquire_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                              uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                              const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                              uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                              uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel, uint32_t *d_bin,
                              uint32_t *d_npe, uint32_t *d_q_int, float *d_t_first, uint32_t *d_flags,
                              uint32_t *d_outside, uint64_t *npulses);
/* ---- dark noise of the time-binned DAQ ------------------------------------------------------------
 * PMT dark counts as further photoelectrons of a pulse acquisition, drawn on the device.  Noise is
 * drawn per (row r, channel c) WORD of the acquisition, from the Philox stream 1 + acquisition + r (the
 * stream row r's photons use) of the pseudo-photon 0xffffffff00000000 | c.  Word w of a stream is word
 * w & 3 of block w >> 2, as cm_rng (include/chroma_math.h) has it.
 *
 *   The count:  k = #{ j < ncount : word 0 >= count_cdf[j] }.  count_cdf is non-decreasing; the caller
 *     puts a scaled Poisson CDF there (entry j: P(X <= j) * 2^32), the device only compares integers.
 *   Candidate j = 0 .. k - 1 has the words a = 1 + 3 j, b = 2 + 3 j, c = 3 + 3 j and is
 *     KEPT iff (word a >> 1) < d_accept[channel]: the thinning of a channel's rate against the largest one; 2^31
 *       keeps every candidate, 0 none.  A channel whose accept word is 0 is skipped without a draw (it
 *       needs no Philox block; the result is the same).
 *     Its bin: with P = (uint64)b * nbins, bin = (uint32)(P >> 32) -- always inside the window -- and
 *       f = (float)((uint32)P >> 8) * 2^-24 (exact); time = t0 + ((float)bin + f) * dt in float32, each
 *       operation rounded once.  THE BIN IS THE DRAWN ONE, whatever rounding makes of `time` (a time
 *       that rounds up to the next bin's edge stays in its bin; (time - t0) / dt is not consulted).
 *     Its charge, as a photon's: charge = interp_table(cm_u32_to_uniform(c), the charge CDF) and
 *       charge_int = cm_f2u32(cm_roundf(charge / charge_unit)): toward zero after rounding; NaN and
 *       negatives give 0; saturating; as cvt.rzi.u32.f32 / v_cvt_u32_f32.
 *     Its history: `flag`.
 * A kept noise photoelectron enters the pulses exactly like an accepted in-window photon of row r: it
 * counts in npe, adds to the wrapping q_int, competes for t_first and ORs `flag` into flags.  A pulse
 * may mix light and noise.  Rows without photons, and a call whose photon span is empty, still get
 * their noise; early and late (d_outside) count photons only.  Everything is counter-based: the result
 * does not depend on the launch shape or on how a batch is cut into calls (row r of a call with
 * `acquisition` a is row 0 of a call with a + r). */
typedef struct chroma_daq_noise {
    const uint32_t *count_cdf;   /* HOST array of `ncount` words, non-decreasing */
    uint32_t ncount;             /* 1 .. 64: the most candidates a word can have */
    const uint32_t *d_accept;    /* DEVICE array, nchannels words, each 0 .. 2^31 */
    uint32_t flag;               /* exactly one history bit */
} chroma_daq_noise;
/* chroma_daq_count_pulses / chroma_daq_acquire_pulses with noise; `noise` NULL gives the bits of those
 * calls.  *naccepted is the accepted in-window photons PLUS the kept noise photoelectrons; the capacity
 * rules are unchanged.  d_row_noise (nrows words, or NULL): the kept noise photoelectrons of each row,
 * written, not accumulated -- the truth counterpart of d_outside.  Beyond `capacity` nothing of the
 * caller's is written, d_row_noise included, and *npulses holds what is needed.
 * Refused before anything is launched, besides what those calls refuse: with noise, ncount outside
 * 1 .. 64, a descending count_cdf, a flag that is not exactly one bit, a NULL array, nrows * nchannels of
 * 2^32 or more, and photon ids (rng.photon_id_base + [0, nphotons)) that reach the high word 0xffffffff
 * of the pseudo-photons. */
int chroma_daq_count_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                                  uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                                  const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                                  uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                  const chroma_daq_noise *noise, uint64_t *naccepted);
int chroma_daq_acquire_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables,
                                    uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                                    const chroma_photon_arrays *photons, uint32_t nphotons, chroma_rng rng,
                                    uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                    const chroma_daq_noise *noise, uint64_t capacity, uint32_t *d_offsets,
                                    int32_t *d_channel, uint32_t *d_bin, uint32_t *d_npe, uint32_t *d_q_int,
                                    float *d_t_first, uint32_t *d_flags, uint32_t *d_outside,
                                    uint32_t *d_row_noise, uint64_t *npulses);
/* The same draws on the host (no GPU, no context): the kept noise photoelectrons of `nrows` rows in
 * (row, channel, candidate) order -- row, channel, bin, time bits, charge count, `capacity` entries each
 * (may be NULL when capacity is 0).  Here the charge CDF of `tables` (the time CDF is not read) and
 * noise->d_accept are HOST arrays.  *n: their number; beyond `capacity` the first `capacity` are written
 * and the call is CHROMA_ERR_INVALID.  Refuses what the calls above refuse of the noise and the window. */
int chroma_daq_noise_host(const chroma_daq_tables *tables, const chroma_daq_window *window,
                          const chroma_daq_noise *noise, uint32_t nrows, uint32_t nchannels, uint64_t seed,
                          uint32_t acquisition, uint64_t capacity, uint32_t *row, uint32_t *channel,
                          uint32_t *bin, uint32_t *time_bits, uint32_t *charge_int, uint64_t *n);
/* ---- the trigger of the time-binned DAQ: firings and their readout gates ------------------------
 * A second, purely integer stage on the pulses of chroma_daq_acquire_pulses (no random draws): a
 * multiplicity or photoelectron sum over a sliding coincidence window, a level trigger with lockout on
 * it, and per firing the pulses of its readout gate, reduced per channel.
 *
 * The sum.  For row r and bin b, with W = width:
 *   CHROMA_TRIGGER_NHIT  S(r, b) = the number of DISTINCT channels of row r that have a pulse in a bin p
 *                        with b - W < p <= b;
 *   CHROMA_TRIGGER_NPE   S(r, b) = the sum of npe over row r's pulses with b - W < p <= b (exact below
 *                        2^32; it wraps beyond).
 * The firing rule.  Per row, next = 0; through b = 0 .. nbins - 1 ascending the trigger fires at b iff
 * S(r, b) >= threshold and b >= next, and then next = b + holdoff.  A level trigger with lockout: it
 * fires again after the lockout while the sum is still at or above threshold.  The gate of a firing at
 * bin b is the bins [b - pre, b + post), clipped to [0, nbins); holdoff >= pre + post, so the gates of
 * one row never overlap and a pulse lies in one gate at the most. */
#define CHROMA_TRIGGER_NHIT 0
#define CHROMA_TRIGGER_NPE 1
typedef struct chroma_daq_trigger {   /* 24 bytes, all in BINS of the window */
    uint32_t kind;        /* CHROMA_TRIGGER_NHIT = 0: channels; CHROMA_TRIGGER_NPE = 1: photoelectrons */
    uint32_t threshold;   /* >= 1 */
    uint32_t width;       /* W, the coincidence window: 1 .. nbins */
    uint32_t holdoff;     /* H, bins from one firing to the next possible one: >= max(1, pre + post) */
    uint32_t pre, post;   /* the gate of a firing at bin b: bins [b - pre, b + post), clipped to [0, nbins); post >= 1 */
} chroma_daq_trigger;
/* Input: the pulses of `nrows` rows as chroma_daq_acquire_pulses writes them -- d_offsets (nrows + 1
 * words) and, per pulse, d_channel, d_bin, d_npe, d_q_int, d_t_first and d_flags (npulses entries, in
 * ascending (row, channel, bin) order) -- the window they were binned with and the number of channels.
 *
 * Output, its order from scans and a sort, never from the arrival order of atomics:
 *   triggers, in (row, bin) order: row r the entries [d_trig_offsets[r], d_trig_offsets[r + 1])
 *     (nrows + 1 words) of d_trig_bin and d_trig_sum (S at the firing bin), `trigger_capacity` entries
 *     each; d_hit_offsets, trigger_capacity + 1 words of which *ntriggers + 1 are written;
 *   gated hits, in (trigger, channel) order: trigger k the entries [d_hit_offsets[k],
 *     d_hit_offsets[k + 1]) of d_hit_channel, d_hit_npe, d_hit_q_int, d_hit_t_first and d_hit_flags
 *     (`hit_capacity` entries each) -- one entry per (trigger, channel) with at least one pulse of the
 *     trigger's row in its gate: the sum of their npe, the wrapping sum of their q_int, the smallest of
 *     their t_first as floats (-0 below +0) and the OR of their flags.  A trigger may have no hit (a
 *     gate shorter than the coincidence window);
 *   d_pulse_trigger (npulses words, or NULL): per pulse the index of the trigger whose gate holds it,
 *     or 0xffffffff.
 *
 * Capacities.  nrows * ceil(nbins / holdoff) triggers always suffice, and so do npulses *
 * ceil(width / holdoff) (a pulse holds the sum up for `width` bins); npulses hits always suffice.  If
 * either capacity is too small NOTHING is written, *ntriggers and *nhits hold what is needed and the
 * call is CHROMA_ERR_INVALID.
 *
 * Refused, CHROMA_ERR_INVALID before anything is launched: a window the pulse calls refuse; nrows or
 * nchannels of 0; threshold == 0; width outside 1 .. nbins; post == 0; holdoff < max(1, pre + post); an
 * unknown kind; npulses of 2^31 - 1 or more (so of 2^32 or more), nrows * nbins of 2^31 or more; a NULL
 * array that is needed (the pulse arrays when npulses, the trigger arrays when trigger_capacity, the hit
 * arrays when hit_capacity; d_offsets, d_trig_offsets, d_hit_offsets, ntriggers and nhits always).
 *
 * npulses == 0 is CHROMA_OK with all offsets zero.  A pulse whose bin is >= nbins, whose channel is
 * outside [0, nchannels) or which the offsets put in no row contributes nothing, indexes nothing and
 * has 0xffffffff in d_pulse_trigger.  Input that is not in (row, channel, bin) order gives unspecified
 * values, but no access outside the caller's arrays and the call's scratch.
 *
 * Runs on the context's stream and returns when the arrays are written.  Scratch is the context's
 * pooled per-call block: 4 bytes per (row, bin) for the sum, some 50 bytes per pulse, 8 bytes per
 * trigger of the bound above. */
int chroma_daq_trigger_pulses(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                              const chroma_daq_trigger *trigger, const uint32_t *d_offsets, const int32_t *d_channel,
                              const uint32_t *d_bin, const uint32_t *d_npe, const uint32_t *d_q_int,
                              const float *d_t_first, const uint32_t *d_flags, uint64_t npulses,
                              uint64_t trigger_capacity, uint32_t *d_trig_offsets, uint32_t *d_trig_bin,
                              uint32_t *d_trig_sum, uint32_t *d_hit_offsets, uint64_t hit_capacity,
                              int32_t *d_hit_channel, uint32_t *d_hit_npe, uint32_t *d_hit_q_int,
                              float *d_hit_t_first, uint32_t *d_hit_flags, uint32_t *d_pulse_trigger,
                              uint64_t *ntriggers, uint64_t *nhits);
/* ---- the digitiser of the time-binned DAQ: a shaped ADC trace per gated hit -------------------------
 * A third integer stage, on the outputs of chroma_daq_acquire_pulses and chroma_daq_trigger_pulses where
 * they lie: every photoelectron charge count becomes a pulse of `ntaps` bins, pulses pile up, the tail of
 * light from before the gate is on the line, the electronics add a pedestal and noise, and the converter
 * clips.  The reference has no counterpart; this is the definition.
 *
 * A TRACE belongs to a gated hit.  Hit i is (trigger k, channel c) as chroma_daq_trigger_pulses wrote it
 * (d_hit_offsets[k] <= i < d_hit_offsets[k + 1], c = d_hit_channel[i]); trigger k fires at bin b =
 * d_trig_bin[k] of row r (d_trig_offsets[r] <= k < d_trig_offsets[r + 1]).  One trace per hit is
 * zero-suppressed readout: a channel is read iff it has a pulse in the gate.  Every trace has G = pre +
 * post samples (of the trigger, NOT clipped to the window); sample s stands for the signed bin number
 * B(s) = b - pre + s, which may lie before bin 0 or at or beyond nbins: no pulses there, but the ADC keeps
 * sampling.
 *
 * The signal.  Over ALL pulses p of (row r, channel c) with 0 <= B(s) - bin[p] < ntaps -- not the gate's
 * alone: pulses before the gate and in an earlier firing's gate have their tails on the line --
 *   acc(s) = sum of (uint64)(int64)((int64)q_int[p] * taps[B(s) - bin[p]]),
 * summed as 64-bit unsigned, wrapping, and then read as signed.  The sample is
 *   v(s) = clip(pedestal + (acc(s) >> shift, arithmetic) + e(s), 0, 2^bits - 1)
 * in int64, stored as uint16 (the sum of the three terms is the exact one: it is not left to wrap).
 *
 * The electronics noise.  e(s) = 0 when nnoise == 0; otherwise e(s) = noise_lo + #{ j < nnoise : w >=
 * noise_cdf[j] } with w one Philox word of (acquisition + row, channel, ABSOLUTE bin), whichever firing
 * reads it and however the hits are sliced: with u = (uint32)(B(s) + 65536) (>= 0: pre <= G <= 65536), w
 * is word u & 3 of cm_philox4x32_10(0x80000000 | (u >> 2), 1 + acquisition + r, c, 0xffffffff, seed lo,
 * seed hi) -- the dark noise's pseudo-photon of channel c in the stream of row r, in blocks whose top
 * bit is set, so that they never meet the dark noise's blocks 0 .. 48.  As with the dark noise, photon
 * ids must not reach the high word 0xffffffff; this call sees no photons and cannot check it
 * (GPUEventDaq does, before any call).  The caller puts a scaled CDF into noise_cdf (for a Gaussian of
 * sigma ADC counts: noise_lo = -32, entry j = floor(Phi((noise_lo + j + 0.5) / sigma) * 2^32), saturated);
 * the device only compares integers.
 *
 * d_trace_flags, a word per trace: bit 0 some sample was clipped at the top, bit 1 some at 0. */
typedef struct chroma_daq_digitizer {
    const int32_t *taps;       /* HOST array: the response to one charge count, tap d = d bins after the pulse's bin, fixed point */
    uint32_t ntaps;            /* 1 .. 1024 */
    uint32_t shift;            /* 0 .. 31: the fixed point's fractional bits */
    int32_t  pedestal;         /* ADC counts */
    uint32_t bits;             /* 1 .. 16: samples are clipped to [0, 2^bits - 1] */
    const uint32_t *noise_cdf; /* HOST array, non-decreasing, or NULL */
    uint32_t nnoise;           /* 0 (no electronics noise) .. 64 */
    int32_t  noise_lo;         /* the noise value when the drawn word is below every entry */
} chroma_daq_digitizer;
/* Writes d_adc[(i - first_hit) * G + s] and d_trace_flags[i - first_hit] for the hits i of [first_hit,
 * first_hit + nhits_call): the slice lets a caller bound the memory of one call, and a slice is that part
 * of the whole.  d_adc has `sample_capacity` entries.  Inputs: the pulses (d_offsets, nrows + 1 words;
 * d_channel, d_bin, d_q_int, npulses entries in (row, channel, bin) order), the triggers (d_trig_offsets,
 * nrows + 1 words; d_trig_bin, ntriggers entries) and the hits (d_hit_offsets, ntriggers + 1 words;
 * d_hit_channel, nhits entries) of the calls above, with the window, the trigger and the number of
 * channels they were made with, the context's seed and the acquisition number of row 0 (row r of a call
 * is row 0 of a call with acquisition + r).
 *
 * Refused, CHROMA_ERR_INVALID before anything is launched and with nothing written: what
 * chroma_daq_trigger_pulses refuses of window, trigger, nrows and nchannels; G > 65536; ntaps outside
 * 1 .. 1024, shift > 31, bits outside 1 .. 16, nnoise > 64; a descending noise_cdf; npulses, ntriggers or
 * nhits of 2^32 or more; a NULL array that is needed (taps; noise_cdf when nnoise; the pulse arrays when
 * npulses, d_trig_bin when ntriggers, d_hit_channel when nhits, d_adc and d_trace_flags when nhits_call;
 * the three offset arrays always); a slice that ends beyond nhits; sample_capacity < nhits_call * G.
 * nhits_call == 0 is CHROMA_OK and launches nothing.
 *
 * Every search runs over a fixed index range, whatever the arrays hold.  A hit whose channel is outside
 * [0, nchannels), or whose trigger the offsets put in no row, has no signal: its trace is pedestal plus
 * noise (of row 0 where there is no row, and with b = 0 where the hit offsets put the hit in no trigger;
 * the channel word of the noise is the hit's channel as it stands).  Input that is not sorted gives
 * unspecified values, but no access outside the caller's arrays.
 *
 * Runs on the context's stream and returns when the arrays are written.  Scratch: the taps. */
int chroma_daq_digitize_gates(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                              const chroma_daq_trigger *trigger, const chroma_daq_digitizer *digitizer, uint64_t seed,
                              uint32_t acquisition, const uint32_t *d_offsets, const int32_t *d_channel,
                              const uint32_t *d_bin, const uint32_t *d_q_int, uint64_t npulses,
                              const uint32_t *d_trig_offsets, const uint32_t *d_trig_bin, uint64_t ntriggers,
                              const uint32_t *d_hit_offsets, const int32_t *d_hit_channel, uint64_t nhits,
                              uint64_t first_hit, uint64_t nhits_call, uint64_t sample_capacity, uint16_t *d_adc,
                              uint32_t *d_trace_flags);
/* The same on the host (no GPU, no context), a plain loop over trace, sample and pulse: the same arguments
 * on HOST arrays, the same refusals, the same bits. */
int chroma_daq_digitize_host(uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                             const chroma_daq_trigger *trigger, const chroma_daq_digitizer *digitizer, uint64_t seed,
                             uint32_t acquisition, const uint32_t *offsets, const int32_t *channel, const uint32_t *bin,
                             const uint32_t *q_int, uint64_t npulses, const uint32_t *trig_offsets,
                             const uint32_t *trig_bin, uint64_t ntriggers, const uint32_t *hit_offsets,
                             const int32_t *hit_channel, uint64_t nhits, uint64_t first_hit, uint64_t nhits_call,
                             uint64_t sample_capacity, uint16_t *adc, uint32_t *trace_flags);
/* ---- the trace reduction of the time-binned DAQ: found pulses, their charge and their time ----------
 * A fourth integer stage, on the samples chroma_daq_digitize_gates left on the device: what the
 * electronics make of a trace -- the pulses in it, the charge of each and a constant-fraction time.  A
 * function of the traces alone (d_adc: ntraces traces of G samples each) and of the parameters below.
 * The reference has no counterpart; this is the definition.  All sums are of integers: their order does
 * not show, and the host twin gives the same bits.
 *
 * Per trace, with samples v(s), s in [0, G): N = max(nbaseline, 1); base = the sum of v(s) over s <
 * nbaseline when nbaseline > 0, else pedestal; y(s) = polarity * (N * v(s) - base) as int32 (|y| < 2^22);
 * T = N * threshold.
 *
 * Runs and pulses.  A RUN [a, e) is a maximal stretch of consecutive samples with y(s) >= T, over the
 * whole trace, the baseline samples included.  A PULSE is a run with e - a >= min_width; the pulses of a
 * trace are numbered j = 0 .. n - 1 by ascending a.  The samples of a rejected run are ordinary samples.
 *
 * The integration window [begin_j, stop_j) of pulse j, non-overlapping by construction:
 *   stop_j  = min(e_j + lag, a_{j+1} if there is a pulse j + 1, G),
 *   begin_j = max(a_j - lead clamped at 0, stop_{j-1} if j > 0).
 *
 * Per found pulse: start = a_j; width = e_j - a_j; peak = the largest y of the run; peak_sample = the
 * FIRST sample of the run that attains it; integral (int64: 65536 samples of 2^22) = the sum of y(s) over
 * the window; time, in 1/256 of a sample; flags: bit 0 TIME_AT_EDGE, bit 1 OPEN_AT_START (a_j == 0), bit
 * 2 OPEN_AT_END (e_j == G).
 *
 * The time.  L = max(1, (peak * cfd) >> 8); s_c = the smallest s of [begin_j, peak_sample] with y(u) >= L
 * for every u of [s, peak_sample].  If s_c == begin_j and (begin_j == 0 or y(begin_j - 1) >= L): time =
 * 256 * s_c and TIME_AT_EDGE is set.  Otherwise, with y0 = y(s_c - 1) < L <= y1 = y(s_c),
 *   time = 256 * (s_c - 1) + ((L - y0) * 256) / (y1 - y0),
 * an unsigned 32-bit floor division of operands below 2^31; the fraction lies in (0, 256].
 *
 * Per trace: d_found_offsets (ntraces + 1 words, the first 0), the trace's place in the pulse arrays;
 * d_trace_base (int32) = base; d_reduced_flags: bit 0 BASELINE_BUSY iff nbaseline > 0 and the largest
 * minus the smallest baseline sample exceeds baseline_spread. */
typedef struct chroma_daq_reducer {   /* 36 bytes */
    int32_t  polarity;         /* +1: pulses rise; -1: they fall */
    uint32_t nbaseline;        /* 0 .. 64 and <= G: the leading samples the baseline is measured over; 0: `pedestal` */
    uint32_t pedestal;         /* 0 .. 65535, used iff nbaseline == 0 */
    uint32_t baseline_spread;  /* the largest allowed max - min over the baseline samples */
    uint32_t threshold;        /* 1 .. 65535 ADC counts above baseline */
    uint32_t min_width;        /* 1 .. 65536: the shortest run of samples that counts as a pulse */
    uint32_t lead, lag;        /* 0 .. 65535 each: samples integrated before and behind a pulse */
    uint32_t cfd;              /* 1 .. 256: the constant fraction, in 1/256 */
} chroma_daq_reducer;
#define CHROMA_FOUND_TIME_AT_EDGE 1u
#define CHROMA_FOUND_OPEN_AT_START 2u
#define CHROMA_FOUND_OPEN_AT_END 4u
#define CHROMA_REDUCED_BASELINE_BUSY 1u
/* Count, scan, fill: a pass counts the pulses per trace, an exclusive sum makes d_found_offsets, a pass
 * fills the pulse arrays (`found_capacity` entries each).  *nfound, the offsets, d_trace_base and
 * d_reduced_flags are always written.  If *nfound > found_capacity the pulse arrays stay untouched and the
 * call is CHROMA_ERR_INVALID, as chroma_daq_trigger_pulses' is with too few trigger entries: grow them
 * and call again.
 *
 * Refused, CHROMA_ERR_INVALID before anything is launched and with nothing written: a parameter outside
 * the ranges above; G outside 1 .. 65536; ntraces * G of 2^32 or more, or ntraces of 2^31 - 1 or more
 * (the scan's count); a NULL array that is needed (d_adc and the three per-trace arrays when ntraces; the
 * pulse arrays when ntraces and found_capacity; reducer and nfound always).  ntraces == 0 is CHROMA_OK: it launches
 * nothing, writes nothing but *nfound = 0.  Every uint16 is a valid sample: no input makes an access
 * outside the arrays.
 *
 * Runs on the context's stream and returns when the arrays are written.  Scratch: the scan's workspace. */
int chroma_daq_reduce_traces(chroma_ctx *ctx, const chroma_daq_reducer *reducer, uint32_t G, uint64_t ntraces,
                             const uint16_t *d_adc, uint64_t found_capacity, uint32_t *d_found_offsets,
                             int32_t *d_trace_base, uint32_t *d_reduced_flags, uint32_t *d_found_start,
                             uint32_t *d_found_width, uint32_t *d_found_peak, uint32_t *d_found_peak_sample,
                             int64_t *d_found_integral, uint32_t *d_found_time, uint32_t *d_found_flags,
                             uint64_t *nfound);
/* The same on the host (no GPU, no context), plain loops over trace, sample and pulse: the same
 * arguments on HOST arrays, the same refusals, the same bits. */
int chroma_daq_reduce_host(const chroma_daq_reducer *reducer, uint32_t G, uint64_t ntraces, const uint16_t *adc,
                           uint64_t found_capacity, uint32_t *found_offsets, int32_t *trace_base,
                           uint32_t *reduced_flags, uint32_t *found_start, uint32_t *found_width,
                           uint32_t *found_peak, uint32_t *found_peak_sample, int64_t *found_integral,
                           uint32_t *found_time, uint32_t *found_flags, uint64_t *nfound);
/* `convert_sortable_int_to_float` + `convert_charge_int_to_float` (daq.cu:152-173) */
int chroma_daq_convert(chroma_ctx *ctx, uint32_t nchannels, float charge_unit, const uint32_t *d_earliest_time_int,
                       const uint32_t *d_channel_q_int, float *d_earliest_time, float *d_channel_q);

/* ---- vertex seed: a time-residual fit over a lattice of positions --------------------------------------
 * What turns the (channel, time, charge) rows of a firing into a position and a time to start a
 * likelihood from: for a hypothesised position the hits' times less their straight-line times of flight
 * pile up in one bin of a histogram when the position is right; the score of a position is the fullest
 * stretch of that histogram under a short shape, and the search takes the best of a list of candidates and
 * refines it on shrinking 5 x 5 x 5 lattices.  The reference has no counterpart; this is the definition.
 * All quantities are integers -- positions in position units, times in ticks; what a unit and a tick are
 * is the caller's business -- and all sums are of integers: their order does not show, and the host twin
 * gives the same bits.
 *
 * Fit f holds the hits [offsets[f], offsets[f + 1]).  For fit f and a position x, hit i of the fit is
 * placed so: a hit whose channel is not in [0, nchannels) is OUTSIDE.  Otherwise w_i = min(hit_weight,
 * 255); D2 = the sum of the three squared coordinate differences between the channel's position and x
 * (below 2^53); d_i = floor(sqrt(D2)); tof_i = (d_i * slowness + 32768) >> 16 in 64 bits; tau_i =
 * hit_time - tof_i as int64.  If tau_i < tau0[f] the hit is OUTSIDE; otherwise b_i = (tau_i - tau0[f]) /
 * bin_ticks, and b_i >= nbins is OUTSIDE.  H[b] is the sum of w_i over the hits with b_i = b, and H[b] = 0
 * for b >= nbins.
 *
 * A[s] = the sum over j < K of shape[j] * H[s + j], s in [0, nbins); score(f, x) = the largest A[s] (it fits
 * 32 bits: 255 * 65535 * 255 < 2^32) and bin(f, x) = the smallest s that attains it.  A fit without hits
 * inside has score 0 and bin 0.
 *
 * Level 0: the candidate with the greatest score, the lowest index among equals: best_cand, and
 * level_score[0] its score.  Levels l = 1 .. L: s_l = step >> (l - 1); the 125 points x = best + ((i - 2),
 * (j - 2), (k - 2)) * s_l, i, j, k in 0 .. 4, m = i + 5 j + 25 k; the greatest score wins, a tie goes to the
 * centre (m = 62) if it is among the tied points, else to the lowest m; level_score[l] is the winner's
 * score.  The centre takes part, so level_score never decreases.  After level L: best_pos, best_score and
 * best_bin are those of the final point and `outside` is the number of its OUTSIDE hits. */
typedef struct chroma_vertex_seeder {   /* 88 bytes */
    uint32_t slowness;    /* 1 .. 2^24: ticks per position unit, in 1/65536 */
    uint32_t bin_ticks;   /* 1 .. 2^20 */
    uint32_t nbins;       /* 1 .. 1024 */
    uint32_t nshape;      /* K, 1 .. 16 */
    uint32_t step;        /* 0 .. 2^21: lattice spacing of refinement level 1, position units */
    uint32_t nlevels;     /* L, 0 .. 8 */
    uint32_t shape[16];   /* each 0 .. 255; the largest of shape[0 .. K) is >= 1; entries from K on are ignored */
} chroma_vertex_seeder;
/* d_channel_pos (int32, 3 per channel), d_cand (int32, 3 per candidate: the level-0 candidates, shared by
 * all fits), the hit arrays (d_hit_channel int32, d_hit_time int32 ticks, d_hit_weight uint32) and the
 * outputs are DEVICE arrays; `offsets` (nfits + 1 words) and `tau0` (nfits) are HOST arrays.  Per fit:
 * d_best_pos (int32, 3), d_best_score, d_best_bin, d_best_cand, d_outside (uint32) and d_level_score
 * (uint32, L + 1 per fit).  d_scores (uint32, nfits * ncand: score(f, cand[c]) at f * ncand + c) may be
 * NULL.
 *
 * The function is total: no content of the hit, channel or candidate arrays makes an access outside the
 * arrays.  Refused, CHROMA_ERR_INVALID before a fit is launched and with nothing written: a seeder field
 * outside its range; ncand of 0 or above 2^20; nchannels above (2^32 - 1) / 3 or nfits above 2^31 - 1
 * (32-bit indices); a coordinate of d_channel_pos or d_cand beyond 2^23 in
 * magnitude (the two device arrays are checked by a validation pass of their own, whose verdict is read
 * back before the first fit is launched); offsets not starting at 0, descending, or with a fit of more
 * than 65535 hits; nfits * ncand of 2^32 or more when d_scores is asked for; a NULL array that is needed
 * (seeder always; the candidates, offsets, tau0 and the per-fit outputs when nfits; the channel positions
 * when nchannels and nfits; the hit arrays when there are hits).  nfits == 0 is CHROMA_OK and writes
 * nothing.
 *
 * Runs on the context's stream and returns when the outputs are written.  Scratch: the offsets, tau0, the
 * level-0 maxima (a 64-bit word per fit) and the validation's verdict. */
int chroma_vertex_seed(chroma_ctx *ctx, const chroma_vertex_seeder *seeder, uint32_t nchannels,
                       const int32_t *d_channel_pos, uint32_t ncand, const int32_t *d_cand, uint32_t nfits,
                       const uint32_t *offsets, const int32_t *tau0, const int32_t *d_hit_channel,
                       const int32_t *d_hit_time, const uint32_t *d_hit_weight, int32_t *d_best_pos,
                       uint32_t *d_best_score, uint32_t *d_best_bin, uint32_t *d_best_cand, uint32_t *d_outside,
                       uint32_t *d_level_score, uint32_t *d_scores);
/* The same on the host (no GPU, no context), plain loops over fit, position and hit on one thread: the same
 * arguments on HOST arrays, the same refusals, the same bits. */
int chroma_vertex_seed_host(const chroma_vertex_seeder *seeder, uint32_t nchannels, const int32_t *channel_pos,
                            uint32_t ncand, const int32_t *cand, uint32_t nfits, const uint32_t *offsets,
                            const int32_t *tau0, const int32_t *hit_channel, const int32_t *hit_time,
                            const uint32_t *hit_weight, int32_t *best_pos, uint32_t *best_score,
                            uint32_t *best_bin, uint32_t *best_cand, uint32_t *outside, uint32_t *level_score,
                            uint32_t *scores);

/* ---- direction seed: a cone fit about the vertex --------------------------------------------------------
 * What gives a seed vertex the direction it lacks: seen from the vertex, the hits of a Cherenkov ring lie
 * at one angle to the particle's direction.  The score of a hypothesised direction is the sum over the
 * hits of a profile of the cosine between the hit's direction from the vertex and the hypothesis; the
 * search takes the best of a list of candidate directions and refines it on shrinking 5 x 5 x 5 lattices,
 * every point renormalised.  The reference has no counterpart; this is the definition.  Everything that
 * shows is an integer; sums are of integers, so their order does not show, and the host twin gives the
 * same bits.  Positions are in the vertex seed's position units; a direction is an integer 3-vector, a
 * UNIT direction has length about 2^14 (Q14), a cosine is an integer in [-16384, 16383].
 *
 * Fit f holds the hits [offsets[f], offsets[f + 1]) and is seen from its vertex v_f (int32 x 3).  A hit
 * whose channel is not in [0, nchannels) is OUTSIDE.  Otherwise (dx, dy, dz) = the channel's position -
 * v_f in 64 bits and d = floor(sqrt(dx^2 + dy^2 + dz^2)) (the vertex seed's); d == 0 is OUTSIDE (no
 * direction).  Where hit times are given (d_hit_time != NULL): b = the vertex seed's bin of the hit with
 * `timing`'s slowness, bin_ticks and nbins and tau0[f] (tof = (d * slowness + 32768) >> 16; tau = time -
 * tof; tau < tau0[f] or (tau - tau0[f]) / bin_ticks >= nbins is OUTSIDE), and b < bin[f] + first or b >=
 * bin[f] + first + width, compared in 64 bits, is OUTSIDE: the prompt-light cut about the seed's own
 * best_bin.  Without times no cut is made.  Otherwise the hit is INSIDE with w = min(hit_weight, 255) and
 * n = (trunc(dx * 16384 / d), trunc(dy * 16384 / d), trunc(dz * 16384 / d)), C's truncation toward zero:
 * every component within +-16384.  inside[f] is the sum of w over the INSIDE hits (an energy proxy),
 * outside[f] the number of OUTSIDE hits.
 *
 * A point a (int32 x 3, every component within +-2^15): L = floor(sqrt(a . a)); if L == 0 its unit vector
 * is (0, 0, 0); otherwise u = (trunc(a_x * 16384 / L), ...), every component within +-16384.  A unit
 * vector u of (0, 0, 0) scores 0.  Otherwise, per INSIDE hit, c = clamp((n . u) >> 14, -16384, 16383)
 * (the shift arithmetic, the dot product in int32: 3 * 2^28 < 2^31), k = (c + 16384) >> (15 - m) for a
 * profile of 2^m entries, and score(f, u) = the sum of w * profile[k] (it fits 32 bits: 65535 * 255 * 255
 * < 2^32).
 *
 * Level 0: the candidate whose unit vector scores greatest, the lowest index among equals: best_cand;
 * best_dir is its unit vector and level_score[0] its score.  Levels l = 1 .. L: s_l = step >> (l - 1);
 * the 125 points best_dir + ((i - 2), (j - 2), (k - 2)) * s_l, m = i + 5 j + 25 k, each renormalised as
 * above -- but the centre (m = 62), which is taken as it is, so level_score never decreases; the greatest
 * score wins, a tie goes to the centre if it is among the tied points, else to the lowest m; best_dir
 * becomes the winner's unit vector and level_score[l] its score.  After level L: best_dir, best_score (=
 * level_score[L]), best_cand, level_score, inside, outside and, if asked for, cos_hist[f][k] = the sum of
 * w over the INSIDE hits whose k about best_dir is k (2^m words per fit; about a best_dir of (0, 0, 0)
 * every hit's c is 0): the ring's opening-angle distribution. */
typedef struct chroma_direction_seeder {   /* 276 bytes */
    uint32_t log2_ncos;    /* m, 4 .. 8: the profile has 2^m entries */
    uint32_t step;         /* 0 .. 2^13: lattice spacing of refinement level 1, Q14 */
    uint32_t nlevels;      /* L, 0 .. 8 */
    uint32_t first;        /* 0 .. 1040: the prompt window begins `first` bins behind bin[f] ... */
    uint32_t width;        /* 1 .. 2048: ... and has so many bins */
    uint8_t  profile[256]; /* some entry among the first 2^m is >= 1; entries from 2^m on are ignored */
} chroma_direction_seeder;
/* d_channel_pos (int32, 3 per channel), d_cand (int32, 3 per candidate: the level-0 candidates, shared by
 * all fits), d_vertex (int32, 3 per fit), d_bin (uint32, one per fit), the hit arrays and the outputs are
 * DEVICE arrays -- a vertex seed's d_best_pos and d_best_bin can be passed as they lie; `offsets` (nfits +
 * 1 words) and `tau0` (nfits) are HOST arrays.  `timing` is read only with times (d_hit_time != NULL),
 * and of it only slowness, bin_ticks and nbins, with the vertex seed's ranges; d_bin and tau0 likewise are
 * needed only with times.  Per fit: d_best_dir (int32, 3), d_best_score, d_best_cand, d_inside, d_outside
 * (uint32), d_level_score (uint32, L + 1 per fit) and d_cos_hist (uint32, 2^m per fit; may be NULL).
 *
 * The function is total: no content of the hit, channel, vertex or bin arrays makes an access outside an
 * array.  Refused, CHROMA_ERR_INVALID before anything is launched on the fits and with nothing written: a
 * field of the seeder (or, with times, of `timing`) outside its range, a profile whose first 2^m entries
 * are all 0; ncand of 0 or above 2^20; nchannels above (2^32 - 1) / 3 or nfits above 2^31 - 1; a
 * candidate component beyond 2^15, a channel or vertex coordinate beyond 2^23 in magnitude (the device
 * arrays are checked by a validation pass whose verdict is read back first); offsets not starting at 0,
 * descending, or with a fit of more than 65535 hits; a NULL array that is needed (seeder always; the
 * candidates, offsets, vertices and the per-fit outputs but d_cos_hist when nfits; the channel positions
 * when nchannels and nfits; d_hit_channel and d_hit_weight when there are hits; timing, tau0 and d_bin with
 * times).  nfits == 0 is CHROMA_OK and writes nothing.
 *
 * Runs on the context's stream and returns when the outputs are written.  Scratch: the offsets, tau0, the
 * level-0 maxima (a 64-bit word per fit), the validation's verdict and an 8-byte record per hit. */
int chroma_direction_seed(chroma_ctx *ctx, const chroma_direction_seeder *seeder, const chroma_vertex_seeder *timing,
                          uint32_t nchannels, const int32_t *d_channel_pos, uint32_t ncand, const int32_t *d_cand,
                          uint32_t nfits, const uint32_t *offsets, const int32_t *tau0, const int32_t *d_vertex,
                          const uint32_t *d_bin, const int32_t *d_hit_channel, const int32_t *d_hit_time,
                          const uint32_t *d_hit_weight, int32_t *d_best_dir, uint32_t *d_best_score,
                          uint32_t *d_best_cand, uint32_t *d_inside, uint32_t *d_outside, uint32_t *d_level_score,
                          uint32_t *d_cos_hist);
/* The same on the host (no GPU, no context), plain loops on one thread: the same arguments on HOST arrays,
 * the same refusals, the same bits. */
int chroma_direction_seed_host(const chroma_direction_seeder *seeder, const chroma_vertex_seeder *timing,
                               uint32_t nchannels, const int32_t *channel_pos, uint32_t ncand, const int32_t *cand,
                               uint32_t nfits, const uint32_t *offsets, const int32_t *tau0, const int32_t *vertex,
                               const uint32_t *bin, const int32_t *hit_channel, const int32_t *hit_time,
                               const uint32_t *hit_weight, int32_t *best_dir, uint32_t *best_score,
                               uint32_t *best_cand, uint32_t *inside, uint32_t *outside, uint32_t *level_score,
                               uint32_t *cos_hist);

/* ---- PDFs and likelihood terms over DAQ output (chroma/cuda/pdf.cu) ------------------------
 * Every call reads the GPUChannels layout: `ndaq` copies of `nchannels` entries, copy i at
 * [i * stride, i * stride + nchannels) (stride >= nchannels).  An MC time >= 1e8 means "not hit".
 * The copies of a channel are taken in copy order, so one call over K copies gives the same bits as
 * K calls of one copy each.  All arrays are device arrays, accumulated into; launches go on the
 * context's stream.  CHROMA_ERR_INVALID for a bad layout, zero bins, an empty or inverted range. */
/* `bin_hits` (pdf.cu:9-32): per channel, copies with t < 1e8, tmin <= t < tmax, qmin <= q < qmax
 * (q truncated to an unsigned integer, negative -> 0) add 1 to hitcount and to the bin
 * (channel, tbin, qbin) of the row-major uint32 histogram; bin indices clamped to the histogram. */
int chroma_pdf_bin_hits(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                        const float *d_channel_q, const float *d_channel_t, int32_t tbins, float tmin,
                        float tmax, int32_t qbins, float qmin, float qmax, uint32_t *d_hitcount,
                        uint32_t *d_pdf);
/* `accumulate_bincount` + `accumulate_nearest_neighbor` (pdf.cu:34-219): per channel, copies with
 * an MC time < 1e8 inside [tmin, tmax] add 1 to hitcount; for the `nhit` channels the event hit,
 * listed in d_hit_channels (each at most once; d_event_hit non-zero there), d = |mc - event_time|
 * adds 1 to bincount when d < min_twidth / 2 and, while the running bincount is below
 * min_bin_content (1 .. 1024), is a candidate for d_nearest[h * min_bin_content ...]: the
 * min_bin_content smallest candidate distances of hit channel h so far, ascending, padded with 1e9
 * (initialise it so). */
int chroma_pdf_eval_accumulate(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                               const uint32_t *d_event_hit, const float *d_event_time, const float *d_mc_time,
                               uint32_t nhit, const uint32_t *d_hit_channels, float min_twidth, float tmin,
                               float tmax, int32_t min_bin_content, uint32_t *d_hitcount,
                               uint32_t *d_bincount, float *d_nearest);
/* `accumulate_moments` (pdf.cu:223-265): count, sum and sum of squares of the MC times (and charges
 * unless time_only; the charge arrays may be NULL when time_only) inside the closed ranges. */
int chroma_pdf_moments(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                       const float *d_mc_time, const float *d_mc_charge, float tmin, float tmax, float qmin,
                       float qmax, uint32_t *d_mom0, float *d_t_mom1, float *d_t_mom2, float *d_q_mom1,
                       float *d_q_mom2);
/* `accumulate_kernel_eval` (pdf.cu:267-368): per channel, copies inside the closed ranges add 1 to
 * hitcount and, on channels the event hit, a Gaussian kernel term (inverse bandwidths given per
 * channel) normalised inside the window to the PDF values.  Charge arrays may be NULL when time_only. */
int chroma_pdf_kernel_eval(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                           const uint32_t *d_event_hit, const float *d_event_time, const float *d_event_charge,
                           const float *d_mc_time, const float *d_mc_charge, float tmin, float tmax, float qmin,
                           float qmax, const float *d_inv_time_bandwidths, const float *d_inv_charge_bandwidths,
                           uint32_t *d_hitcount, float *d_time_pdf_values, float *d_charge_pdf_values);

/* Isotropic photon bomb generated on the device (the benchmark source of
 * chroma/benchmark.py:77-83, formulas chroma/sample.py:16-30), photon i drawn from
 * Philox stream (seed, 0xB0B0000000000000 + id_base + i).  wavelength_hi <= wavelength_lo
 * gives a mono-energetic bomb. */
int chroma_generate_bomb(chroma_ctx *ctx, const chroma_photon_arrays *photons, uint64_t nphotons,
                         uint64_t seed, uint64_t id_base, const float pos[3],
                         float wavelength_lo, float wavelength_hi);

/* ---- photons from charged-particle steps (csrc/steps_common.h: the per-segment and per-photon functions, compiled for
 * the device and for the host alike) ----
 * A SEGMENT is two consecutive step points A -> B of one track.  It emits Cherenkov light (Frank-Tamm: mean
 * 2 pi alpha z^2 L sum_trapezoid max(0, 1 - 1/(beta^2 n_j^2)) / lambda_j^2 d_lambda over the grid nodes cherenkov_lo ..
 * cherenkov_hi, L and lambda in one unit) and scintillation light (mean light_yield * qedep).  Counts: Poisson by Knuth's
 * product of uniforms for a mean <= 16, max(0, round(mean + sqrt(mean) * normal)) above.  Random streams: segment g =
 * segment_base + its index draws its two counts (Cherenkov first) from Philox stream word 0 of id 0x57E9000000000000 + g,
 * photon j of the segment (Cherenkov photons first) everything it needs from stream word 1 + j of the same id -- so a
 * photon does not depend on how the segments were split into calls.  The propagation stream (keyed by photon id) is not
 * touched: rng_counters of a generated photon is 0. */

/* One medium's tables, HOST pointers (the calls copy what they need), on the geometry's wavelength and time grids. */
typedef struct chroma_light_source {
    const float *refractive_index;    /* [wavelength_n] n at the grid nodes                                       */
    const float *scintillation_cdf;   /* [wavelength_n] CDF of the emission spectrum, 0 .. 1; NULL: no such light */
    const float *time_cdf;            /* [time_n] CDF of the emission delay, 0 .. 1; NULL: prompt                 */
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    float light_yield;                /* scintillation photons per unit of (quenched) deposit                    */
    uint32_t cherenkov_lo, cherenkov_hi;   /* first and last grid node of the Cherenkov range, lo < hi            */
} chroma_light_source;

/* The segments of one call as arrays (DEVICE pointers for the device calls, host pointers for the _host calls). */
typedef struct chroma_step_segments {
    const float *a, *b;               /* [n][3] the two step points, mm                                           */
    const float *t_a, *t_b;           /* [n] their times, ns                                                      */
    const float *beta;                /* [n] mean of the two points' beta                                         */
    const float *z;                   /* [n] charge in units of e; 0: no Cherenkov light                          */
    const float *qedep;               /* [n] quenched deposit of the step                                         */
    const uint32_t *evidx;            /* [n] event index given to the photons; NULL: 0                            */
    uint64_t n;
    uint64_t segment_base;            /* global index of segment 0                                                */
} chroma_step_segments;

/* Counts: d_offsets[2 n + 1] (uint32) gets the exclusive sum of (Cherenkov_0, scintillation_0, Cherenkov_1, ...), so the
 * photons of segment s are [d_offsets[2 s], d_offsets[2 s + 2]) of the output, Cherenkov before scintillation, and
 * d_offsets[2 n] == *total.  CHROMA_ERR_INVALID when the total does not fit 32 bits. */
int chroma_steps_count(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                       uint32_t *d_offsets, uint64_t *total);
/* The photons themselves, into the first d_offsets[2 n] slots of `photons` (all ten arrays; last_hit_triangles -1, weights 1,
 * rng_counters 0).  `capacity` < that total: CHROMA_ERR_INVALID and nothing is written.  Queued on the context's stream. */
int chroma_steps_generate(chroma_ctx *ctx, const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                          const uint32_t *d_offsets, const chroma_photon_arrays *photons, uint64_t capacity);
/* The same two calls as loops on the host (every pointer a host pointer): the same photons bit for bit. */
int chroma_steps_count_host(const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                            uint32_t *offsets, uint64_t *total);
int chroma_steps_generate_host(const chroma_light_source *src, const chroma_step_segments *segs, uint64_t seed,
                               const uint32_t *offsets, const chroma_photon_arrays *photons, uint64_t capacity);

/* ---- a medium per segment ----
 * The media of a detector as ONE device-resident table, a row per medium (for chroma_locate_materials' answers: a row per
 * material of the geometry), made once: the single-medium calls above copy their tables up on every call.  Row m is the
 * chroma_light_source with row m of each table, light_yield[m] (0: no scintillation light, the two CDF rows are ignored) and
 * time_cdf = prompt[m] ? NULL : row m; the grids and the Cherenkov range are the same for all rows.  Checked row by row as
 * one source is, and every CDF row that is read has to be finite and must not fall. */
typedef struct chroma_light_media_desc {
    uint32_t nmedia;
    const float *refractive_index;    /* [nmedia][wavelength_n]                                                   */
    const float *scintillation_cdf;   /* [nmedia][wavelength_n]; rows of media without such light are ignored     */
    const float *time_cdf;            /* [nmedia][time_n]; ditto                                                  */
    const float *light_yield;         /* [nmedia]; 0: no scintillation                                            */
    const uint8_t *prompt;            /* [nmedia]; 1: no time_cdf row, emission is prompt                         */
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n;       float time_start, time_step;
    uint32_t cherenkov_lo, cherenkov_hi;
} chroma_light_media_desc;            /* HOST pointers */
typedef struct chroma_light_media chroma_light_media;

/* The table on the device of `ctx` (blocks of chroma_malloc's pool); the desc's arrays are the caller's again on return. */
int chroma_light_media_create(chroma_ctx *ctx, const chroma_light_media_desc *desc, chroma_light_media **media);
/* Before chroma_shutdown of its context.  NULL: nothing. */
int chroma_light_media_destroy(chroma_light_media *media);

/* chroma_steps_count / chroma_steps_generate with segment s in row d_medium[s] (int32 [n], a DEVICE array; host for the
 * _host calls).  A segment whose row is negative or >= nmedia emits nothing: both its counts are 0.  Segment s in medium m
 * emits, bit for bit, what the single-medium call emits for it with medium m's chroma_light_source, seed and global segment
 * index being the same.  Layout, offsets, the 32-bit refusal and the capacity rule are those of the calls above. */
int chroma_steps_count_media(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs,
                             const int32_t *d_medium, uint64_t seed, uint32_t *d_offsets, uint64_t *total);
int chroma_steps_generate_media(chroma_ctx *ctx, const chroma_light_media *media, const chroma_step_segments *segs,
                                const int32_t *d_medium, uint64_t seed, const uint32_t *d_offsets,
                                const chroma_photon_arrays *photons, uint64_t capacity);
int chroma_steps_count_media_host(const chroma_light_media_desc *desc, const chroma_step_segments *segs, const int32_t *medium,
                                  uint64_t seed, uint32_t *offsets, uint64_t *total);
int chroma_steps_generate_media_host(const chroma_light_media_desc *desc, const chroma_step_segments *segs, const int32_t *medium,
                                     uint64_t seed, const uint32_t *offsets, const chroma_photon_arrays *photons,
                                     uint64_t capacity);

/* ---- charged particles stepped through the detector (continuous slowing down) ----
 * What makes the step points the calls above start from.  Units: MeV, mm, ns.  A particle loses the MEAN stopping power of the
 * medium it is in (a table per medium and species, read by linear interpolation in log ke, the end nodes' values beyond them),
 * in steps limited by `max_step`, by the fraction `max_loss` of its kinetic energy, and by the next volume boundary (the
 * engine's own ray cast); at the end of a step its direction is scattered by the Highland formula.  No secondaries, no
 * straggling, no lateral displacement: see DESIGN.md 3.8.
 *
 * Random streams: particle p = particle_base + its index draws from Philox stream word 0 of id 0x9A27000000000000 + p, from
 * its own counter (rng_counter) on: a track does not depend on how particles are split over calls. */
#define CHROMA_PARTICLE_SPECIES 6      /* the rows of a medium, by |pdg code|: e, mu, pi, K, p, alpha */
#define CHROMA_PARTICLE_ALIVE     0u
#define CHROMA_PARTICLE_STOPPED   1u   /* its kinetic energy fell below ke_cut: all of it deposited          */
#define CHROMA_PARTICLE_LEFT      2u   /* in no medium of the table, or in vacuum with no triangle ahead      */
#define CHROMA_PARTICLE_TRUNCATED 3u   /* max_steps steps made                                                */
#define CHROMA_PARTICLE_UNTRACKED 4u   /* unknown or neutral species, or no kinetic energy: the vertex alone  */
#define CHROMA_PARTICLE_NAN_ABORT 5u   /* a NaN in its position or direction                                  */

typedef struct chroma_stopping_media_desc {
    uint32_t nmedia, nke;
    float ke_min, log_step;           /* node j: ke_min * exp(j * log_step) MeV                                   */
    const float *stopping_power;      /* [nmedia][CHROMA_PARTICLE_SPECIES][nke] MeV/mm, finite and not negative   */
    const float *radiation_length;    /* [nmedia] mm, above 0; +inf: no scattering (vacuum)                       */
    const float *birks;               /* [nmedia] mm/MeV: qedep = edep / (1 + birks * S)                          */
} chroma_stopping_media_desc;         /* HOST pointers */
typedef struct chroma_stopping_media chroma_stopping_media;

/* The table on the device of `ctx` (one block of chroma_malloc's pool); the desc's arrays are the caller's again on return. */
int chroma_stopping_media_create(chroma_ctx *ctx, const chroma_stopping_media_desc *desc, chroma_stopping_media **media);
/* Before chroma_shutdown of its context.  NULL: nothing. */
int chroma_stopping_media_destroy(chroma_stopping_media *media);

/* The particles of one call as arrays (DEVICE pointers for the device calls, host pointers for the _host calls); all are read
 * and, but for species, z, mass and evidx, written.  A particle enters with status ALIVE and nsteps 0. */
typedef struct chroma_particle_arrays {
    float *pos, *dir;                 /* [n][3] mm; unit vector                                                   */
    float *ke, *t;                    /* [n] kinetic energy MeV, time ns                                          */
    int32_t *last_hit;                /* [n] the triangle the last step ended on (the next cast excludes it), -1  */
    int32_t *species;                 /* [n] row 0 .. 5 of the medium's table; -1: unknown or neutral             */
    float *z, *mass;                  /* [n] charge in e, mass in MeV                                             */
    uint32_t *evidx;                  /* [n] event index handed to the segments                                   */
    uint32_t *nsteps;                 /* [n] steps made: the particle has nsteps + 1 points                       */
    uint32_t *rng_counter;            /* [n] draws taken from the particle's stream                               */
    uint32_t *status;                 /* [n] CHROMA_PARTICLE_*                                                    */
    uint64_t n;
    uint64_t particle_base;           /* global index of particle 0                                               */
} chroma_particle_arrays;

typedef struct chroma_particle_options {
    int32_t max_steps;                /* steps per particle, 1 .. 2^20                                            */
    float max_step;                   /* mm                                                                       */
    float max_loss;                   /* largest fraction of ke lost in one step, (0, 1]                          */
    float ke_cut;                     /* MeV: a particle that would fall below deposits the rest and stops        */
    int32_t scatter;                  /* 0: straight tracks                                                       */
    int32_t outside;                  /* the medium row of a particle with no triangle ahead; -1: none            */
} chroma_particle_options;

/* Step points as columns: point 0 of a particle is its vertex (zero deposits, medium -1), point k the end of step k with the
 * kinetic energy left, the step's deposit, its quenched deposit and the medium it was made in.  As a MATRIX of the calls
 * below: point k of particle i is row k * n + i of n * (max_steps + 1) rows. */
typedef struct chroma_particle_points {
    float *pos, *t, *dir, *ke, *edep, *qedep;      /* [rows][3], [rows], [rows][3], [rows] ...  */
    int32_t *medium;                               /* [rows]                                    */
} chroma_particle_points;

/* ONE iteration for every ALIVE particle i, given the nearest triangle along its direction (d_distance[i], d_triangle[i]: a
 * triangle < 0 or a distance that is not finite means none; NULL arrays: none for all) and the medium row on the particle's
 * side of it (d_medium[i]; NULL: options->outside for all).  A particle's first iteration writes its vertex as well.  Points
 * go to the matrix `points`.  Queued on the context's stream. */
int chroma_particles_advance(chroma_ctx *ctx, const chroma_stopping_media *media, const chroma_particle_arrays *particles,
                             const chroma_particle_options *options, uint64_t seed, const float *d_distance,
                             const int32_t *d_triangle, const int32_t *d_medium, const chroma_particle_points *points);
int chroma_particles_advance_host(const chroma_stopping_media_desc *desc, const chroma_particle_arrays *particles,
                                  const chroma_particle_options *options, uint64_t seed, const float *distance,
                                  const int32_t *triangle, const int32_t *medium, const chroma_particle_points *points);

/* Every particle to its end: per iteration the ray cast of chroma_intersect_mesh for the live particles (pos, dir, last_hit),
 * the medium from the hit triangle's side by fill_state's rule on the particle's own direction (outer material when
 * dot(normal, -dir) > 0, inner otherwise; no triangle: options->outside), one iteration as above, and the particles still
 * ALIVE queued for the next.  `geom` NULL: no boundaries, every particle in row options->outside.  The points stay in the
 * context's pooled scratch as a matrix until another call of the context uses it; chroma_particles_points /
 * chroma_particles_segments, called next, read them, and `particles` has to live until then.  *total_points = the sum of
 * nsteps + 1.  CHROMA_ERR_INVALID with a message when the matrix cannot be allocated.  Returns when the tracks are done. */
int chroma_particles_track(chroma_ctx *ctx, chroma_geometry *geom, const chroma_stopping_media *media,
                           const chroma_particle_arrays *particles, const chroma_particle_options *options, uint64_t seed,
                           uint64_t *total_points);
/* The loop with geom == NULL on the host, into the caller's matrix `points`. */
int chroma_particles_track_host(const chroma_stopping_media_desc *desc, const chroma_particle_arrays *particles,
                                const chroma_particle_options *options, uint64_t seed, const chroma_particle_points *points,
                                uint64_t *total_points);

/* The points of the last chroma_particles_track of `ctx` as flat arrays in particle order: d_offsets[n + 1] (uint32) gets the
 * exclusive sum of the particles' point counts, the points of particle i are [d_offsets[i], d_offsets[i + 1]) of `out`.
 * `capacity` below the total: CHROMA_ERR_INVALID and nothing is written.  Queued on the context's stream. */
int chroma_particles_points(chroma_ctx *ctx, const chroma_particle_points *out, uint32_t *d_offsets, uint64_t capacity);
/* ... and its sum of nsteps segments (points k -> k + 1 of one particle) in particle order, straight into the arrays of a
 * chroma_step_segments (`out`: its eight arrays, written; n and segment_base are not read) and d_medium, for
 * chroma_steps_count_media / chroma_steps_generate_media: beta = 0.5f * (beta_a + beta_b) of the two points' kinetic energies,
 * qedep and medium those of point k + 1.  `capacity` below the total: CHROMA_ERR_INVALID and nothing is written. */
int chroma_particles_segments(chroma_ctx *ctx, const chroma_step_segments *out, int32_t *d_medium, uint64_t capacity);
/* The same from a host matrix (`particles`: nsteps, z, mass, evidx are read; `max_steps`: the matrix's). */
int chroma_particles_points_host(const chroma_particle_arrays *particles, int32_t max_steps, const chroma_particle_points *matrix,
                                 const chroma_particle_points *out, uint32_t *offsets, uint64_t capacity);
int chroma_particles_segments_host(const chroma_particle_arrays *particles, int32_t max_steps, const chroma_particle_points *matrix,
                                   const chroma_step_segments *out, int32_t *medium, uint64_t capacity);

/* tools.argsort_direction (chroma/tools.py:175-193) and the reordering it serves, for a photon set on the device: the
 * photons are put in the order of a 32-bit Morton code of (theta, phi) of their directions (stable), every array of
 * the set gathered accordingly.  The reference's own benchmark does this to its photons before it starts the clock
 * (chroma/benchmark.py:80-82); bench.py does the same to its bomb.  Slot i afterwards holds the photon of rank i. */
int chroma_photons_sort_direction(chroma_ctx *ctx, const chroma_photon_arrays *photons, uint64_t nphotons);

/* Flat hits (what chroma_copy_photon_hits / chroma_propagate_hits left in `hits` and `d_channels`) put in (evidx, channel) order, in
 * place and stably: the split by event and by channel that the reference's callers do next with one mask over all hits per event and
 * per channel (chroma/sim.py:118-123, chroma/gpu/photon.py:96-105) is then a matter of slices.  The reference leaves the order of
 * flat hits unspecified (its compaction goes through an atomic); this is one valid order. */
int chroma_hits_sort(chroma_ctx *ctx, const chroma_photon_arrays *hits, int32_t *d_channels, uint64_t nhits);

/* `render` (chroma/cuda/render.cu:37-181): every triangle along each ray, the `alpha_depth` nearest kept as
 * a per-ray list sorted by distance (d_dx [n][alpha_depth], d_color [n][alpha_depth][4], d_dxlen [n]: in and
 * out, so that a second call continues the first -- GPURays.render(keep_last_render=True)), composited
 * front to back over bg_color into d_pixels [n] (0xAARRGGBB).  Directions are used as given (not normalised). */
int chroma_render(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const float *d_origin, const float *d_direction,
                  uint32_t alpha_depth, uint32_t *d_pixels, float *d_dx, uint32_t *d_dxlen, float *d_color, uint32_t bg_color);
/* The hybrid render (chroma/cuda/hybrid_render.cu; chroma/camera.py:188-249 drives it).  Both sample passes follow a photon
 * with the propagate physics (all models, no weights) to its FIRST diffuse reflection, and stop there, on any terminal
 * outcome, on a miss, on the NaN abort or after max_steps steps.  Thread k draws from the Philox stream
 * (rng.seed, rng.photon_id_base + k) starting at d_rng_counters[k], and writes the advanced counter back: the caller's
 * counter array (ncounters entries) plays the part of the reference's rng_states.  Lookup tables and images are float3
 * arrays; the tables hold one entry per triangle (nlookup must equal the triangle count).  Optional per-thread sample
 * outputs (give all or none): the diffusing triangle or -1, its side (1 = inside to outside, the reference's
 * State::inside_to_outside), the final history, and (lookup) cos_theta.  Sizes, ranges and max_steps >= 0 are checked
 * before any launch (CHROMA_ERR_INVALID; CHROMA_ERR_STACK for a BVH deeper than the walk supports).
 *
 * chroma_hybrid_lookup (update_xyz_lookup): thread k samples triangle offset + k, for k < nthreads and offset + k below
 * both total_threads and the triangle count (other threads draw nothing).  A sample whose ray from `position` first hits
 * its own triangle and then diffuses adds cos_theta * xyz to the diffusing triangle's entry of d_lookup1 (inside to
 * outside) or d_lookup2.  Deterministic: the contributions of one call are summed per (triangle, side) in sample order in
 * f32, and each sum is added once to its entry.
 * chroma_hybrid_image (update_xyz_image): ray k (k < nthreads <= nimage) adds xyz * lookup[triangle] / nlookup_calls
 * (nlookup_calls >= 1) to d_image[k].
 * chroma_hybrid_pixels (process_image): d_pixels[k] = 0xFF << 24 | r << 16 | g << 8 | b of d_image[k] / nimages
 * (nimages >= 1), each channel clamped to [0, 1] (NaN to 0) and floorf(x * 255). */
int chroma_hybrid_lookup(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, int32_t total_threads, int32_t offset,
                         const float position[3], chroma_rng rng, uint32_t *d_rng_counters, uint32_t ncounters, float wavelength,
                         const float xyz[3], float *d_lookup1, float *d_lookup2, uint32_t nlookup, int32_t max_steps,
                         int32_t *d_sample_triangle, uint32_t *d_sample_side, uint32_t *d_sample_history, float *d_sample_cos);
int chroma_hybrid_image(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, chroma_rng rng, uint32_t *d_rng_counters,
                        uint32_t ncounters, const float *d_positions, const float *d_directions, float wavelength, const float xyz[3],
                        const float *d_lookup1, const float *d_lookup2, uint32_t nlookup, float *d_image, uint32_t nimage,
                        int32_t nlookup_calls, int32_t max_steps, int32_t *d_sample_triangle, uint32_t *d_sample_side,
                        uint32_t *d_sample_history);
int chroma_hybrid_pixels(chroma_ctx *ctx, int32_t nthreads, const float *d_image, uint32_t *d_pixels, int32_t nimages);
/* `color_solids` (chroma/cuda/mesh.h:153-166; host: GPUGeometry.color_solids, chroma/gpu/geometry.py:283-298): triangle t of
 * [first_triangle, first_triangle + ntriangles) takes d_solid_colors[solid_id_map[t]] where d_solid_hit[solid_id_map[t]] is set
 * (one byte per solid, as numpy bool); both arrays hold `nsolids` entries, a triangle of a solid beyond them keeps its colour.
 * Writes the geometry's `colors` array, the one chroma_render reads. */
int chroma_color_solids(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_triangle, int32_t ntriangles, const uint8_t *d_solid_hit,
                        const uint32_t *d_solid_colors, uint32_t nsolids);
/* `translate`, `rotate`, `rotate_around_point` (chroma/cuda/transform.cu:9-53) on a float3 array */
int chroma_points_translate(chroma_ctx *ctx, int32_t n, float *d_a, const float v[3]);
int chroma_points_rotate(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3]);
int chroma_points_rotate_around_point(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3], const float point[3]);

/* ---- the hit reduction across the GPUs of a node ------------------------------
 * The reference has no multi-GPU mode.  Here one process drives one GPU, photons are sharded by
 * global id, the geometry is replicated, and the ONE exchange per batch is the per-channel arrays:
 * RCCL over xGMI, on the library's stream, in place on the device arrays chroma_channel_hits /
 * chroma_daq_acquire filled.  Rendezvous: one rank calls chroma_comm_unique_id and hands the 128
 * bytes to the others by any means (bench.py: torch.distributed broadcast); every rank then calls
 * chroma_comm_init.  Without a communicator the reductions are the identity (single GPU). */
#define CHROMA_COMM_ID_BYTES 128
int chroma_comm_unique_id(uint8_t id[CHROMA_COMM_ID_BYTES]);
int chroma_comm_init(chroma_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[CHROMA_COMM_ID_BYTES]);
int chroma_comm_destroy(chroma_ctx *ctx);
/* hit_count: sum; earliest-time bit patterns: min (valid for t >= 0, chroma/cuda/daq.cu:5-20); d_earliest may be NULL */
int chroma_allreduce_hits(chroma_ctx *ctx, uint32_t *d_hit_count, uint32_t *d_earliest_time_bits, uint32_t nchannels);
/* DAQ accumulators of sharded photons (chroma/cuda/daq.cu:73-75): time bits min, integer charge sum, histories OR */
int chroma_allreduce_daq(chroma_ctx *ctx, uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                         uint32_t *d_channel_histories, uint32_t nchannels);

/* Test probe: ONE call per element of a single device function of the propagate path, so that tests
 * can pin the engine's own device code on the CPU oracle and on the reference's headers compiled for
 * gfx950 (oracle/ref_headers_driver.hip).  All pointers are device pointers.
 *   fn 0  interp_property (chroma/cuda/geometry.h:64-75)   d_x[n], d_tab_f[ntab], grid (start, step)
 *   fn 1  interp_idx (chroma/cuda/interpolate.h:5-29)      d_x[n], d_tab_x[ntab]
 *   fn 2  interp (chroma/cuda/interpolate.h:32-57)         d_x[n], d_tab_x[ntab], d_tab_f[ntab]
 *   fn 3  rotate (chroma/cuda/rotate.h:22-28)              d_x[7 n] = a.xyz, phi, axis.xyz -> d_out[5 n] = r.xyz, cos phi, sin phi
 *   fn 4  the float3 algebra (chroma/cuda/linalg.h)        d_x[7 n] = a.xyz, b.xyz, c -> d_out[32 n] = -a, a+b, a-b, a*c, c*a, a/c, c/a,
 *                                                          cross(a,b), dot(a,b), norm(a), normalize(a), a/b */
int chroma_probe(chroma_ctx *ctx, int32_t fn, uint64_t n, const float *d_x, const float *d_tab_x, const float *d_tab_f,
                 uint32_t ntab, float start, float step, float *d_out);

/* Test probe of the numeric contract: ONE call per element of a single primitive of include/chroma_math.h as compiled
 * for the device, so that tests (tests/test_gpu_math_contract.py) can hold it bit for bit to the host compiler's build of
 * the same header (the CPU oracle: oracle_math, oracle_rng_probe, same numbering).  All pointers are device pointers to
 * 32-bit words: a float travels as its bits, integer results are written as they are.  Arrays an op does not read may
 * be NULL.  n < 2^31.
 *   op  0 cm_logf    1 cm_expf    2 cm_sinf    3 cm_cosf   4 cm_tanf   5 cm_asinf   6 cm_acosf      d_x[n] -> d_out[n]
 *       8 cm_sqrtf  10 cm_atanf  11 cm_floorf 12 cm_roundf                                           d_x[n] -> d_out[n]
 *       9 cm_u32_to_uniform (d_x[n]: the words)   13 cm_f2i   14 cm_f2u32 (d_out[n]: the integers)   d_x[n] -> d_out[n]
 *       7 cm_atan2f(x, y)   15 x / y   16 cm_fminf(x, y)   17 cm_fmaxf(x, y)                  d_x[n], d_y[n] -> d_out[n]
 *      18 cm_fmaf(x, y, z)                                                            d_x[n], d_y[n], d_z[n] -> d_out[n]
 *      19 cm_philox4x32_10   d_x[6 n] = counter words 0..3, key words 0..1 -> d_out[4 n]
 *      20 cm_rng_uniform     d_x[6 n] = seed lo, seed hi, photon id lo, id hi, stream word, start counter
 *                            -> d_out[8 n]: the 8 draws that follow
 *      21 cm_rng_normal      d_x[6 n] as for 20 -> d_out[4 n]: the 4 normal deviates (two uniforms each) that follow */
int chroma_probe_math(chroma_ctx *ctx, int32_t op, uint64_t n, const void *d_x, const void *d_y, const void *d_z, void *d_out);

/* ---- host-side BVH construction -------------------------------------------------------
 * Recursive-grid builder: replaces make_recursive_grid_bvh (chroma/bvh/grid.py:11-95) and the
 * kernels it drives -- make_leaves, make_parents_detailed, copy_and_offset, collapse_child
 * (chroma/cuda/bvh.cu:149-203,270-308,365-384,530-543; hosts chroma/gpu/bvh.py:18-130,239-267).
 * Runs on the host cores (no device needed).  Two-phase: build returns a handle and the sizes,
 * fetch copies nodes ([nnodes][4] uint32) and layer bounds ([nlayers+1] uint64), free releases.
 * Both builders return CHROMA_ERR_INVALID with a message, before any work is done, for target_degree < 2 (with
 * distinct Morton codes a degree of 1 gives every node a parent of its own and the tree never closes) and for a frame
 * that cannot quantise: world_scale not finite or <= 0 (a mesh without extent), or a non-finite world_origin (a mesh
 * with non-finite vertices).  For vertices outside [origin, origin + 65535 * scale] the result is unspecified: the
 * conversion of the quantised float to uint32 saturates on the device and wraps on the host. */
int chroma_bvh_build(const float *vertices, uint32_t nvertices, const uint32_t *triangles, uint32_t ntriangles,
                     const float world_origin[3], float world_scale, int32_t target_degree,
                     void **handle, uint64_t *nnodes, uint32_t *nlayers);
/* The same builder ON THE DEVICE of `ctx` (csrc/bvh_device.hip), as in the reference, where these steps ARE device
 * kernels: leaf boxes + 48-bit Morton codes (bvh.cu:149-203), a device radix sort (grid.py:26-28), group boundaries by
 * one histogram pass and two scans (grid.py:37-76), parent unions per layer (bvh.cu:270-308), concatenate + offset
 * (bvh.cu:365-384), collapse (bvh.cu:530-543).  Host arrays in, the same kind of handle out, and the SAME node array
 * bit for bit as chroma_bvh_build (tests/test_gpu_bvh.py). */
int chroma_bvh_build_device(chroma_ctx *ctx, const float *vertices, uint32_t nvertices, const uint32_t *triangles,
                            uint32_t ntriangles, const float world_origin[3], float world_scale, int32_t target_degree,
                            void **handle, uint64_t *nnodes, uint32_t *nlayers);
int chroma_bvh_fetch(void *handle, uint32_t *nodes_out, uint64_t *layer_bounds_out);
/* zero-copy access to the arrays owned by the handle (valid until chroma_bvh_free) */
int chroma_bvh_data(void *handle, const uint32_t **nodes, const uint64_t **layer_bounds);
int chroma_bvh_free(void *handle);

/* ---- derived traversal tree ------------------------------------------------------------
 * chroma_geometry_create derives, from the reference-format nodes it is given, the tree the ray
 * cast actually walks on MI355X: 8-wide nodes of 128 bytes (one L2 line) whose entries are boxes
 * of the reference tree (chroma/cuda/geometry_types.h:57-67 format, w = child wide node, or
 * 0x80000000 | record index of a triangle, or 0xFFFFFFFF for an empty slot), the order of the
 * 48-byte triangle records, and each triangle's position in the test order of the reference
 * walk (chroma/cuda/mesh.h:68-110), which breaks exact distance ties the way the reference does.
 * These entry points expose that host-side step on its own (no device needed) for inspection
 * and tests; arrays stay owned by the handle until chroma_wide_free.
 *   wnodes      [nwide][8][4] uint32      tri_to_record [ntriangles] uint32
 *   record_to_tri [nrecords] uint32       rank [ntriangles] uint32 (0xFFFFFFFF: under no leaf) */
int chroma_wide_build(const uint32_t *nodes, uint64_t nnodes, uint32_t ntriangles, void **handle,
                      uint64_t *nwide, uint64_t *nrecords, uint32_t *depth);
/* The same step ON THE DEVICE of `ctx` (csrc/wide_device.hip): HIP kernels over one level of the tree at a time -- the
 * place where the reference builds its own tree (chroma/gpu/bvh.py, chroma/cuda/bvh.cu run on the GPU).  The result is the
 * tree CHROMA_TREE=levels makes on the host, bit for bit (tests/test_gpu_wide.py); same handle, same accessors. */
int chroma_wide_build_device(chroma_ctx *ctx, const uint32_t *nodes, uint64_t nnodes, uint32_t ntriangles, void **handle,
                             uint64_t *nwide, uint64_t *nrecords, uint32_t *depth);
int chroma_wide_data(void *handle, const uint32_t **wnodes, const uint32_t **tri_to_record,
                     const uint32_t **record_to_tri, const uint32_t **rank);
int chroma_wide_free(void *handle);
/* Index checks chroma_geometry_create runs on the derived tree before it uploads anything (every
 * inner child word names a later wide node, every leaf word a record < nrecords, every record a
 * triangle < ntriangles, every triangle a record that names it back): CHROMA_OK or CHROMA_ERR_INVALID.
 * The device buffers are sized from exactly these counts, so a tree that passes cannot index past them. */
int chroma_wide_validate(const uint32_t *wnodes, uint64_t nwide, const uint32_t *tri_to_record, uint32_t ntriangles,
                         const uint32_t *record_to_tri, uint64_t nrecords);

/* Merge identical vertices of a flattened mesh: replaces Mesh.remove_duplicate_vertices
 * (chroma/geometry.py:58-67, np.unique on a structured view) for large meshes.  The survivors
 * are written to `unique_out` ([nvertices][3] capacity) in lexicographic (x, y, z) order and
 * `triangle_indices` ([nindices], may be NULL) is remapped in place.  Host-side, all cores. */
int chroma_dedupe_vertices(const float *vertices, uint64_t nvertices, uint32_t *triangle_indices,
                           uint64_t nindices, float *unique_out, uint64_t *nunique);

/* accumulated counters of chroma_propagate_step launches since the last read */
int chroma_propagate_stats_read(chroma_ctx *ctx, chroma_propagate_stats *stats);
/* enable (1) / disable (0) node/triangle visit counting in the propagate kernels */
int chroma_set_counting(chroma_ctx *ctx, int32_t enabled);

/* Which tree the one-step ray cast walks, and how.
 *
 * The fast walks (QUAD, the default; PAIR, COOP, WIDE) go through the derived 8-wide tree nearest-first.  They agree
 * with EACH OTHER on every ray, and with the reference (chroma/cuda/mesh.h:42-118) on every ray whose winning
 * triangle's Moeller-Trumbore hit lies inside that triangle's own leaf box -- i.e. every hit that is geometrically one.
 * They do NOT reproduce the reference on rays for which mesh.h:82-101 accepts a numerically erratic hit: a ray almost
 * inside a triangle's plane (determinant above the FLT_EPSILON cut of intersect.h:58 but tiny) can "hit" hundreds of
 * millimetres in FRONT of the triangle's box; the reference's depth-first order may meet that triangle before any
 * nearer one and keep the bogus distance, while a nearest-first walk has pruned the box.
 * Measured: 0 of 2.4e8 random bomb photons on the 10k- and 29k-PMT detectors, ~2e-6 of rays aimed exactly at mesh
 * vertices / edge midpoints / centroids (profiles/r02/parity_sweep_*.txt; tests/test_gpu_exact_walk.py checks the
 * invariant "a ray on which QUAD and LITERAL differ is one whose reference hit lies outside its leaf box").
 *
 * LITERAL is the reference's loop as it stands -- its tree, its child order, its float box arithmetic, every triangle
 * tested the moment its leaf box is entered -- for EVERY ray, one ray per lane: the one mode that returns the
 * reference's triangle on every ray, the erratic ones included; several times slower (bench.py reports its rate as
 * config.exact_walk_photons_per_s).  GPUPhotons.propagate(exact=True), Simulation(exact=True) and chroma-sim --exact
 * select it per call.  REFERENCE walks the reference's tree in the reference's order but postpones triangle tests by up
 * to 8 per lane (a superset of the reference's tests in the same order): a cross-check walk, equal to LITERAL except
 * where an erratic hit belongs to a triangle the reference had already pruned.  chroma_intersect_mesh /
 * chroma_distance_to_mesh run the literal loop under both REFERENCE and LITERAL.
 * Env CHROMA_WALK=literal|reference|wide|coop|quad|pair sets the initial mode of a context. */
#define CHROMA_WALK_REFERENCE 0
#define CHROMA_WALK_WIDE      1
#define CHROMA_WALK_COOP      2
#define CHROMA_WALK_QUAD      3   /* the wide tree with four lanes per ray, two child entries per lane */
#define CHROMA_WALK_PAIR      4   /* the wide tree with two lanes per ray, four child entries per lane  */
#define CHROMA_WALK_LITERAL   5   /* chroma/cuda/mesh.h:42-118 literally, for every ray: exact (k_raycast_literal: four lanes per ray) */
#define CHROMA_WALK_LITERAL_LANE 6 /* the same loop with one lane per ray and no refill (intersect_mesh_strict): LITERAL's cross-check */
int chroma_set_walk(chroma_ctx *ctx, int32_t mode);

/* The first step of a chroma_propagate call can go to k_raycast_packet: 64 rays per wavefront walk the wide tree as ONE
 * packet (one stack, scalar node fetches, every triangle tested by all lanes whose ray enters its box) -- the same
 * results as the default walk, lane by lane, whatever the rays; much faster when the photons of neighbouring slots are
 * coherent (a direction-sorted bomb as chroma/benchmark.py:80-82 prepares it, a Cherenkov cone), much slower when they
 * are not.  AUTO: k_load_working looks at the photons (same origin, within 50 mrad, per wave of 64) and the packet kernel
 * takes the step when three quarters of the waves are coherent.  OFF is the default: measured on the 29k-PMT detector the
 * packet kernel is no faster than the default walk even on perfectly coherent rays (31.3 against 29.5 ms per 1e8 rays,
 * profiles/r03/ab_packet_first_step.txt: the union of 64 paths costs what the shared bookkeeping saves), so it stays an
 * opt-in with its parity tests.  Env CHROMA_PACKET=off|on|auto. */
#define CHROMA_PACKET_OFF  0
#define CHROMA_PACKET_ON   1
#define CHROMA_PACKET_AUTO 2
int chroma_set_packet(chroma_ctx *ctx, int32_t mode);

/* The ORDER in which a large chroma_propagate call (>= 2^21 photons, ncopies 1, default walk) takes its photons up.  Nothing
 * in the result depends on it (streams are keyed by photon id, results stored by photon id), the time does: rays of
 * neighbouring slots that walk the same part of the tree make the first launches of a call a quarter faster -- which is why
 * the reference's benchmark sorts its photons with tools.argsort_direction before the clock starts (chroma/benchmark.py:80-82).
 * AUTO: a sample of the input decides -- one origin and directions all over the place (a bomb or a calibration
 * source in generation order) are ordered by a 16-bit direction cell on the device (one radix sort of indices; the photon
 * arrays stay as they are); photons that are coherent already, or that come from many places, are taken as they come.
 * ON: every large call.  OFF (default): never -- measured at 1e8 photons on the 29k-PMT detector the index sort and the
 * gather through it cost 50 ms to win 15 (profiles/r03/ab_autosort.txt), so ordering stays the caller's preparation
 * (chroma_photons_sort_direction, as the reference's benchmark does it before its clock starts).
 * Env CHROMA_AUTOSORT=off|on|auto.  stats.reordered counts the photons so taken. */
#define CHROMA_AUTOSORT_OFF  0
#define CHROMA_AUTOSORT_ON   1
#define CHROMA_AUTOSORT_AUTO 2
int chroma_set_autosort(chroma_ctx *ctx, int32_t mode);

/* How chroma_propagate finishes a batch and, with FUSED, how it runs it at all (same results; for
 * tests and benchmarks).  COOP: per-step launch sets, then ONE cooperative launch for all remaining
 * steps once fewer than 8192 photons are alive.  SPLIT: per-step launch sets to the end.  FUSED: the
 * reference's own shape (chroma/gpu/photon.py:225-252) -- the lane-per-photon kernel of
 * chroma_propagate_step, one step per launch, then all remaining steps in one.
 * Env CHROMA_TAIL=coop|split|fused sets the initial mode of a context. */
#define CHROMA_TAIL_COOP  0
#define CHROMA_TAIL_SPLIT 1
#define CHROMA_TAIL_FUSED 2
int chroma_set_tail(chroma_ctx *ctx, int32_t mode);

#ifdef __cplusplus
}
#endif
#endif /* CHROMA_HIP_H */
