// ref_physics_driver.cc -- TEST INFRASTRUCTURE.  A HOST driver around the reference's OWN physics, DAQ and hybrid-render
// sources, compiled by g++ from where they lie (found through -I, see oracle/Makefile; nothing is copied):
// chroma/cuda/propagate.cu (the `propagate` kernel, :217-319) with photon.h (fill_state, Rayleigh scattering, bulk
// absorption and re-emission, Fresnel, both reflectors, the thin film, WLS, dichroic), random.h, cx.h, mesh.h,
// intersect.h, geometry.h, rotate.h, interpolate.h, linalg.h; and chroma/cuda/daq.cu (run_daq :35-86, run_daq_many
// :88-150); and chroma/cuda/hybrid_render.cu (fAtomicAdd, to_diffuse :20-58, update_xyz_lookup :63-131, update_xyz_image
// :133-168, process_image :170-200) with matrix.h.  The CUDA names those sources use come from the stand-ins of
// oracle/ref_shim (the project's own text).
//
// What this pins, and what it cannot: the reference's statements run as written -- every branch, every rescaling,
// every clamp, which statement draws and in what order.  The random stream is the project's per-photon Philox stream
// behind the names curand_uniform / curand_normal (the reference's XORWOW has no counterpart here), so the generator,
// the mapping of a word to (0, 1] and the Box-Muller normal deviate stay the project's own contract.
//
// Built twice: against the host libm (libchroma_ref_physics_libm.so, the comparand of liboracle_libm.so) and with
// the transcendental calls of the reference sources mapped onto include/chroma_math.h (-DREF_PHYS_CONTRACT:
// libchroma_ref_physics_contract.so, the comparand of liboracle.so and so of the HIP engine).
//
// One host thread runs the threads of a block in order, thread 0 first (see ref_shim/cuda_host_shim.h).
#include <vector>

#include "cuda_host_shim.h"
#include "curand_kernel.h"
#include "cuComplex.h"
#include "../include/chroma_hip.h"

#ifdef REF_PHYS_CONTRACT
// Every transcendental call of the reference sources, the untyped `exp` of photon.h:446,477,508 included (in C++ it
// resolves to the float overload).  sqrtf, fabsf, fminf, fmaxf and roundf are exact IEEE operations and stay.
#define sinf    cm_sinf
#define cosf    cm_cosf
#define tanf    cm_tanf
#define asinf   cm_asinf
#define acosf   cm_acosf
#define atan2f  cm_atan2f
#define logf    cm_logf
#define expf    cm_expf
#define exp     cm_expf
#define sincosf cm_sincosf
#endif

#include "propagate.cu"
#include "daq.cu"
#include "hybrid_render.cu"

#ifdef REF_PHYS_CONTRACT
#undef sinf
#undef cosf
#undef tanf
#undef asinf
#undef acosf
#undef atan2f
#undef logf
#undef expf
#undef exp
#undef sincosf
#endif

namespace {

// The reference's pointer-linked Geometry / Material / Surface / DichroicProps (geometry_types.h) over the tables of
// a chroma_geometry_desc.  Every table is copied with ONE extra float behind it that repeats the last value: the
// reference's interp_property reads fp[jl + 1] for a wavelength exactly on the last grid point (geometry.h:72-74,
// an out-of-bounds read multiplied by a zero distance), and inside a table that read is the next row's first value.
struct World {
    std::vector<std::vector<float> > tables;
    std::vector<Material> materials;
    std::vector<Material *> material_ptrs;
    std::vector<std::vector<float *> > row_ptrs;
    std::vector<Surface> surfaces;
    std::vector<Surface *> surface_ptrs;
    std::vector<DichroicProps> dichroics;
    Geometry g;

    float *table(const float *src, size_t count)
    {
        tables.emplace_back(count + 1, 0.0f);
        std::vector<float> &t = tables.back();
        if (src && count) {
            memcpy(t.data(), src, count * sizeof(float));
            t[count] = src[count - 1];
        }
        return t.data();
    }

    // Row pointers of one material / dichroic surface, plus ONE more behind them: the reference's dichroic model reads
    // dichroic_reflect[1] of a one-angle table (photon.h:648: `iidx < nangles - 2` in unsigned arithmetic), a pointer
    // behind its array.  Here that is the table's next row (the last row again at the table's end), weighted by 0.
    float **rows(float *base, size_t first, size_t n, size_t stride, size_t total)
    {
        row_ptrs.emplace_back(n + 1, (float *)0);
        std::vector<float *> &r = row_ptrs.back();
        for (size_t i = 0; i < n; i++) r[i] = base + (first + i) * stride;
        if (total) r[n] = base + (first + n < total ? first + n : total - 1) * stride;
        return r.data();
    }

    explicit World(const chroma_geometry_desc *d)
    {
        const size_t wn = d->wavelength_n, tn = d->time_n;
        tables.reserve(32);
        row_ptrs.reserve(4 * (size_t)d->nmaterials + 2 * (size_t)d->ndichroic + 8);

        float *refr = table(d->mat_refractive_index, d->nmaterials * wn);
        float *absl = table(d->mat_absorption_length, d->nmaterials * wn);
        float *scat = table(d->mat_scattering_length, d->nmaterials * wn);
        float *c_prob = table(d->comp_reemission_prob, d->ncomp_total * wn);
        float *c_wvl = table(d->comp_reemission_wvl_cdf, d->ncomp_total * wn);
        float *c_abs = table(d->comp_absorption_length, d->ncomp_total * wn);
        float *c_time = table(d->comp_reemission_time_cdf, d->ncomp_total * tn);
        materials.resize(d->nmaterials);
        for (uint32_t m = 0; m < d->nmaterials; m++) {
            Material &M = materials[m];
            memset(&M, 0, sizeof M);
            M.refractive_index = refr + m * wn;
            M.absorption_length = absl + m * wn;
            M.scattering_length = scat + m * wn;
            M.num_comp = d->mat_num_comp ? d->mat_num_comp[m] : 0;
            size_t first = (d->mat_comp_offset && M.num_comp) ? d->mat_comp_offset[m] : 0;
            M.comp_reemission_prob = rows(c_prob, first, M.num_comp, wn, d->ncomp_total);
            M.comp_reemission_wvl_cdf = rows(c_wvl, first, M.num_comp, wn, d->ncomp_total);
            M.comp_absorption_length = rows(c_abs, first, M.num_comp, wn, d->ncomp_total);
            M.comp_reemission_time_cdf = rows(c_time, first, M.num_comp, tn, d->ncomp_total);
            M.wavelength_n = d->wavelength_n; M.wavelength_step = d->wavelength_step; M.wavelength_start = d->wavelength_start;
            M.time_n = d->time_n; M.time_step = d->time_step; M.time_start = d->time_start;
        }
        for (uint32_t m = 0; m < d->nmaterials; m++) material_ptrs.push_back(&materials[m]);

        float *d_angles = table(d->dichroic_angles, d->ndichroic_angles_total);
        float *d_refl = table(d->dichroic_reflect, d->ndichroic_angles_total * wn);
        float *d_tran = table(d->dichroic_transmit, d->ndichroic_angles_total * wn);
        dichroics.resize(d->ndichroic);
        for (uint32_t k = 0; k < d->ndichroic; k++) {
            DichroicProps &D = dichroics[k];
            D.nangles = d->dichroic_nangles[k];
            D.angles = d_angles + d->dichroic_offset[k];
            D.dichroic_reflect = rows(d_refl, d->dichroic_offset[k], D.nangles, wn, d->ndichroic_angles_total);
            D.dichroic_transmit = rows(d_tran, d->dichroic_offset[k], D.nangles, wn, d->ndichroic_angles_total);
        }

        float *s_detect = table(d->surf_detect, d->nsurfaces * wn);
        float *s_absorb = table(d->surf_absorb, d->nsurfaces * wn);
        float *s_reemit = table(d->surf_reemit, d->nsurfaces * wn);
        float *s_diffuse = table(d->surf_reflect_diffuse, d->nsurfaces * wn);
        float *s_specular = table(d->surf_reflect_specular, d->nsurfaces * wn);
        float *s_eta = table(d->surf_eta, d->nsurfaces * wn);
        float *s_k = table(d->surf_k, d->nsurfaces * wn);
        float *s_cdf = table(d->surf_reemission_cdf, d->nsurfaces * wn);
        surfaces.resize(d->nsurfaces);
        for (uint32_t s = 0; s < d->nsurfaces; s++) {
            Surface &S = surfaces[s];
            memset(&S, 0, sizeof S);
            S.detect = s_detect + s * wn; S.absorb = s_absorb + s * wn; S.reemit = s_reemit + s * wn;
            S.reflect_diffuse = s_diffuse + s * wn; S.reflect_specular = s_specular + s * wn;
            S.eta = s_eta + s * wn; S.k = s_k + s * wn; S.reemission_cdf = s_cdf + s * wn;
            int di = d->surf_dichroic_index ? d->surf_dichroic_index[s] : -1;
            S.dichroic_props = (di >= 0 && (uint32_t)di < d->ndichroic) ? &dichroics[di] : (DichroicProps *)0;
            S.model = d->surf_model[s];
            S.wavelength_n = d->wavelength_n; S.wavelength_step = d->wavelength_step; S.wavelength_start = d->wavelength_start;
            S.transmissive = d->surf_transmissive[s];
            S.thickness = d->surf_thickness[s];
        }
        for (uint32_t s = 0; s < d->nsurfaces; s++) surface_ptrs.push_back(&surfaces[s]);

        memset(&g, 0, sizeof g);
        g.vertices = (float3 *)d->vertices;
        g.triangles = (uint3 *)d->triangles;
        g.material_codes = (unsigned int *)d->material_codes;
        g.colors = (unsigned int *)d->colors;
        g.primary_nodes = (uint4 *)d->nodes;
        g.extra_nodes = (uint4 *)0;
        g.materials = material_ptrs.data();
        g.surfaces = surface_ptrs.data();
        g.world_origin = make_float3(d->world_origin[0], d->world_origin[1], d->world_origin[2]);
        g.world_scale = d->world_scale;
        g.nprimary_nodes = (int)d->nnodes;
    }
};

void set_launch(unsigned int nblocks, unsigned int nthreads_per_block)
{
    gridDim.x = nblocks; gridDim.y = gridDim.z = 1;
    blockDim.x = nthreads_per_block; blockDim.y = blockDim.z = 1;
}

}  // namespace

extern "C" {

const char *ref_phys_variant(void)
{
#ifdef REF_PHYS_CONTRACT
    return "contract";
#else
    return "libm";
#endif
}

// GPUPhotons.propagate (chroma/gpu/photon.py:225-252, without `track`) around the reference's kernel: one step per
// launch while the queue holds at least 64 * 16 * 8 photons and weights are off, else all remaining steps in one
// launch; scatter_first only in the first launch; the queue of survivors that propagate.cu:315-318 appends to becomes
// the next input.  The curandState of a thread is its photon's stream at that photon's counter, and is written back.
// (photon.py splits a launch into chunks of 1024 blocks; a thread's result does not depend on which chunk runs it.)
int ref_phys_propagate(const chroma_geometry_desc *desc, const chroma_photon_arrays *a, uint64_t nphotons_total,
                       chroma_rng rng, int32_t max_steps, int32_t use_weights, int32_t scatter_first, uint64_t *launches_out)
{
    const unsigned int nthreads_per_block = 64;
    uint64_t launches = 0;
    if (launches_out) *launches_out = 0;
    if (nphotons_total == 0) return 0;
    if (nphotons_total >= 0x7fffffffull) return -1;
    World w(desc);
    std::vector<unsigned int> queue_a(nphotons_total + 1), queue_b(nphotons_total + 1, 0u);
    unsigned int *input_queue = queue_a.data(), *output_queue = queue_b.data();
    input_queue[0] = 0;
    for (uint64_t i = 0; i < nphotons_total; i++) input_queue[1 + i] = (unsigned int)i;
    output_queue[0] = 1;
    std::vector<curandState> states(nphotons_total);

    unsigned int nphotons = (unsigned int)nphotons_total;
    int step = 0;
    while (step < max_steps) {
        int nsteps = (nphotons < nthreads_per_block * 16 * 8 || use_weights) ? (max_steps - step) : 1;
        for (unsigned int id = 0; id < nphotons; id++) {
            unsigned int photon_id = input_queue[1 + id];
            curand_init(rng.seed, rng.photon_id_base + photon_id, a->rng_counters[photon_id], &states[id]);
        }
        unsigned int nblocks = (nphotons + nthreads_per_block - 1) / nthreads_per_block;
        set_launch(nblocks, nthreads_per_block);
        for (unsigned int b = 0; b < nblocks; b++)
            for (unsigned int t = 0; t < nthreads_per_block; t++) {
                blockIdx.x = b; threadIdx.x = t;
                propagate(0, (int)nphotons, input_queue + 1, output_queue, states.data(),
                          (float3 *)a->pos, (float3 *)a->dir, a->wavelengths, (float3 *)a->pol, a->t, a->flags,
                          a->last_hit_triangles, a->weights, a->evidx, nsteps, use_weights, scatter_first, &w.g);
            }
        launches++;
        for (unsigned int id = 0; id < nphotons; id++) a->rng_counters[input_queue[1 + id]] = states[id].counter;

        step += nsteps;
        scatter_first = 0;
        if (step < max_steps) {
            unsigned int *tmp = input_queue; input_queue = output_queue; output_queue = tmp;
            output_queue[0] = 1;
            nphotons = input_queue[0] - 1;
            if (nphotons == 0) break;
        }
    }
    if (launches_out) *launches_out = launches;
    return 0;
}

// ONE call of one of the reference's six routines on photon 0 of `a` with an explicit State: the argument list and
// the numbering of oracle_single (oracle/chroma_oracle.c).  which: 0 rayleigh_scatter, 1 propagate_at_boundary,
// 2 propagate_at_specular_reflector, 3 propagate_at_diffuse_reflector, 4 propagate_at_surface, 5 propagate_to_boundary.
int ref_phys_single(const chroma_geometry_desc *desc, const chroma_photon_arrays *a, chroma_rng rng_desc, int which,
                    const float normal[3], float n1, float n2, float absorption_length, float scattering_length,
                    int material1, int surface_index, float distance_to_boundary, int use_weights, int scatter_first)
{
    World w(desc);
    Photon p;
    p.position = make_float3(a->pos[0], a->pos[1], a->pos[2]);
    p.direction = make_float3(a->dir[0], a->dir[1], a->dir[2]);
    p.polarization = make_float3(a->pol[0], a->pol[1], a->pol[2]);
    p.wavelength = a->wavelengths[0]; p.time = a->t[0]; p.last_hit_triangle = a->last_hit_triangles[0];
    p.history = a->flags[0]; p.weight = a->weights[0]; p.evidx = a->evidx[0];
    State s;
    memset(&s, 0, sizeof s);
    s.surface_normal = make_float3(normal[0], normal[1], normal[2]);
    s.refractive_index1 = n1; s.refractive_index2 = n2;
    s.absorption_length = absorption_length; s.scattering_length = scattering_length;
    s.material1 = (material1 >= 0 && (uint32_t)material1 < desc->nmaterials) ? w.g.materials[material1] : (Material *)0;
    s.surface_index = surface_index; s.distance_to_boundary = distance_to_boundary;
    curandState rng;
    curand_init(rng_desc.seed, rng_desc.photon_id_base, a->rng_counters[0], &rng);
    int command = -1;
    switch (which) {
    case 0: rayleigh_scatter(p, rng); break;
    case 1: propagate_at_boundary(p, s, rng); break;
    case 2: command = propagate_at_specular_reflector(p, s); break;
    case 3: command = propagate_at_diffuse_reflector(p, s, rng); break;
    case 4:
        if (surface_index < 0 || (uint32_t)surface_index >= desc->nsurfaces) return -101;
        command = propagate_at_surface(p, s, rng, &w.g, use_weights != 0);
        break;
    case 5:
        if (!s.material1) return -101;
        command = propagate_to_boundary(p, s, rng, use_weights != 0, scatter_first);
        break;
    default: return -100;
    }
    a->rng_counters[0] = rng.counter;
    a->pos[0] = p.position.x; a->pos[1] = p.position.y; a->pos[2] = p.position.z;
    a->dir[0] = p.direction.x; a->dir[1] = p.direction.y; a->dir[2] = p.direction.z;
    a->pol[0] = p.polarization.x; a->pol[1] = p.polarization.y; a->pol[2] = p.polarization.z;
    a->wavelengths[0] = p.wavelength; a->t[0] = p.time; a->flags[0] = p.history;
    a->last_hit_triangles[0] = p.last_hit_triangle; a->weights[0] = p.weight;
    return command;
}

static Detector make_detector(const chroma_geometry_desc *desc, const chroma_daq_tables *tab)
{
    Detector det;
    memset(&det, 0, sizeof det);
    det.solid_id_to_channel_index = (int *)desc->solid_id_to_channel_index;
    det.time_cdf_x = (float *)tab->d_time_cdf_x; det.time_cdf_y = (float *)tab->d_time_cdf_y;
    det.charge_cdf_x = (float *)tab->d_charge_cdf_x; det.charge_cdf_y = (float *)tab->d_charge_cdf_y;
    det.nchannels = (int)desc->nchannels;
    det.time_cdf_len = tab->time_cdf_len; det.charge_cdf_len = tab->charge_cdf_len;
    det.charge_unit = tab->charge_unit;
    return det;
}

// run_daq (daq.cu:35-86), argument list of oracle_run_daq: thread `id` holds the DAQ stream (stream word
// 1 + acquisition) of photon first_photon + id at counter 0.
int ref_phys_run_daq(const chroma_geometry_desc *desc, const chroma_daq_tables *tab, int32_t first_photon, int32_t nphotons,
                     uint32_t detection_state, const chroma_photon_arrays *a, chroma_rng rng_desc, uint32_t acquisition,
                     float global_weight, uint32_t *earliest_time_int, uint32_t *channel_q_int, uint32_t *channel_histories)
{
    if (nphotons <= 0) return 0;
    const unsigned int nthreads_per_block = 64;
    Detector det = make_detector(desc, tab);
    std::vector<curandState> states((size_t)nphotons);
    for (int id = 0; id < nphotons; id++) {
        curand_init(rng_desc.seed, rng_desc.photon_id_base + (uint64_t)(first_photon + id), 0, &states[id]);
        states[id].stream = 1u + acquisition;
    }
    unsigned int nblocks = ((unsigned int)nphotons + nthreads_per_block - 1) / nthreads_per_block;
    set_launch(nblocks, nthreads_per_block);
    for (unsigned int b = 0; b < nblocks; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            blockIdx.x = b; threadIdx.x = t;
            run_daq(states.data(), detection_state, first_photon, nphotons, a->t, a->flags, a->last_hit_triangles,
                    a->weights, (int *)desc->solid_id_map, &det, earliest_time_int, channel_q_int, channel_histories,
                    global_weight);
        }
    return 0;
}

// run_daq_many (daq.cu:88-150), argument list of oracle_run_daq_many: one block per photon and blockDim.x = ndaq, so
// that thread i of a block serves copy i alone; its state is the photon's DAQ stream at counter 8 i.
int ref_phys_run_daq_many(const chroma_geometry_desc *desc, const chroma_daq_tables *tab, int32_t first_photon, int32_t nphotons,
                          uint32_t detection_state, const chroma_photon_arrays *a, chroma_rng rng_desc, uint32_t acquisition,
                          float global_weight, int32_t ndaq, int32_t channel_stride,
                          uint32_t *earliest_time_int, uint32_t *channel_q_int, uint32_t *channel_histories)
{
    if (nphotons <= 0 || ndaq <= 0) return 0;
    Detector det = make_detector(desc, tab);
    const unsigned int nthreads_per_block = (unsigned int)ndaq;
    std::vector<curandState> states((size_t)nphotons * nthreads_per_block);
    for (int b = 0; b < nphotons; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            curandState &s = states[(size_t)b * nthreads_per_block + t];
            curand_init(rng_desc.seed, rng_desc.photon_id_base + (uint64_t)(first_photon + b), 8u * t, &s);
            s.stream = 1u + acquisition;
        }
    set_launch((unsigned int)nphotons, nthreads_per_block);
    for (unsigned int b = 0; b < (unsigned int)nphotons; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            blockIdx.x = b; threadIdx.x = t;
            run_daq_many(states.data(), detection_state, first_photon, nphotons, a->t, a->flags, a->last_hit_triangles,
                         a->weights, (int *)desc->solid_id_map, &det, earliest_time_int, channel_q_int, channel_histories,
                         ndaq, channel_stride, global_weight);
        }
    return 0;
}

}  // extern "C"

// ---- the hybrid render (hybrid_render.cu) ----------------------------------------------------------------------------
namespace {

// Where and what the running thread of update_xyz_lookup adds: the atomicExch stand-in (ref_shim/cuda_host_shim.h, the
// project's own text) reports every exchange of a non-zero value, which in fAtomicAdd is `data + what the entry held`.
// The record pass below runs a thread against tables that hold zeros, so the value noted is 0 + data = data, exactly.
struct ExchNote {
    float *table[2];            // [0] xyz_lookup1, [1] xyz_lookup2 of the record pass
    size_t nfloats;
    int which, triangle;        // of the running thread: table (-1: none yet), row
    float value[3];
    bool confused;              // an exchange outside the tables, or a second row
} exch_note;

void note_exchange(float *p, float v)
{
    for (int w = 0; w < 2; w++) {
        if (p < exch_note.table[w] || p >= exch_note.table[w] + exch_note.nfloats) continue;
        size_t at = (size_t)(p - exch_note.table[w]);
        int tri = (int)(at / 3);
        if (exch_note.which == -1) { exch_note.which = w; exch_note.triangle = tri; }
        if (exch_note.which != w || exch_note.triangle != tri) exch_note.confused = true;
        exch_note.value[at % 3] = v;
        return;
    }
    exch_note.confused = true;
}

}  // namespace

extern "C" {

// ONE update_xyz_lookup launch (hybrid_render.cu:63-131) over `nthreads` threads, 64 to a block, onto xyz_lookup1 / 2
// ([ntriangles][3] each).  Thread k holds the stream rng.photon_id_base + k at counters[k]; the counter is written back.
//
// rec_triangle / rec_side / rec_value (each may be null, all or none): thread k's OWN addition -- the row, the table
// (1: xyz_lookup1, the inside_to_outside one; 0: xyz_lookup2) and the three values handed to fAtomicAdd -- or triangle -1
// where it added nothing.  They come from a record pass BEFORE the launch: every thread once more, from a copy of its
// state, onto scratch tables of zeros, the exchange stand-in noting what was put there.  (A component whose value is
// +-0 makes no exchange, hybrid_render.cu:15, and stays 0.0f in the record.)
int ref_hybrid_lookup(const chroma_geometry_desc *desc, int32_t nthreads, int32_t total_threads, int32_t offset, const float *position,
                      chroma_rng rng, uint32_t *counters, float wavelength, const float *xyz, float *xyz_lookup1, float *xyz_lookup2,
                      int32_t max_steps, int32_t *rec_triangle, uint32_t *rec_side, float *rec_value)
{
    if (nthreads <= 0) return 0;
    // the kernel fetches triangle offset + k of every thread below total_threads and checks nothing else (the camera
    // passes the triangle count, chroma/camera.py:213-217): a launch that would read past the mesh is not made
    if (offset < 0 || total_threads < 0 || (uint32_t)total_threads > desc->ntriangles) return -3;
    const unsigned int nthreads_per_block = 64;
    World w(desc);
    const float3 pos = make_float3(position[0], position[1], position[2]);
    const float3 colour = make_float3(xyz[0], xyz[1], xyz[2]);
    std::vector<curandState> states((size_t)nthreads);
    unsigned int nblocks = ((unsigned int)nthreads + nthreads_per_block - 1) / nthreads_per_block;
    set_launch(nblocks, nthreads_per_block);

    if (rec_triangle) {
        if (!rec_side || !rec_value) return -1;
        std::vector<float> scratch1((size_t)desc->ntriangles * 3, 0.0f), scratch2((size_t)desc->ntriangles * 3, 0.0f);
        exch_note.table[0] = scratch1.data(); exch_note.table[1] = scratch2.data();
        exch_note.nfloats = scratch1.size();
        exch_note.confused = false;
        for (int k = 0; k < nthreads; k++) curand_init(rng.seed, rng.photon_id_base + (uint64_t)k, counters[k], &states[k]);
        ref_shim_exch_note = note_exchange;
        for (int k = 0; k < nthreads; k++) {
            exch_note.which = -1; exch_note.triangle = -1;
            exch_note.value[0] = exch_note.value[1] = exch_note.value[2] = 0.0f;
            blockIdx.x = (unsigned int)k / nthreads_per_block; threadIdx.x = (unsigned int)k % nthreads_per_block;
            update_xyz_lookup(nthreads, total_threads, offset, pos, states.data(), wavelength, colour,
                              (float3 *)scratch1.data(), (float3 *)scratch2.data(), max_steps, &w.g);
            rec_triangle[k] = exch_note.triangle;
            rec_side[k] = exch_note.which == 0 ? 1u : 0u;
            for (int c = 0; c < 3; c++) rec_value[3 * k + c] = exch_note.value[c];
            if (exch_note.which >= 0) {
                float *row = exch_note.table[exch_note.which] + 3 * (size_t)exch_note.triangle;
                row[0] = row[1] = row[2] = 0.0f;
            }
        }
        ref_shim_exch_note = 0;
        if (exch_note.confused) return -2;
    }

    for (int k = 0; k < nthreads; k++) curand_init(rng.seed, rng.photon_id_base + (uint64_t)k, counters[k], &states[k]);
    for (unsigned int b = 0; b < nblocks; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            blockIdx.x = b; threadIdx.x = t;
            update_xyz_lookup(nthreads, total_threads, offset, pos, states.data(), wavelength, colour,
                              (float3 *)xyz_lookup1, (float3 *)xyz_lookup2, max_steps, &w.g);
        }
    for (int k = 0; k < nthreads; k++) counters[k] = states[k].counter;
    return 0;
}

// ONE update_xyz_image launch (hybrid_render.cu:133-168) over `nthreads` rays, 64 to a block; streams as above.
int ref_hybrid_image(const chroma_geometry_desc *desc, int32_t nthreads, chroma_rng rng, uint32_t *counters, const float *positions,
                     const float *directions, float wavelength, const float *xyz, const float *xyz_lookup1, const float *xyz_lookup2,
                     float *image, int32_t nlookup_calls, int32_t max_steps)
{
    if (nthreads <= 0) return 0;
    const unsigned int nthreads_per_block = 64;
    World w(desc);
    std::vector<curandState> states((size_t)nthreads);
    for (int k = 0; k < nthreads; k++) curand_init(rng.seed, rng.photon_id_base + (uint64_t)k, counters[k], &states[k]);
    unsigned int nblocks = ((unsigned int)nthreads + nthreads_per_block - 1) / nthreads_per_block;
    set_launch(nblocks, nthreads_per_block);
    for (unsigned int b = 0; b < nblocks; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            blockIdx.x = b; threadIdx.x = t;
            update_xyz_image(nthreads, states.data(), (float3 *)positions, (float3 *)directions, wavelength,
                             make_float3(xyz[0], xyz[1], xyz[2]), (float3 *)xyz_lookup1, (float3 *)xyz_lookup2, (float3 *)image,
                             nlookup_calls, max_steps, &w.g);
        }
    for (int k = 0; k < nthreads; k++) counters[k] = states[k].counter;
    return 0;
}

// process_image (hybrid_render.cu:170-200) over `nthreads` pixels, 64 to a block.  The caller keeps NaN out of `image`:
// the kernel converts floorf(NaN) to unsigned, which a host build leaves undefined.
int ref_hybrid_pixels(int32_t nthreads, const float *image, uint32_t *pixels, int32_t nimages)
{
    if (nthreads <= 0) return 0;
    const unsigned int nthreads_per_block = 64;
    unsigned int nblocks = ((unsigned int)nthreads + nthreads_per_block - 1) / nthreads_per_block;
    set_launch(nblocks, nthreads_per_block);
    for (unsigned int b = 0; b < nblocks; b++)
        for (unsigned int t = 0; t < nthreads_per_block; t++) {
            blockIdx.x = b; threadIdx.x = t;
            process_image(nthreads, (float3 *)image, pixels, nimages);
        }
    return 0;
}

}  // extern "C"
