// geometry.hip -- chroma_geometry_create and its companions: the checks of a geometry description, its upload, the arrays
// derived from it on the device (kernels_geometry.h).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>

#include "chroma_internal.h"
#include "propagate_device.h"
#include "wide_build.h"
#include "host_utils.h"

#include "kernels_geometry.h"

template <class T>
static int upload(chroma_geometry *g, const T *host, size_t count, const T **dev_out)
{
    *dev_out = nullptr;
    size_t bytes = std::max(count, (size_t)1) * sizeof(T);
    void *d = nullptr;
    HIP_TRY(ctx_malloc(g->ctx, &d, bytes));
    g->allocations.push_back(d);
    g->device_bytes += bytes;
    if (count && host) HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(d, 0, bytes));
    *dev_out = (const T *)d;
    return CHROMA_OK;
}

// runs `pass` until an entry no longer changes; returns need[0]
template <class Pass>
static int stack_need_fixed_point(chroma_ctx *ctx, size_t n, Pass pass, uint32_t *result)
{
    uint32_t *d_need = nullptr, *d_changed = nullptr;
    HIP_TRY(ctx_malloc(ctx, (void **)&d_need, std::max<size_t>(n, 1) * 4));
    if (hipMalloc(&d_changed, 4) != hipSuccess) { hipFree(d_need); return set_error(CHROMA_ERR_INTERNAL, "out of device memory"); }
    hipError_t e = hipMemsetAsync(d_need, 0, std::max<size_t>(n, 1) * 4, ctx->stream);
    uint32_t changed = 1, h_need = 0;
    for (int it = 0; e == hipSuccess && changed && it < 8192; it++) {
        e = hipMemsetAsync(d_changed, 0, 4, ctx->stream);
        for (int k = 0; k < 4; k++) pass(d_need, d_changed);                    // (four passes per question)
        if (e == hipSuccess) e = hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(&h_need, d_need, 4, hipMemcpyDeviceToHost);
    hipFree(d_need); hipFree(d_changed);
    if (e != hipSuccess) return set_error((int)e, "stack need: %s", hipGetErrorString(e));
    if (changed) return set_error(CHROMA_ERR_INVALID, "stack need: the tree does not settle (a child range that points back?)");
    *result = h_need;
    return CHROMA_OK;
}

extern "C" {

// ---- geometry -------------------------------------------------------------------------------------
int chroma_geometry_create(chroma_ctx *ctx, const chroma_geometry_desc *d, chroma_geometry **out)
{
    if (!ctx || !d || !out) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!d->vertices || !d->triangles || !d->material_codes || !d->nodes || d->nnodes == 0 || d->ntriangles == 0)
        return set_error(CHROMA_ERR_INVALID, "geometry: missing mesh or BVH arrays");
    if (d->wavelength_n < 2 || d->nmaterials == 0 || d->nmaterials > 127 || d->nsurfaces > 127)
        return set_error(CHROMA_ERR_INVALID, "geometry: bad optics table sizes (8-bit signed material/surface indices)");
    if (!d->mat_refractive_index || !d->mat_absorption_length || !d->mat_scattering_length || !d->mat_num_comp || !d->mat_comp_offset)
        return set_error(CHROMA_ERR_INVALID, "geometry: missing material tables");
    // host-side shape checks the kernels rely on (all cores; the first offender in index order is reported)
    {
        using chroma_host::parallel_for;
        std::atomic<size_t> bad_tri(SIZE_MAX), bad_node(SIZE_MAX), bad_code(SIZE_MAX);
        auto note = [](std::atomic<size_t> &slot, size_t i) { size_t cur = slot.load(); while (i < cur && !slot.compare_exchange_weak(cur, i)) {} };
        parallel_for((size_t)d->ntriangles * 3, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) if (d->triangles[i] >= d->nvertices) { note(bad_tri, i); break; }
        });
        if (bad_tri != SIZE_MAX) { size_t i = bad_tri; return set_error(CHROMA_ERR_INVALID, "triangle %zu references vertex %u >= %u", i / 3, d->triangles[i], d->nvertices); }
        parallel_for((size_t)d->nnodes, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                uint32_t w = d->nodes[4 * i + 3];
                uint32_t nchild = w >> CHROMA_CHILD_BITS, child = w & ~CHROMA_NCHILD_MASK;
                bool bad = nchild == 0 ? child >= d->ntriangles : ((size_t)child + nchild > d->nnodes || child <= i);
                if (bad) { note(bad_node, i); break; }
            }
        });
        if (bad_node != SIZE_MAX) {
            size_t i = bad_node;
            uint32_t w = d->nodes[4 * i + 3], nchild = w >> CHROMA_CHILD_BITS, child = w & ~CHROMA_NCHILD_MASK;
            if (nchild == 0) return set_error(CHROMA_ERR_INVALID, "leaf node %zu references triangle %u >= %u", i, child, d->ntriangles);
            return set_error(CHROMA_ERR_INVALID, "node %zu has a bad child range [%u, %u)", i, child, child + nchild);
        }
        parallel_for((size_t)d->ntriangles, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                uint32_t code = d->material_codes[i];
                int inner = (int8_t)(code >> 24), outer = (int8_t)(code >> 16), surf = (int8_t)(code >> 8);
                bool bad = inner < 0 || outer < 0 || inner >= (int)d->nmaterials || outer >= (int)d->nmaterials || surf < -1 || surf >= (int)d->nsurfaces;
                if (!bad && d->nsolids && d->solid_id_map && d->solid_id_map[i] >= d->nsolids) bad = true;
                if (bad) { note(bad_code, i); break; }
            }
        });
        if (bad_code != SIZE_MAX) {
            size_t i = bad_code;
            uint32_t code = d->material_codes[i];
            int inner = (int8_t)(code >> 24), outer = (int8_t)(code >> 16), surf = (int8_t)(code >> 8);
            if (inner < 0 || outer < 0 || inner >= (int)d->nmaterials || outer >= (int)d->nmaterials || surf < -1 || surf >= (int)d->nsurfaces)
                return set_error(CHROMA_ERR_INVALID, "triangle %zu has material code 0x%08x outside the tables", i, code);
            return set_error(CHROMA_ERR_INVALID, "triangle %zu has solid id %u >= %u", i, d->solid_id_map[i], d->nsolids);
        }
    }
    for (uint32_t m = 0; m < d->nmaterials; m++)
        if (d->mat_num_comp[m] && d->mat_comp_offset[m] + d->mat_num_comp[m] > d->ncomp_total)
            return set_error(CHROMA_ERR_INVALID, "material %u: component rows out of range", m);
    for (uint32_t s = 0; s < d->nsurfaces; s++) {
        if (d->surf_model[s] == CHROMA_SURFACE_DICHROIC) {
            int di = d->surf_dichroic_index ? d->surf_dichroic_index[s] : -1;
            if (di < 0 || di >= (int)d->ndichroic || d->dichroic_nangles[di] < 2 ||
                d->dichroic_offset[di] + d->dichroic_nangles[di] > d->ndichroic_angles_total)
                return set_error(CHROMA_ERR_INVALID, "surface %u: dichroic tables missing or out of range", s);
        }
    }

    const bool timing = getenv("CHROMA_TIMING") != nullptr;
    auto t_phase = std::chrono::steady_clock::now();
    auto phase = [&](const char *what) {
        if (!timing) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[chroma_geometry_create] %-28s %.2f s\n", what, std::chrono::duration<double>(now - t_phase).count());
        t_phase = now;
    };
    phase("validation");
    HIP_TRY(hipSetDevice(ctx->device));
    chroma_geometry *g = new chroma_geometry;
    g->ctx = ctx;
    g->nvertices = d->nvertices; g->ntriangles = d->ntriangles; g->nnodes = d->nnodes;
    GeoView &v = g->view;
    memset(&v, 0, sizeof v);
    int rc;
#define UP(field, src, count) if ((rc = upload(g, src, (size_t)(count), &v.field)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; }
    // nodes as passed in (what GPUGeometry.nodes shows)
    { const uint4 *p; if ((rc = upload(g, (const uint4 *)d->nodes, d->nnodes, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } g->d_nodes_api = (void *)p; }
    // derived 8-wide tree, device triangle order and reference test ranks (csrc/wide_build.cpp)
    chroma_host::WideTree wt;
    const bool wide_given = d->wide_nodes != nullptr;
    if (wide_given) {
        if (!d->wide_tri_to_record || !d->wide_record_to_tri || !d->wide_rank || d->nwide == 0 || d->nrecords == 0) {
            chroma_geometry_destroy(g);
            return set_error(CHROMA_ERR_INVALID, "geometry: a supplied wide tree needs its nodes, both record maps and the ranks");
        }
    } else {
        // the default topology is built where the reference builds its tree: on the device (csrc/wide_device.hip);
        // the others, and CHROMA_WIDE_BUILD=host, on the host cores (csrc/wide_build.cpp) -- "levels" gives the same tree either way
        std::string werr;
        const int topology = chroma_host::wide_topology_from_env();
        const char *where = getenv("CHROMA_WIDE_BUILD");
        if (topology == chroma_host::WIDE_TOPOLOGY_LEVELS && !(where && !strcmp(where, "host"))) {
            void *h = nullptr;
            rc = chroma_wide_build_device(ctx, d->nodes, d->nnodes, d->ntriangles, &h, nullptr, nullptr, nullptr);
            if (rc == (int)hipErrorOutOfMemory) {
                // (the builder's scratch -- ~150 bytes per triangle -- did not fit beside what the caller keeps on the card:
                //  give the pool's parked blocks back and try once more; then the host cores build the SAME tree)
                (void)hipGetLastError();
                chroma_pool_trim(ctx);
                rc = chroma_wide_build_device(ctx, d->nodes, d->nnodes, d->ntriangles, &h, nullptr, nullptr, nullptr);
            }
            if (rc == (int)hipErrorOutOfMemory) {
                (void)hipGetLastError();
                fprintf(stderr, "chroma_geometry_create: no room on the device for the tree builder's scratch: building the same tree on the host cores\n");
                if (chroma_host::build_wide_tree(d->nodes, d->nnodes, d->ntriangles, wt, werr, topology) != 0) {
                    chroma_geometry_destroy(g);
                    return set_error(CHROMA_ERR_INVALID, "%s", werr.c_str());
                }
            } else if (rc != CHROMA_OK) { chroma_geometry_destroy(g); return rc; }
            else {
                wt = std::move(*(chroma_host::WideTree *)h);
                delete (chroma_host::WideTree *)h;
            }
        } else if (chroma_host::build_wide_tree(d->nodes, d->nnodes, d->ntriangles, wt, werr, topology) != 0) {
            chroma_geometry_destroy(g);
            return set_error(CHROMA_ERR_INVALID, "%s", werr.c_str());
        }
    }
    phase(wide_given ? "nodes upload" : "nodes upload + wide tree");
    const uint32_t *wide_nodes = wide_given ? d->wide_nodes : wt.wnodes.data();
    const uint32_t *tri_to_dev = wide_given ? d->wide_tri_to_record : wt.tri_to_dev.data();
    const uint32_t *dev_to_tri = wide_given ? d->wide_record_to_tri : wt.dev_to_tri.data();
    const uint32_t *tri_rank = wide_given ? d->wide_rank : wt.rank.data();
    const size_t nwide = wide_given ? (size_t)d->nwide : wt.nwide;
    const size_t nrecords = wide_given ? (size_t)d->nrecords : wt.dev_to_tri.size();
    {   // the walks index the wide nodes and the records with what this tree holds: check it before any upload
        std::string werr;
        if (chroma_host::validate_wide_tree(wide_nodes, nwide, tri_to_dev, d->ntriangles, dev_to_tri, nrecords, werr) != 0) {
            chroma_geometry_destroy(g);
            return set_error(CHROMA_ERR_INVALID, "%s", werr.c_str());
        }
    }
    phase("wide tree index checks");
    { const uint4 *p; if ((rc = upload(g, (const uint4 *)wide_nodes, nwide * 8, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } v.wnodes = p; }
    v.nwide = (uint32_t)nwide;
    g->nwide = nwide; g->wide_depth = wt.depth; g->nrecords = nrecords;
    {
        const uint4 *dw = v.wnodes;
        const uint32_t nw = (uint32_t)nwide;
        hipStream_t st = ctx->stream;
        if ((rc = stack_need_fixed_point(ctx, nwide, [&](uint32_t *need, uint32_t *changed) {
                 hipLaunchKernelGGL(k_stack_need_wide, dim3((nw + 255) / 256), dim3(256), 0, st, dw, nw, need, changed); }, &g->wide_stack_need)) != CHROMA_OK) {
            chroma_geometry_destroy(g);
            return rc;
        }
    }
    { chroma_host::WordBuffer().swap(wt.wnodes); }
    UP(tri_to_dev, tri_to_dev, d->ntriangles);
    UP(dev_to_tri, dev_to_tri, nrecords);
    // traversal copy of the nodes: leaf child -> device triangle index (a pass over the array uploaded above)
    {
        void *dn = nullptr;
        size_t bytes = (size_t)d->nnodes * 16;
        hipError_t e = ctx_malloc(ctx, &dn, bytes);
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "hipMalloc(%zu) for nodes: %s", bytes, hipGetErrorString(e)); }
        g->allocations.push_back(dn);
        g->device_bytes += bytes;
        hipLaunchKernelGGL(k_traversal_nodes, dim3((unsigned)((d->nnodes + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4 *)g->d_nodes_api, (uint32_t)d->nnodes,
                           v.tri_to_dev, d->ntriangles, (uint4 *)dn);
        v.nodes = (const uint4 *)dn;
    }
    phase("wide nodes + traversal copy");
    // API-visible copies of the mesh arrays (GPUGeometry.vertices/.triangles/.material_codes/.colors)
    { const float *p; if ((rc = upload(g, d->vertices, (size_t)d->nvertices * 3, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } g->d_vertices = (void *)p; }
    { const uint32_t *p; if ((rc = upload(g, d->triangles, (size_t)d->ntriangles * 3, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } g->d_triangles = (void *)p; }
    { const uint32_t *p; if ((rc = upload(g, d->material_codes, d->ntriangles, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } g->d_material_codes = (void *)p; }
    memcpy(v.world_origin, d->world_origin, sizeof v.world_origin);   // (the leaf boxes of the physics records need them)
    v.world_scale = d->world_scale;
    // 48-byte triangle records in device order: gathered on the device from those arrays (+ the ranks, uploaded for this only)
    {
        void *dtri = nullptr;
        size_t bytes = nrecords * (16 * TRI_STRIDE);
        hipError_t e = ctx_malloc(ctx, &dtri, bytes);
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "hipMalloc(%zu) for triangle records: %s", bytes, hipGetErrorString(e)); }
        g->allocations.push_back(dtri);
        g->device_bytes += bytes;
        uint32_t *d_rank = nullptr;
        e = ctx_malloc(ctx, (void **)&d_rank, std::max<size_t>(d->ntriangles, 1) * 4);
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "hipMalloc for triangle ranks: %s", hipGetErrorString(e)); }
        rc = chroma_memcpy_htod(ctx, d_rank, tri_rank, (size_t)d->ntriangles * 4);
        if (rc == CHROMA_OK) {
            hipLaunchKernelGGL(k_triangle_records, dim3((unsigned)((nrecords + 255) / 256)), dim3(256), 0, ctx->stream, (const float *)g->d_vertices, (const uint32_t *)g->d_triangles,
                               (const uint32_t *)g->d_material_codes, d_rank, v.dev_to_tri, (uint32_t)nrecords, (float4 *)dtri);
            e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) rc = set_error((int)e, "triangle records: %s", hipGetErrorString(e));
        }
        hipFree(d_rank);
        if (rc != CHROMA_OK) { chroma_geometry_destroy(g); return rc; }
        v.tri = (const float4 *)dtri;
    }
    // 32-byte physics records, in the same order: derived from the 48-byte ones (k_physics reads only these)
    {
        void *dphys = nullptr;
        size_t bytes = std::max<size_t>(nrecords, 1) * 32;
        hipError_t e = ctx_malloc(ctx, &dphys, bytes);
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "hipMalloc(%zu) for physics records: %s", bytes, hipGetErrorString(e)); }
        g->allocations.push_back(dphys);
        g->device_bytes += bytes;
        if (nrecords) hipLaunchKernelGGL(k_triangle_phys, dim3((unsigned)((nrecords + 255) / 256)), dim3(256), 0, ctx->stream, v, (uint32_t)nrecords, (uint4 *)dphys);
        e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "physics records: %s", hipGetErrorString(e)); }
        v.tri_phys = (const uint4 *)dphys;
    }
    // 48-byte intersection records, in the same order: the edge form of the fast walks' triangle test
    {
        void *disect = nullptr;
        size_t bytes = std::max<size_t>(nrecords, 1) * 48;
        hipError_t e = ctx_malloc(ctx, &disect, bytes);
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "hipMalloc(%zu) for intersection records: %s", bytes, hipGetErrorString(e)); }
        g->allocations.push_back(disect);
        g->device_bytes += bytes;
        if (nrecords) hipLaunchKernelGGL(k_triangle_isect, dim3((unsigned)((nrecords + 255) / 256)), dim3(256), 0, ctx->stream, v, (uint32_t)nrecords, (float4 *)disect);
        e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { chroma_geometry_destroy(g); return set_error((int)e, "intersection records: %s", hipGetErrorString(e)); }
        v.tri_isect = (const float4 *)disect;
    }
    phase("triangle records");
    { const uint32_t *p; if ((rc = upload(g, d->colors, d->colors ? d->ntriangles : 0, &p)) != CHROMA_OK) { chroma_geometry_destroy(g); return rc; } g->d_colors = (void *)p; }
    UP(solid_id_map, d->solid_id_map, d->solid_id_map ? d->ntriangles : 0);
    size_t wn = d->wavelength_n;
    UP(mat_refractive_index, d->mat_refractive_index, d->nmaterials * wn);
    UP(mat_absorption_length, d->mat_absorption_length, d->nmaterials * wn);
    UP(mat_scattering_length, d->mat_scattering_length, d->nmaterials * wn);
    UP(mat_num_comp, d->mat_num_comp, d->nmaterials);
    UP(mat_comp_offset, d->mat_comp_offset, d->nmaterials);
    UP(comp_reemission_prob, d->comp_reemission_prob, d->ncomp_total * wn);
    UP(comp_reemission_wvl_cdf, d->comp_reemission_wvl_cdf, d->ncomp_total * wn);
    UP(comp_absorption_length, d->comp_absorption_length, d->ncomp_total * wn);
    UP(comp_reemission_time_cdf, d->comp_reemission_time_cdf, (size_t)d->ncomp_total * d->time_n);
    UP(surf_detect, d->surf_detect, d->nsurfaces * wn);
    UP(surf_absorb, d->surf_absorb, d->nsurfaces * wn);
    UP(surf_reemit, d->surf_reemit, d->nsurfaces * wn);
    UP(surf_reflect_diffuse, d->surf_reflect_diffuse, d->nsurfaces * wn);
    UP(surf_reflect_specular, d->surf_reflect_specular, d->nsurfaces * wn);
    UP(surf_eta, d->surf_eta, d->nsurfaces * wn);
    UP(surf_k, d->surf_k, d->nsurfaces * wn);
    UP(surf_reemission_cdf, d->surf_reemission_cdf, d->nsurfaces * wn);
    {
        std::vector<SurfaceInfo> info(std::max<uint32_t>(d->nsurfaces, 1));
        for (uint32_t s = 0; s < d->nsurfaces; s++)
            info[s] = SurfaceInfo{d->surf_model[s], d->surf_transmissive[s], d->surf_thickness[s],
                                  d->surf_dichroic_index ? d->surf_dichroic_index[s] : -1};
        UP(surf_info, info.data(), info.size());
    }
    UP(dichroic_nangles, d->dichroic_nangles, d->ndichroic);
    UP(dichroic_offset, d->dichroic_offset, d->ndichroic);
    UP(dichroic_angles, d->dichroic_angles, d->ndichroic_angles_total);
    UP(dichroic_reflect, d->dichroic_reflect, d->ndichroic_angles_total * wn);
    UP(dichroic_transmit, d->dichroic_transmit, d->ndichroic_angles_total * wn);
    UP(solid_id_to_channel_index, d->solid_id_to_channel_index, d->nsolids);
#undef UP
    {   // ~16 ulp of the largest world coordinate (record_hit_is_regular)
        float maxabs = 0.0f;
        for (int a = 0; a < 3; a++)
            maxabs = std::max(maxabs, std::max(fabsf(d->world_origin[a]), fabsf(d->world_origin[a] + 65535.0f * d->world_scale)));
        v.suspect_margin = 2e-6f * maxabs;
        // growth of the boxes in the fast slab test (ray_growth, propagate_device.h): four times the bound on what the fused
        // evaluation can differ from the reference's, at least a quarter of a quantum, at most the whole quantum of rounds 1-2
        // (CHROMA_SLAB_GROW overrides: A/B runs)
        const double bound = ldexp(1.0, -24) * (10.0 * 65534.0 + 2.0 * (double)maxabs / std::max((double)d->world_scale, 1e-30));
        v.slab_grow = (float)std::min(1.0, std::max(0.25, 4.0 * bound));
        if (const char *e = getenv("CHROMA_SLAB_GROW")) v.slab_grow = (float)std::min(1.0, std::max(0.0625, atof(e)));
    }
    v.wavelength_n = d->wavelength_n; v.wavelength_start = d->wavelength_start; v.wavelength_step = d->wavelength_step;
    v.time_n = d->time_n; v.time_start = d->time_start; v.time_step = d->time_step;
    v.nnodes = d->nnodes; v.ntriangles = d->ntriangles; v.nsolids = d->nsolids; v.nchannels = d->nchannels;
    v.plain_optics = 1u;
    for (uint32_t m = 0; m < d->nmaterials; m++) if (d->mat_num_comp[m]) v.plain_optics = 0u;
    for (uint32_t k = 0; k < d->nsurfaces; k++) if (d->surf_model[k] != CHROMA_SURFACE_DEFAULT) v.plain_optics = 0u;
    if (getenv("CHROMA_FULL_PHYSICS")) v.plain_optics = 0u;          // (A/B: the all-models kernel on a plain geometry)

    phase("mesh arrays + tables");
    {
        const uint4 *dn = (const uint4 *)g->d_nodes_api;
        const uint32_t nn = (uint32_t)d->nnodes;
        hipStream_t st = ctx->stream;
        uint32_t need = 0;
        if ((rc = stack_need_fixed_point(ctx, d->nnodes, [&](uint32_t *nd, uint32_t *changed) {
                 hipLaunchKernelGGL(k_stack_need_ref, dim3((nn + 255) / 256), dim3(256), 0, st, dn, nn, nd, changed); }, &need)) != CHROMA_OK) {
            chroma_geometry_destroy(g);
            return rc;
        }
        g->stack_need = std::max<uint32_t>(1, need);
    }
    phase("stack need");
    if (g->stack_need > STACK_LDS + STACK_SCRATCH) {
        uint32_t need = g->stack_need;
        chroma_geometry_destroy(g);
        return set_error(CHROMA_ERR_STACK, "BVH needs %u traversal stack entries, more than the %d supported", need, STACK_LDS + STACK_SCRATCH);
    }
    *out = g;
    return CHROMA_OK;
}

int chroma_geometry_destroy(chroma_geometry *g)
{
    if (!g) return CHROMA_OK;
    hipSetDevice(g->ctx->device);
    hipStreamSynchronize(g->ctx->stream);
    for (void *p : g->allocations) hipFree(p);
    delete g;
    return CHROMA_OK;
}

int chroma_geometry_device_ptr(chroma_geometry *g, const char *name, void **d_ptr, size_t *nbytes)
{
    if (!g || !name || !d_ptr) return set_error(CHROMA_ERR_INVALID, "bad argument");
    std::string n(name);
    size_t bytes = 0; void *p = nullptr;
    if (n == "nodes") { p = g->d_nodes_api; bytes = g->nnodes * 16; }
    else if (n == "vertices") { p = g->d_vertices; bytes = g->nvertices * 12; }
    else if (n == "triangles") { p = g->d_triangles; bytes = g->ntriangles * 12; }
    else if (n == "material_codes") { p = g->d_material_codes; bytes = g->ntriangles * 4; }
    else if (n == "colors") { p = g->d_colors; bytes = g->ntriangles * 4; }
    else if (n == "solid_id_map") { p = (void *)g->view.solid_id_map; bytes = g->ntriangles * 4; }
    else if (n == "solid_id_to_channel_index") { p = (void *)g->view.solid_id_to_channel_index; bytes = (size_t)g->view.nsolids * 4; }
    else if (n == "triangle_records") { p = (void *)g->view.tri; bytes = g->nrecords * (16 * TRI_STRIDE); }
    else if (n == "triangle_phys") { p = (void *)g->view.tri_phys; bytes = g->nrecords * 32; }
    else if (n == "triangle_isect") { p = (void *)g->view.tri_isect; bytes = g->nrecords * 48; }
    else if (n == "wide_nodes") { p = (void *)g->view.wnodes; bytes = g->nwide * 128; }
    else if (n == "tri_to_dev") { p = (void *)g->view.tri_to_dev; bytes = g->ntriangles * 4; }
    else if (n == "dev_to_tri") { p = (void *)g->view.dev_to_tri; bytes = g->nrecords * 4; }
    else return set_error(CHROMA_ERR_INVALID, "unknown geometry array '%s'", name);
    *d_ptr = p;
    if (nbytes) *nbytes = bytes;
    return CHROMA_OK;
}

int chroma_geometry_stack_need(chroma_geometry *g, uint32_t *entries)
{
    if (!g || !entries) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *entries = g->stack_need;
    return CHROMA_OK;
}

}  // extern "C"
