// kernel_calls.hip -- the entry points that are the checks of their arguments around one kernel launch on the context's
// stream, as the reference's kernels are called from Python: the photon-array and hit calls, the PDFs, chroma_render,
// chroma_color_solids, point transforms, the probe, the bomb generator; and hipCUB's scan and sort for the other units.  (The DAQ is
// daq_calls.hip, the photons from particle steps steps_calls.hip: their pipelines are more than that.)
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "chroma_internal.h"
#include "propagate_device.h"

#include "kernels_photons_hits.h"

#include "kernels_render.h"

#include "kernels_probe_math.h"

#include "kernels_pdf.h"

// The count and copy calls: the hit word cleared, the launch it is given run on it (none for an empty range), the word read back
template <class Launch>
static int counted_launch(const CallScope &scope, bool any, uint32_t *count, Launch &&launch)
{
    uint32_t n = 0;
    int rc = scope.clear_words(W_HIT_COUNT); if (rc) return rc;
    if (any) { launch(scope.state().d_words + W_HIT_COUNT); HIP_TRY(hipGetLastError()); }
    rc = scope.read_word(W_HIT_COUNT, &n);
    if (count) *count = n;
    return rc;
}

extern "C" {

int chroma_photon_duplicate(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads,
                            const chroma_photon_arrays *photons, int32_t copies, int32_t stride)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    int rc = check_photons(photons, false);
    if (rc) return rc;
    if (nthreads <= 0 || copies <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_photon_duplicate, dim3((nthreads + 255) / 256), dim3(256), 0, ctx->stream, to_view(photons),
                       first_photon, nthreads, copies, stride);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_count_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, uint32_t target_flag,
                         const uint32_t *d_flags, uint32_t *count)
{
    if (!ctx || !d_flags || !count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    return counted_launch(scope, nthreads > 0, count, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_count_photons, dim3((unsigned)std::min((nthreads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, d_flags, first_photon,
                           nthreads, target_flag, word);
    });
}

int chroma_copy_photons(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, uint32_t target_flag,
                        const chroma_photon_arrays *src, const chroma_photon_arrays *dst, uint32_t *ncopied)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nthreads > 0, ncopied, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_copy_photons, dim3((unsigned)(((long long)nthreads + 16 * 256 - 1) / (16 * 256))), dim3(256), 0, ctx->stream, to_view(src), to_view(dst),
                           first_photon, nthreads, target_flag, word);
    });
}

int chroma_copy_photon_queue(chroma_ctx *ctx, int32_t first_photon, int32_t nthreads, const uint32_t *d_queue,
                             const chroma_photon_arrays *src, const chroma_photon_arrays *dst)
{
    if (!ctx || !d_queue) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    if (nthreads <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_copy_photon_queue, dim3((nthreads + 255) / 256), dim3(256), 0, ctx->stream, to_view(src), to_view(dst),
                       first_photon, nthreads, d_queue);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_count_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon, int32_t nphotons,
                             uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t *count)
{
    if (!ctx || !geom || !count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(photons, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nphotons > 0, count, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_count_hits, dim3((unsigned)std::min((nphotons + 255) / 256, 4096)), dim3(256), 0, ctx->stream, geom->view, photons->flags,
                           photons->last_hit_triangles, first_photon, nphotons, detection_state, word);
    });
}

int chroma_copy_photon_hits(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon, int32_t nphotons,
                            uint32_t detection_state, const chroma_photon_arrays *src, const chroma_photon_arrays *dst,
                            int32_t *d_channels, uint32_t *ncopied)
{
    if (!ctx || !geom || !d_channels) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(src, false); if (rc) return rc;
    rc = check_photons(dst, false); if (rc) return rc;
    const CallScope scope(ctx);
    return counted_launch(scope, nphotons > 0, ncopied, [&](uint32_t *word) {
        hipLaunchKernelGGL(k_copy_hits, dim3((unsigned)(((long long)nphotons + COPY_ITEMS * 256 - 1) / (COPY_ITEMS * 256))), dim3(256), 0, ctx->stream, geom->view, to_view(src),
                           to_view(dst), d_channels, first_photon, nphotons, detection_state, word);
    });
}

int chroma_channel_hits(chroma_ctx *ctx, chroma_geometry *geom, uint64_t nphotons, uint32_t detection_state,
                        const chroma_photon_arrays *photons, uint32_t *d_hit_count, uint32_t *d_earliest_time_bits)
{
    if (!ctx || !geom || !d_hit_count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_channel_hits, dim3((unsigned)((nphotons + 255) / 256)), dim3(256), 0, ctx->stream, geom->view,
                       photons->flags, photons->last_hit_triangles, photons->t, (uint64_t)nphotons, detection_state,
                       d_hit_count, d_earliest_time_bits);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// ---- PDFs over DAQ output (kernels_pdf.h) ----
static int check_pdf_layout(uint32_t nchannels, int32_t ndaq, uint32_t stride)
{
    if (ndaq < 1 || stride < nchannels)
        return set_error(CHROMA_ERR_INVALID, "ndaq must be positive and the channel stride at least the number of channels");
    return CHROMA_OK;
}

int chroma_pdf_bin_hits(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride, const float *d_channel_q,
                        const float *d_channel_t, int32_t tbins, float tmin, float tmax, int32_t qbins, float qmin, float qmax,
                        uint32_t *d_hitcount, uint32_t *d_pdf)
{
    if (!ctx || !d_channel_q || !d_channel_t || !d_hitcount || !d_pdf) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (tbins < 1 || qbins < 1 || (int64_t)tbins * qbins > INT32_MAX)
        return set_error(CHROMA_ERR_INVALID, "need at least one time and one charge bin (and fewer than 2^31 per channel)");
    if (!(tmin < tmax) || !(qmin < qmax)) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_bin_hits, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, (int)ndaq, stride,
                       d_channel_q, d_channel_t, d_hitcount, (int)tbins, tmin, tmax, (int)qbins, qmin, qmax, d_pdf);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_eval_accumulate(chroma_ctx *ctx, uint32_t nchannels, int32_t ndaq, uint32_t stride, const uint32_t *d_event_hit,
                               const float *d_event_time, const float *d_mc_time, uint32_t nhit, const uint32_t *d_hit_channels,
                               float min_twidth, float tmin, float tmax, int32_t min_bin_content, uint32_t *d_hitcount,
                               uint32_t *d_bincount, float *d_nearest)
{
    if (!ctx || !d_event_hit || !d_event_time || !d_mc_time || !d_hitcount || !d_bincount || (nhit && (!d_hit_channels || !d_nearest)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (min_bin_content < 1 || min_bin_content > 1024) return set_error(CHROMA_ERR_INVALID, "min_bin_content must be in 1 .. 1024");
    if (!(tmin < tmax)) return set_error(CHROMA_ERR_INVALID, "empty or inverted time range");
    if (nhit > nchannels) return set_error(CHROMA_ERR_INVALID, "more hit channels than channels");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_eval_hitcount, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, (int)ndaq, stride,
                       d_event_hit, d_mc_time, tmin, tmax, d_hitcount);
    HIP_TRY(hipGetLastError());
    if (nhit == 0) return CHROMA_OK;          // an event with no hit channel: nothing to sort
    hipLaunchKernelGGL(k_pdf_eval_accumulate, dim3((nhit + PDF_EVAL_WAVES - 1) / PDF_EVAL_WAVES), dim3(64 * PDF_EVAL_WAVES), 0,
                       ctx->stream, nchannels, (int)ndaq, stride, nhit, d_hit_channels, d_event_hit, d_event_time, d_mc_time,
                       0.5f * min_twidth, tmin, tmax, (int)min_bin_content, d_hitcount, d_bincount, d_nearest);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_moments(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride, const float *d_mc_time,
                       const float *d_mc_charge, float tmin, float tmax, float qmin, float qmax, uint32_t *d_mom0, float *d_t_mom1,
                       float *d_t_mom2, float *d_q_mom1, float *d_q_mom2)
{
    if (!ctx || !d_mc_time || !d_mom0 || !d_t_mom1 || !d_t_mom2 || (!time_only && (!d_mc_charge || !d_q_mom1 || !d_q_mom2)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (!(tmin < tmax) || (!time_only && !(qmin < qmax))) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_moments, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, (int)(time_only != 0), nchannels,
                       (int)ndaq, stride, d_mc_time, d_mc_charge, tmin, tmax, qmin, qmax, d_mom0, d_t_mom1, d_t_mom2, d_q_mom1, d_q_mom2);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_pdf_kernel_eval(chroma_ctx *ctx, int32_t time_only, uint32_t nchannels, int32_t ndaq, uint32_t stride,
                           const uint32_t *d_event_hit, const float *d_event_time, const float *d_event_charge, const float *d_mc_time,
                           const float *d_mc_charge, float tmin, float tmax, float qmin, float qmax, const float *d_inv_time_bandwidths,
                           const float *d_inv_charge_bandwidths, uint32_t *d_hitcount, float *d_time_pdf_values,
                           float *d_charge_pdf_values)
{
    if (!ctx || !d_event_hit || !d_event_time || !d_mc_time || !d_inv_time_bandwidths || !d_hitcount || !d_time_pdf_values ||
        (!time_only && (!d_event_charge || !d_mc_charge || !d_inv_charge_bandwidths || !d_charge_pdf_values)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pdf_layout(nchannels, ndaq, stride); if (rc) return rc;
    if (!(tmin < tmax) || (!time_only && !(qmin < qmax))) return set_error(CHROMA_ERR_INVALID, "empty or inverted time or charge range");
    if (nchannels == 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (one at a time with the context's other calls; it uses none of their scratch)
    hipLaunchKernelGGL(k_pdf_kernel_eval, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, (int)(time_only != 0), nchannels,
                       (int)ndaq, stride, d_event_hit, d_event_time, d_event_charge, d_mc_time, d_mc_charge, tmin, tmax, qmin, qmax,
                       d_inv_time_bandwidths, d_inv_charge_bandwidths, d_hitcount, d_time_pdf_values, d_charge_pdf_values);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_render(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const float *d_origin, const float *d_direction,
                  uint32_t alpha_depth, uint32_t *d_pixels, float *d_dx, uint32_t *d_dxlen, float *d_color, uint32_t bg_color)
{
    if (!ctx || !geom || !d_origin || !d_direction || !d_pixels || !d_dx || !d_dxlen || !d_color)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (alpha_depth < 1) return set_error(CHROMA_ERR_INVALID, "alpha_depth must be at least 1");
    if (nthreads <= 0) return CHROMA_OK;
    if (geom->stack_need > STACK_LDS + STACK_SCRATCH)
        return set_error(CHROMA_ERR_STACK, "BVH needs %u traversal stack entries, more than the %d supported", geom->stack_need, STACK_LDS + STACK_SCRATCH);
    const CallScope scope(ctx);          // (the render counts stack overflows into the context's counters)
    hipLaunchKernelGGL((k_render<STACK_LDS>), dim3((unsigned)((nthreads + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, ctx->stream,
                       geom->view, (const uint32_t *)geom->d_colors, (int)nthreads, d_origin, d_direction, alpha_depth, d_pixels, d_dx,
                       d_dxlen, (float4 *)d_color, bg_color, scope.state().d_counters);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_color_solids(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_triangle, int32_t ntriangles, const uint8_t *d_solid_hit,
                        const uint32_t *d_solid_colors, uint32_t nsolids)
{
    if (!ctx || !geom || !d_solid_hit || !d_solid_colors) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->d_colors || !geom->view.solid_id_map) return set_error(CHROMA_ERR_INVALID, "geometry was created without colors / solid_id_map");
    if (first_triangle < 0 || ntriangles < 0 || (uint64_t)first_triangle + (uint64_t)ntriangles > (uint64_t)geom->ntriangles)
        return set_error(CHROMA_ERR_INVALID, "triangles %d .. %lld of %llu", first_triangle, (long long)first_triangle + ntriangles, (unsigned long long)geom->ntriangles);
    if (ntriangles == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_color_solids, dim3((unsigned)((ntriangles + 255) / 256)), dim3(256), 0, ctx->stream, (int)first_triangle, (int)ntriangles,
                       geom->view.solid_id_map, d_solid_hit, d_solid_colors, nsolids, (uint32_t *)geom->d_colors);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

static int rays_transform(chroma_ctx *ctx, int32_t n, float *d_a, int mode, float phi, const float axis[3], const float point[3])
{
    if (!ctx || !d_a) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (n <= 0) return CHROMA_OK;
    const float zero[3] = {0.f, 0.f, 0.f};
    if (!axis) axis = zero;
    if (!point) point = zero;
    hipLaunchKernelGGL(k_rays_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, d_a, mode, phi,
                       axis[0], axis[1], axis[2], point[0], point[1], point[2]);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}
int chroma_points_translate(chroma_ctx *ctx, int32_t n, float *d_a, const float v[3]) { return rays_transform(ctx, n, d_a, 0, 0.f, nullptr, v); }
int chroma_points_rotate(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3]) { return rays_transform(ctx, n, d_a, 1, phi, axis, nullptr); }
int chroma_points_rotate_around_point(chroma_ctx *ctx, int32_t n, float *d_a, float phi, const float axis[3], const float point[3])
{ return rays_transform(ctx, n, d_a, 2, phi, axis, point); }

int chroma_probe(chroma_ctx *ctx, int32_t fn, uint64_t n, const float *d_x, const float *d_tab_x, const float *d_tab_f,
                 uint32_t ntab, float start, float step, float *d_out)
{
    if (!ctx || !d_x || !d_out || fn < 0 || fn > 4) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if ((fn == 0 && (!d_tab_f || ntab < 2)) || (fn == 1 && (!d_tab_x || ntab < 2)) || (fn == 2 && (!d_tab_x || !d_tab_f || ntab < 2)))
        return set_error(CHROMA_ERR_INVALID, "probe %d: table missing", fn);
    if (n == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)fn, n, d_x, d_tab_x, d_tab_f,
                       ntab, start, step, d_out);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_probe_math(chroma_ctx *ctx, int32_t op, uint64_t n, const void *d_x, const void *d_y, const void *d_z, void *d_out)
{
    if (!ctx || !d_x || !d_out || op < 0 || op >= PROBE_MATH_NOPS) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (((op == 7 || (op >= 15 && op <= 18)) && !d_y) || (op == 18 && !d_z))
        return set_error(CHROMA_ERR_INVALID, "probe_math %d: operand array missing", op);
    if (n >= (1ull << 31)) return set_error(CHROMA_ERR_INVALID, "probe_math: too many elements");
    if (n == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_probe_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)op, n, (const uint32_t *)d_x,
                       (const uint32_t *)d_y, (const uint32_t *)d_z, (uint32_t *)d_out);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_generate_bomb(chroma_ctx *ctx, const chroma_photon_arrays *photons, uint64_t nphotons, uint64_t seed,
                         uint64_t id_base, const float pos[3], float wavelength_lo, float wavelength_hi)
{
    if (!ctx || !pos) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(photons, true); if (rc) return rc;
    if (nphotons == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_generate_bomb, dim3((unsigned)((nphotons + 255) / 256)), dim3(256), 0, ctx->stream, to_view(photons),
                       (uint64_t)nphotons, seed, id_base, pos[0], pos[1], pos[2], wavelength_lo, wavelength_hi);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// ---- an exclusive sum in place for the other translation units (chroma_propagate_tracks: rows per photon -> offsets) ----
// Scratch from the context's pool, freed behind the stream's work.
int chroma_internal_exclusive_sum(chroma_ctx *ctx, uint32_t *d_counts, uint32_t n)
{
    if (n == 0) return CHROMA_OK;
    if (n >= 0x7fffffffu) return set_error(CHROMA_ERR_INVALID, "exclusive_sum: bad argument");
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_counts, d_counts, (int)n, ctx->stream));
    void *tmp = nullptr;
    int rc = chroma_malloc(ctx, std::max<size_t>(tmp_bytes, 4), &tmp);
    if (rc != CHROMA_OK) return rc;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_counts, d_counts, (int)n, ctx->stream);
    chroma_free(ctx, tmp);                 // (parked behind the scan)
    if (e != hipSuccess) return set_error((int)e, "exclusive_sum: %s", hipGetErrorString(e));
    return CHROMA_OK;
}

}  // extern "C"

// ... and for the pipelines of daq_calls.hip and steps_calls.hip, which carve the workspace out of their own block; their radix
// sort of (64-bit key, index) pairs here as well, because hipCUB's sort and scan share a kernel
int scan_workspace_bytes(size_t n, hipStream_t stream, size_t *bytes)
{
    uint32_t *nul = nullptr;
    *bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, nul, nul, (int)n, stream));
    return CHROMA_OK;
}

int exclusive_sum(void *workspace, size_t bytes, uint32_t *d_in, uint32_t *d_out, size_t n, hipStream_t stream)
{
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(workspace, bytes, d_in, d_out, (int)n, stream));
    return CHROMA_OK;
}

int sort_pairs_workspace_bytes(size_t n, int end_bit, hipStream_t stream, size_t *bytes)
{
    uint64_t *k = nullptr; uint32_t *v = nullptr;
    *bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, k, k, v, v, (int)n, 0, end_bit, stream));
    return CHROMA_OK;
}

int sort_pairs(void *workspace, size_t bytes, const uint64_t *d_keys, uint64_t *d_keys_out, const uint32_t *d_values, uint32_t *d_values_out,
               size_t n, int end_bit, hipStream_t stream)
{
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(workspace, bytes, d_keys, d_keys_out, d_values, d_values_out, (int)n, 0, end_bit, stream));
    return CHROMA_OK;
}
