// daq_calls.hip -- the DAQ's entry points: the single-launch acquisitions (chroma/cuda/daq.cu's, as kernel_calls.hip has its calls)
// and the pipelines behind them -- the per-event acquisition and its compaction, the time-binned DAQ with its dark noise, its
// trigger, its digitiser and the reduction of its traces.  A pipeline is several launches with a sort, a scan or a read-back between them, on the context's pooled scratch
// block, which each lays out through ONE description (chroma_internal.h: Carver).
#include <stdint.h>
#include <algorithm>
#include <cmath>

#include "chroma_internal.h"
#include "propagate_device.h"

#include "kernels_daq.h"
#include "kernels_daq_pulses.h"
#include "kernels_daq_noise.h"
#include "kernels_daq_trigger.h"
#include "kernels_daq_digitize.h"
#include "kernels_daq_reduce.h"

// ---- what more than one call refuses ----
static int check_daq_tables(const chroma_daq_tables *tables)
{
    if (tables->time_cdf_len < 2 || tables->charge_cdf_len < 2 || !tables->d_time_cdf_x || !tables->d_time_cdf_y ||
        !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need two CDFs of at least 2 points and a positive charge unit");
    return CHROMA_OK;
}

static int check_event_bounds(uint32_t nrows, const uint32_t *bounds, uint32_t nphotons)
{
    for (uint32_t r = 0; r < nrows; r++)
        if (bounds[r] > bounds[r + 1]) return set_error(CHROMA_ERR_INVALID, "event bounds: bound %u is below bound %u", r + 1, r);
    if (bounds[nrows] > nphotons || bounds[nrows] > 0x7fffffffu)
        return set_error(CHROMA_ERR_INVALID, "event bounds: the last bound %u is beyond the %u photons of the set", bounds[nrows], nphotons);
    return CHROMA_OK;
}

static int check_daq_window(const chroma_daq_window *window)
{
    if (!(window->dt > 0.0f) || !std::isfinite(window->dt) || !std::isfinite(window->t0) || window->nbins < 1 || window->nbins > 65536)
        return set_error(CHROMA_ERR_INVALID, "DAQ window: need a finite t0, a finite positive dt and 1 .. 65536 bins");
    return CHROMA_OK;
}

// ---- what the pulses and the trigger's gated hits share: a reduction by key ----
// the bits a radix sort of the keys 0 .. nkeys - 1 has to look at
static int key_bits(uint64_t nkeys)
{
    int end_bit = 1;
    while (end_bit < 64 && ((nkeys - 1) >> end_bit)) end_bit++;
    return end_bit;
}

// (key, index) pairs before and behind their sort, the heads of the sorted keys -- n + 1 flags, then (in place) their exclusive
// sum -- and the workspaces of the sort and of the scan.  Each block description puts the arrays where it always had them.
struct KeySort {
    uint64_t *keys, *keys_sorted;
    uint32_t *order, *order_sorted, *positions;
    void *sort, *scan;
    size_t sort_bytes = 0, scan_bytes = 0;
};

// The first n pairs sorted on the keys' bits [0, end_bit), k_daq_pulses_heads over the sorted keys, the exclusive sum, and the number
// of distinct keys read back (the stream drained).  What a caller launches behind it (open, reduce, finish) is its own.
static int count_sorted_keys(hipStream_t stream, const KeySort &k, uint32_t n, int end_bit, uint32_t *total)
{
    int rc = sort_pairs(k.sort, k.sort_bytes, k.keys, k.keys_sorted, k.order, k.order_sorted, n, end_bit, stream); if (rc) return rc;
    hipLaunchKernelGGL(k_daq_pulses_heads, dim3(n / DAQ_PULSES_BLOCK + 1), dim3(DAQ_PULSES_BLOCK), 0, stream, n, k.keys_sorted, k.positions);
    HIP_TRY(hipGetLastError());
    rc = exclusive_sum(k.scan, k.scan_bytes, k.positions, k.positions, (size_t)n + 1, stream); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(total, k.positions + n, sizeof(*total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

// ---- the time-binned DAQ (kernels_daq_pulses.h) ----
// what chroma_daq_acquire_events refuses, and the window's rules
static int check_pulses_call(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows, const uint32_t *bounds,
                             const chroma_photon_arrays *photons, uint32_t nphotons, const chroma_daq_window *window)
{
    if (!ctx || !geom || !tables || !bounds || !window) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids || !geom->view.nchannels) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (nrows < 1) return set_error(CHROMA_ERR_INVALID, "need at least one row");
    int rc = check_daq_window(window); if (rc) return rc;
    if ((uint64_t)nrows * geom->view.nchannels > 0x7fffffffffffffffull / window->nbins)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u channels of %u bins: more than 63-bit keys hold, pass fewer rows", nrows,
                         geom->view.nchannels, window->nbins);
    rc = check_event_bounds(nrows, bounds, nphotons); if (rc) return rc;
    rc = check_daq_tables(tables); if (rc) return rc;
    return check_photons(photons, false);
}

// The counters of a pulses call, 256 bytes behind the bounds: word 0 the accepted in-window photons (k_daq_pulses_count), word 1 the
// cursor both emits append through, words 2 and 3 the 64-bit count of kept noise photoelectrons (k_daq_noise_count)
enum PulsesCounter { PULSES_PHOTONS = 0, PULSES_CURSOR = 1, PULSES_NOISE = 2, PULSES_COUNTERS = 4 };

// The pooled block of a pulses call: the bounds, the counters, the rows' early and late photons and (behind them) noise counts; then,
// per accepted photon and noise photoelectron, the keys and their positions before and behind the sort, charge count, time bits and
// history; the heads (n + 1); the workspaces of the sort and of the scan.  The count pass lays it out for n = 0 and the acquisition
// again for the n it counted: one description, so what the count pass used is where it was.
struct PulsesBlock {
    uint32_t *bounds = nullptr, *counters, *rows_outside, *rows_noise, *charge, *time, *history;
    KeySort keys;

    void lay(Carver &c, uint32_t nrows, uint32_t n)
    {
        bounds = c.take<uint32_t>((size_t)nrows + 1);
        counters = c.take<uint32_t>(PULSES_COUNTERS);
        rows_outside = c.take<uint32_t>(3 * (size_t)nrows);
        rows_noise = rows_outside ? rows_outside + 2 * (size_t)nrows : nullptr;
        keys.keys = c.take<uint64_t>(n); keys.keys_sorted = c.take<uint64_t>(n);
        keys.order = c.take<uint32_t>(n); keys.order_sorted = c.take<uint32_t>(n);
        charge = c.take<uint32_t>(n); time = c.take<uint32_t>(n); history = c.take<uint32_t>(n);
        keys.positions = c.take<uint32_t>((size_t)n + 1);
        keys.sort = c.take<char>(keys.sort_bytes); keys.scan = c.take<char>(keys.scan_bytes);
    }
};

// Lays `b` out for n entries on the context's scratch, grown to hold it.  THE RULE: the bounds live at offset 0, and they are copied
// up when this is the call's first layout or the block grew (a grown block is a new one: what the call had in it is lost).
static int place_pulses_block(const CallScope &scope, PulsesBlock *b, uint32_t nrows, const uint32_t *bounds, uint32_t n)
{
    const bool first = !b->bounds;
    bool grew = false;
    int rc = carve_call_scratch(scope, [&](Carver &c) { b->lay(c, nrows, n); }, &grew); if (rc) return rc;
    if (!first && !grew) return CHROMA_OK;
    HIP_TRY(hipMemcpyAsync(b->bounds, bounds, ((size_t)nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, scope.ctx->stream));
    HIP_TRY(hipStreamSynchronize(scope.ctx->stream));          // (the caller's bounds are his again when the call returns)
    return CHROMA_OK;
}

// what the calls with noise refuse besides (noise NULL: nothing)
static int check_pulses_noise(const chroma_geometry *geom, uint32_t nrows, uint32_t nphotons, chroma_rng rng, const chroma_daq_noise *noise)
{
    if (!noise) return CHROMA_OK;
    if (const char *why = daq_noise::check(noise)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if ((uint64_t)nrows * geom->view.nchannels > 0xffffffffull)
        return set_error(CHROMA_ERR_INVALID, "DAQ noise: %u rows of %u channels: more than 32-bit word indices hold, pass fewer rows", nrows, geom->view.nchannels);
    const uint64_t last_id = rng.photon_id_base + (nphotons ? nphotons - 1u : 0u);
    if (nphotons && ((rng.photon_id_base >> 32) == daq_noise::ID_HIGH || (last_id >> 32) == daq_noise::ID_HIGH || last_id < rng.photon_id_base))
        return set_error(CHROMA_ERR_INVALID, "DAQ noise: the photon ids reach the high word 0xffffffff of the noise's pseudo-photons");
    return CHROMA_OK;
}

static DaqNoiseView noise_view(const chroma_daq_noise *noise)
{
    DaqNoiseView v;
    for (uint32_t j = 0; j < 64u; j++) v.count_cdf[j] = j < noise->ncount ? noise->count_cdf[j] : 0xffffffffu;
    v.ncount = noise->ncount;
    v.flag = noise->flag;
    v.accept = noise->d_accept;
    return v;
}

// The accepted in-window photons of the window (k_daq_pulses_count) and, with `noise`, the kept noise photoelectrons of the rows'
// words (k_daq_noise_count), with the bounds already in the block; the two counters read back
static int pulses_count(const CallScope &scope, const PulsesBlock &b, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                        uint32_t span, uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng, uint32_t acquisition,
                        float global_weight, const chroma_daq_window *window, const chroma_daq_noise *noise, uint64_t *naccepted)
{
    hipStream_t stream = scope.ctx->stream;
    HIP_TRY(hipMemsetAsync(b.counters, 0, PULSES_COUNTERS * sizeof(uint32_t), stream));
    if (span) {
        hipLaunchKernelGGL(k_daq_pulses_count, dim3((span + DAQ_PULSES_SPAN - 1) / DAQ_PULSES_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream, geom->view,
                           *tables, *window, nrows, b.bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                           photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, b.counters + PULSES_PHOTONS);
        HIP_TRY(hipGetLastError());
    }
    if (noise) {
        const uint32_t nwords = nrows * geom->view.nchannels;
        hipLaunchKernelGGL(k_daq_noise_count, dim3((nwords + DAQ_NOISE_SPAN - 1) / DAQ_NOISE_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream,
                           noise_view(noise), geom->view.nchannels, nwords, rng.seed, acquisition, (unsigned long long *)(b.counters + PULSES_NOISE));
        HIP_TRY(hipGetLastError());
    }
    uint32_t counts[PULSES_COUNTERS] = {0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(counts, b.counters, sizeof(counts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *naccepted = (uint64_t)counts[PULSES_PHOTONS] + (((uint64_t)counts[PULSES_NOISE + 1] << 32) | counts[PULSES_NOISE]);
    return CHROMA_OK;
}

// ---- the trigger of the time-binned DAQ (kernels_daq_trigger.h) ----
// The pooled block of a trigger call over n pulses, sized once from the bounds (growing it would lose what is in it): the sum per
// (row, bin); per pulse its row, its trigger, the indices before and behind the sort, the bin that k_daq_pulses_open writes, the
// gated flags and their scan (n + 1), the heads (n + 1), the keys before and behind the sort; per row the counts and their scan
// (nrows + 1); per trigger (`room`: the most there can be) its bin and sum; the workspaces
struct TriggerBlock {
    uint32_t *sum, *rows, *of, *hit_bin, *gated, *row_triggers, *bins, *sums;
    KeySort keys;

    void lay(Carver &c, uint32_t nrows, uint32_t nbins, uint32_t n, uint32_t room)
    {
        sum = c.take<uint32_t>((size_t)nrows * nbins);
        rows = c.take<uint32_t>(n);
        of = c.take<uint32_t>(n);          // the trigger of every pulse
        keys.order = c.take<uint32_t>(n); keys.order_sorted = c.take<uint32_t>(n);
        hit_bin = c.take<uint32_t>(n);
        gated = c.take<uint32_t>((size_t)n + 1);          // the flags, then (in place) their exclusive sum
        keys.positions = c.take<uint32_t>((size_t)n + 1);
        keys.keys = c.take<uint64_t>(n); keys.keys_sorted = c.take<uint64_t>(n);
        row_triggers = c.take<uint32_t>((size_t)nrows + 1);          // the counts, then (in place) the rows' offsets
        bins = c.take<uint32_t>(room); sums = c.take<uint32_t>(room);
        keys.sort = c.take<char>(keys.sort_bytes); keys.scan = c.take<char>(keys.scan_bytes);
    }
};

extern "C" {

// (chroma_daq_count_pulses is this call without noise)
int chroma_daq_count_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                                  const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                                  chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                  const chroma_daq_noise *noise, uint64_t *naccepted)
{
    if (!naccepted) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pulses_call(ctx, geom, tables, nrows, bounds, photons, nphotons, window); if (rc) return rc;
    rc = check_pulses_noise(geom, nrows, nphotons, rng, noise); if (rc) return rc;
    *naccepted = 0;
    const uint32_t span = bounds[nrows] - bounds[0];
    if (span == 0 && !noise) return CHROMA_OK;
    const CallScope scope(ctx);
    PulsesBlock b;
    rc = place_pulses_block(scope, &b, nrows, bounds, 0); if (rc) return rc;
    return pulses_count(scope, b, geom, tables, nrows, span, detection_state, photons, rng, acquisition, global_weight, window, noise, naccepted);
}

int chroma_daq_count_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                            const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                            chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                            uint64_t *naccepted)
{
    return chroma_daq_count_pulses_noise(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight,
                                         window, nullptr, naccepted);
}

// (chroma_daq_acquire_pulses is this call without noise and without the rows' noise counts)
int chroma_daq_acquire_pulses_noise(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                                    const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                                    chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                                    const chroma_daq_noise *noise, uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel,
                                    uint32_t *d_bin, uint32_t *d_npe, uint32_t *d_q_int, float *d_t_first, uint32_t *d_flags,
                                    uint32_t *d_outside, uint32_t *d_row_noise, uint64_t *npulses)
{
    if (!d_offsets || !d_outside || !npulses || (capacity && (!d_channel || !d_bin || !d_npe || !d_q_int || !d_t_first || !d_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_pulses_call(ctx, geom, tables, nrows, bounds, photons, nphotons, window); if (rc) return rc;
    rc = check_pulses_noise(geom, nrows, nphotons, rng, noise); if (rc) return rc;
    *npulses = 0;
    hipStream_t stream = ctx->stream;
    const size_t offsets_bytes = ((size_t)nrows + 1) * sizeof(uint32_t), outside_bytes = 2 * (size_t)nrows * sizeof(uint32_t);
    const size_t row_noise_bytes = (size_t)nrows * sizeof(uint32_t);
    const uint32_t span = bounds[nrows] - bounds[0];
    if (span == 0 && !noise) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream));
        HIP_TRY(hipMemsetAsync(d_outside, 0, outside_bytes, stream));
        if (d_row_noise) HIP_TRY(hipMemsetAsync(d_row_noise, 0, row_noise_bytes, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return CHROMA_OK;
    }
    const CallScope scope(ctx);
    PulsesBlock b;
    rc = place_pulses_block(scope, &b, nrows, bounds, 0); if (rc) return rc;
    uint64_t accepted = 0;
    rc = pulses_count(scope, b, geom, tables, nrows, span, detection_state, photons, rng, acquisition, global_weight, window, noise, &accepted);
    if (rc) return rc;
    if (accepted >= 0x7fffffffull)
        return set_error(CHROMA_ERR_INVALID, "%llu accepted photons and noise photoelectrons: more than the scan's 31-bit count holds, pass fewer rows",
                         (unsigned long long)accepted);
    const uint32_t n = (uint32_t)accepted;
    const int end_bit = key_bits((uint64_t)nrows * geom->view.nchannels * window->nbins);
    if (n) {
        rc = sort_pairs_workspace_bytes(n, end_bit, stream, &b.keys.sort_bytes); if (rc) return rc;
        rc = scan_workspace_bytes((size_t)n + 1, stream, &b.keys.scan_bytes); if (rc) return rc;
    }
    rc = place_pulses_block(scope, &b, nrows, bounds, n); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(b.counters + PULSES_CURSOR, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(b.rows_outside, 0, outside_bytes + row_noise_bytes, stream));
    // both emits before the sort, onto one cursor: the photons' entries and the noise's lie among one another
    if (span) {
        hipLaunchKernelGGL(k_daq_pulses_emit, dim3((span + DAQ_PULSES_SPAN - 1) / DAQ_PULSES_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream, geom->view,
                           *tables, *window, nrows, b.bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                           photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, n, b.counters + PULSES_CURSOR, b.keys.keys,
                           b.keys.order, b.charge, b.time, b.history, b.rows_outside);
        HIP_TRY(hipGetLastError());
    }
    if (noise) {
        const uint32_t nwords = nrows * geom->view.nchannels;
        hipLaunchKernelGGL(k_daq_noise_emit, dim3((nwords + DAQ_NOISE_SPAN - 1) / DAQ_NOISE_SPAN), dim3(DAQ_PULSES_BLOCK), 0, stream,
                           noise_view(noise), *tables, *window, geom->view.nchannels, nwords, rng.seed, acquisition, n, b.counters + PULSES_CURSOR,
                           b.keys.keys, b.keys.order, b.charge, b.time, b.history, b.rows_noise);
        HIP_TRY(hipGetLastError());
    }
    if (n) {
        const dim3 grid((n + 1 + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), block(DAQ_PULSES_BLOCK);
        uint32_t total = 0;
        rc = count_sorted_keys(stream, b.keys, n, end_bit, &total); if (rc) return rc;
        *npulses = total;
        if (total > capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu pulses, the rows hold %u", (unsigned long long)capacity, total);
        hipLaunchKernelGGL(k_daq_pulses_open, grid, block, 0, stream, n, geom->view.nchannels, window->nbins, b.keys.keys_sorted, b.keys.positions,
                           d_channel, d_bin, d_npe, d_q_int, (uint32_t *)d_t_first, d_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_reduce, dim3((n + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), dim3(DAQ_PULSES_BLOCK), 0, stream, n,
                           b.keys.keys_sorted, b.keys.positions, b.keys.order_sorted, b.charge, b.time, b.history, d_npe, d_q_int,
                           (uint32_t *)d_t_first, d_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_finish, dim3((std::max(total, nrows + 1) + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), block, 0, stream, n, total, nrows,
                           (uint64_t)geom->view.nchannels * window->nbins, b.keys.keys_sorted, b.keys.positions, (uint32_t *)d_t_first, d_offsets);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream));
    }
    HIP_TRY(hipMemcpyAsync(d_outside, b.rows_outside, outside_bytes, hipMemcpyDeviceToDevice, stream));
    if (d_row_noise) HIP_TRY(hipMemcpyAsync(d_row_noise, b.rows_noise, row_noise_bytes, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_daq_acquire_pulses(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                              const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons, uint32_t nphotons,
                              chroma_rng rng, uint32_t acquisition, float global_weight, const chroma_daq_window *window,
                              uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel, uint32_t *d_bin, uint32_t *d_npe,
                              uint32_t *d_q_int, float *d_t_first, uint32_t *d_flags, uint32_t *d_outside, uint64_t *npulses)
{
    return chroma_daq_acquire_pulses_noise(ctx, geom, tables, nrows, bounds, detection_state, photons, nphotons, rng, acquisition, global_weight,
                                           window, nullptr, capacity, d_offsets, d_channel, d_bin, d_npe, d_q_int, d_t_first, d_flags, d_outside,
                                           nullptr, npulses);
}

int chroma_daq_reset(chroma_ctx *ctx, float maxtime, uint32_t nchannels, uint32_t *d_earliest_time_int,
                     uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nchannels == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_daq_reset, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, maxtime, nchannels,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, int32_t first_photon,
                       int32_t nphotons, uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng,
                       uint32_t acquisition, float global_weight, uint32_t *d_earliest_time_int,
                       uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    int rc = check_daq_tables(tables); if (rc) return rc;
    rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons <= 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_run_daq, dim3((nphotons + 255) / 256), dim3(256), 0, ctx->stream, geom->view, *tables, first_photon,
                       nphotons, detection_state, photons->t, photons->flags, photons->last_hit_triangles, photons->weights,
                       rng.seed, rng.photon_id_base, acquisition, global_weight, d_earliest_time_int, d_channel_q_int,
                       d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire_many(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, int32_t first_photon,
                            int32_t nphotons, uint32_t detection_state, const chroma_photon_arrays *photons, chroma_rng rng,
                            uint32_t acquisition, float global_weight, int32_t ndaq, int32_t channel_stride,
                            uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int, uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (ndaq < 1 || channel_stride < (int32_t)geom->view.nchannels)
        return set_error(CHROMA_ERR_INVALID, "ndaq must be positive and the channel stride at least the number of channels");
    int rc = check_daq_tables(tables); if (rc) return rc;
    rc = check_photons(photons, false); if (rc) return rc;
    if (nphotons <= 0) return CHROMA_OK;
    const long long total = (long long)nphotons * ndaq;
    hipLaunchKernelGGL(k_run_daq_many, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, geom->view, *tables,
                       first_photon, nphotons, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                       photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, ndaq, channel_stride,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_acquire_events(chroma_ctx *ctx, chroma_geometry *geom, const chroma_daq_tables *tables, uint32_t nrows,
                              const uint32_t *bounds, uint32_t detection_state, const chroma_photon_arrays *photons,
                              uint32_t nphotons, chroma_rng rng, uint32_t acquisition, float global_weight,
                              uint32_t channel_stride, uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                              uint32_t *d_channel_histories)
{
    if (!ctx || !geom || !tables || !bounds || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
    if (nrows < 1 || channel_stride < geom->view.nchannels)
        return set_error(CHROMA_ERR_INVALID, "need at least one row and a channel stride of at least the number of channels");
    if ((uint64_t)nrows * channel_stride > 0xffffffffull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u words: more than 32-bit word indices hold, pass fewer rows", nrows, channel_stride);
    int rc = check_event_bounds(nrows, bounds, nphotons); if (rc) return rc;
    rc = check_daq_tables(tables); if (rc) return rc;
    rc = check_photons(photons, false); if (rc) return rc;
    const uint32_t window = bounds[nrows] - bounds[0];
    if (window == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    uint32_t *d_bounds = nullptr;          // the block: the bounds
    rc = carve_call_scratch(scope, [&](Carver &c) { d_bounds = c.take<uint32_t>((size_t)nrows + 1); }); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_bounds, bounds, ((size_t)nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));          // (the caller's bounds are his again when the call returns)
    hipLaunchKernelGGL(k_run_daq_events, dim3((window + DAQ_EVENTS_BLOCK - 1) / DAQ_EVENTS_BLOCK), dim3(DAQ_EVENTS_BLOCK), 0, ctx->stream,
                       geom->view, *tables, nrows, d_bounds, detection_state, photons->t, photons->flags, photons->last_hit_triangles,
                       photons->weights, rng.seed, rng.photon_id_base, acquisition, global_weight, channel_stride,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_compact_events(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, uint32_t channel_stride, float charge_unit,
                              const uint32_t *d_earliest_time_int, const uint32_t *d_channel_q_int,
                              const uint32_t *d_channel_histories, uint64_t capacity, uint32_t *d_offsets, int32_t *d_channel,
                              float *d_t, float *d_q, uint32_t *d_flags, uint64_t *ntouched)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories || !d_offsets || !ntouched ||
        (capacity && (!d_channel || !d_t || !d_q || !d_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    *ntouched = 0;
    if (nrows < 1 || nchannels < 1 || channel_stride < nchannels)
        return set_error(CHROMA_ERR_INVALID, "need at least one row, one channel and a channel stride of at least the number of channels");
    if ((uint64_t)nrows * channel_stride > 0xffffffffull || (uint64_t)nrows * nchannels >= 0x7fffffffull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u words: more than the scan's 31-bit count holds, pass fewer rows", nrows, channel_stride);
    const CallScope scope(ctx);
    const uint32_t nwords = nrows * nchannels, nflags = nwords + 1;
    size_t scan_bytes = 0;
    int rc = scan_workspace_bytes(nflags, ctx->stream, &scan_bytes); if (rc) return rc;
    uint32_t *d_positions = nullptr; void *d_scan = nullptr;          // the block: the flags, then (in place) their exclusive sum; the scan's workspace
    rc = carve_call_scratch(scope, [&](Carver &c) { d_positions = c.take<uint32_t>(nflags); d_scan = c.take<char>(scan_bytes); }); if (rc) return rc;
    const dim3 grid((nflags + 255) / 256), block(256);
    hipLaunchKernelGGL(k_daq_events_flag, grid, block, 0, ctx->stream, nwords, nchannels, channel_stride, d_channel_histories, d_positions);
    HIP_TRY(hipGetLastError());
    rc = exclusive_sum(d_scan, scan_bytes, d_positions, d_positions, nflags, ctx->stream); if (rc) return rc;
    hipLaunchKernelGGL(k_daq_events_scatter, grid, block, 0, ctx->stream, nwords, nchannels, channel_stride, charge_unit,
                       d_earliest_time_int, d_channel_q_int, d_channel_histories, d_positions, capacity, d_offsets, d_channel,
                       (uint32_t *)d_t, d_q, d_flags);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_positions + nwords, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *ntouched = total;
    if (total > capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu touched words, the state holds %u", (unsigned long long)capacity, total);
    return CHROMA_OK;
}

int chroma_daq_convert(chroma_ctx *ctx, uint32_t nchannels, float charge_unit, const uint32_t *d_earliest_time_int,
                       const uint32_t *d_channel_q_int, float *d_earliest_time, float *d_channel_q)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_earliest_time || !d_channel_q)
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nchannels == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_daq_convert, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, nchannels, charge_unit,
                       d_earliest_time_int, d_channel_q_int, d_earliest_time, d_channel_q);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_daq_trigger_pulses(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                              const chroma_daq_trigger *trigger, const uint32_t *d_offsets, const int32_t *d_channel, const uint32_t *d_bin,
                              const uint32_t *d_npe, const uint32_t *d_q_int, const float *d_t_first, const uint32_t *d_flags, uint64_t npulses,
                              uint64_t trigger_capacity, uint32_t *d_trig_offsets, uint32_t *d_trig_bin, uint32_t *d_trig_sum,
                              uint32_t *d_hit_offsets, uint64_t hit_capacity, int32_t *d_hit_channel, uint32_t *d_hit_npe, uint32_t *d_hit_q_int,
                              float *d_hit_t_first, uint32_t *d_hit_flags, uint32_t *d_pulse_trigger, uint64_t *ntriggers, uint64_t *nhits)
{
    if (!ctx || !window || !trigger || !d_offsets || !d_trig_offsets || !d_hit_offsets || !ntriggers || !nhits ||
        (npulses && (!d_channel || !d_bin || !d_npe || !d_q_int || !d_t_first || !d_flags)) || (trigger_capacity && (!d_trig_bin || !d_trig_sum)) ||
        (hit_capacity && (!d_hit_channel || !d_hit_npe || !d_hit_q_int || !d_hit_t_first || !d_hit_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nrows < 1 || nchannels < 1 || nchannels > 0x7fffffffu) return set_error(CHROMA_ERR_INVALID, "need at least one row and 1 .. 2^31 - 1 channels");
    int rc = check_daq_window(window); if (rc) return rc;
    const uint32_t nbins = window->nbins;
    if (trigger->kind != CHROMA_TRIGGER_NHIT && trigger->kind != CHROMA_TRIGGER_NPE) return set_error(CHROMA_ERR_INVALID, "DAQ trigger: unknown kind %u", trigger->kind);
    if (trigger->threshold < 1 || trigger->width < 1 || trigger->width > nbins || trigger->post < 1 ||
        trigger->holdoff < std::max<uint64_t>(1, (uint64_t)trigger->pre + trigger->post))
        return set_error(CHROMA_ERR_INVALID, "DAQ trigger: need a threshold of at least 1, a width of 1 .. %u bins, post >= 1 and holdoff >= max(1, pre + post)", nbins);
    if (npulses >= 0x7fffffffull) return set_error(CHROMA_ERR_INVALID, "%llu pulses: more than the scan's 31-bit count holds, pass fewer rows", (unsigned long long)npulses);
    if ((uint64_t)nrows * nbins >= 0x80000000ull)
        return set_error(CHROMA_ERR_INVALID, "%u rows of %u bins: more than 31-bit (row, bin) indices hold, pass fewer rows", nrows, nbins);
    hipStream_t stream = ctx->stream;
    const size_t offsets_bytes = ((size_t)nrows + 1) * sizeof(uint32_t);
    if (npulses == 0) {
        *ntriggers = 0; *nhits = 0;
        HIP_TRY(hipMemsetAsync(d_trig_offsets, 0, offsets_bytes, stream));
        HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(uint32_t), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return CHROMA_OK;
    }
    // (what lies beyond the window changes nothing: a lockout, a gate or a reach of more than nbins bins is one of nbins)
    const uint32_t n = (uint32_t)npulses, holdoff = std::min(trigger->holdoff, nbins), pre = std::min(trigger->pre, nbins), post = std::min(trigger->post, nbins);
    const uint64_t per_row = (nbins + holdoff - 1) / holdoff, per_pulse = (trigger->width + holdoff - 1) / holdoff;
    const uint32_t room = (uint32_t)std::min<uint64_t>((uint64_t)nrows * per_row, (uint64_t)n * per_pulse);          // (<= nrows * nbins < 2^31)
    const CallScope scope(ctx);
    TriggerBlock b;
    size_t scan_rows_bytes = 0;
    rc = sort_pairs_workspace_bytes(n, 64, stream, &b.keys.sort_bytes); if (rc) return rc;
    rc = scan_workspace_bytes((size_t)n + 1, stream, &b.keys.scan_bytes); if (rc) return rc;
    rc = scan_workspace_bytes((size_t)nrows + 1, stream, &scan_rows_bytes); if (rc) return rc;
    b.keys.scan_bytes = std::max(b.keys.scan_bytes, scan_rows_bytes);          // (one workspace for the scans over pulses and over rows)
    rc = carve_call_scratch(scope, [&](Carver &c) { b.lay(c, nrows, nbins, n, room); }); if (rc) return rc;
    const dim3 block(DAQ_TRIGGER_BLOCK), per_pulse_grid((n + DAQ_TRIGGER_BLOCK - 1) / DAQ_TRIGGER_BLOCK), per_pulse1_grid(n / DAQ_TRIGGER_BLOCK + 1);
    HIP_TRY(hipMemsetAsync(b.sum, 0, (size_t)nrows * nbins * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_daq_trigger_edges, per_pulse_grid, block, 0, stream, n, nrows, nchannels, nbins, trigger->kind, trigger->width, d_offsets, d_channel,
                       d_bin, d_npe, b.rows, b.sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_daq_trigger_count, dim3(nrows / DAQ_TRIGGER_WAVES + 1), block, 0, stream, nrows, nbins, trigger->threshold, holdoff, b.sum, b.row_triggers);
    HIP_TRY(hipGetLastError());
    rc = exclusive_sum(b.keys.scan, b.keys.scan_bytes, b.row_triggers, b.row_triggers, (size_t)nrows + 1, stream); if (rc) return rc;
    uint32_t total = 0, ngated = 0, total_hits = 0;
    HIP_TRY(hipMemcpyAsync(&total, b.row_triggers + nrows, sizeof(total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total > room) return set_error(CHROMA_ERR_INTERNAL, "DAQ trigger: %u firings, the bound is %u", total, room);
    if (total) {
        hipLaunchKernelGGL(k_daq_trigger_fire, dim3((nrows + DAQ_TRIGGER_WAVES - 1) / DAQ_TRIGGER_WAVES), block, 0, stream, nrows, nbins, trigger->threshold,
                           holdoff, b.sum, b.row_triggers, room, b.bins, b.sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_trigger_gates, per_pulse1_grid, block, 0, stream, n, pre, post, b.rows, d_bin, b.row_triggers, b.bins, b.of, b.gated);
        HIP_TRY(hipGetLastError());
        rc = exclusive_sum(b.keys.scan, b.keys.scan_bytes, b.gated, b.gated, (size_t)n + 1, stream); if (rc) return rc;
        hipLaunchKernelGGL(k_daq_trigger_compact, per_pulse_grid, block, 0, stream, n, nchannels, b.of, d_channel, b.gated, n, b.keys.keys, b.keys.order);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ngated, b.gated + n, sizeof(ngated), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ngated) { rc = count_sorted_keys(stream, b.keys, ngated, key_bits((uint64_t)total * nchannels), &total_hits); if (rc) return rc; }
    *ntriggers = total; *nhits = total_hits;
    if (total > trigger_capacity || total_hits > hit_capacity)
        return set_error(CHROMA_ERR_INVALID, "room for %llu triggers and %llu hits, the rows hold %u and %u", (unsigned long long)trigger_capacity,
                         (unsigned long long)hit_capacity, total, total_hits);
    // nothing of the caller's was written so far
    HIP_TRY(hipMemcpyAsync(d_trig_offsets, b.row_triggers, offsets_bytes, hipMemcpyDeviceToDevice, stream));
    if (total) {
        HIP_TRY(hipMemcpyAsync(d_trig_bin, b.bins, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_trig_sum, b.sums, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
    if (d_pulse_trigger) {
        if (total) { HIP_TRY(hipMemcpyAsync(d_pulse_trigger, b.of, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream)); }
        else { HIP_TRY(hipMemsetAsync(d_pulse_trigger, 0xff, (size_t)n * sizeof(uint32_t), stream)); }
    }
    if (ngated) {
        const dim3 pulses_block(DAQ_PULSES_BLOCK);
        hipLaunchKernelGGL(k_daq_pulses_open, dim3((ngated + DAQ_PULSES_BLOCK - 1) / DAQ_PULSES_BLOCK), pulses_block, 0, stream, ngated, nchannels, 1u,
                           b.keys.keys_sorted, b.keys.positions, d_hit_channel, b.hit_bin, d_hit_npe, d_hit_q_int, (uint32_t *)d_hit_t_first, d_hit_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_trigger_reduce, dim3((ngated + DAQ_TRIGGER_BLOCK - 1) / DAQ_TRIGGER_BLOCK), block, 0, stream, ngated, b.keys.keys_sorted,
                           b.keys.positions, b.keys.order_sorted, d_npe, d_q_int, (const uint32_t *)d_t_first, d_flags, d_hit_npe, d_hit_q_int,
                           (uint32_t *)d_hit_t_first, d_hit_flags);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_daq_pulses_finish, dim3(std::max(total_hits, total + 1) / DAQ_PULSES_BLOCK + 1), pulses_block, 0, stream, ngated, total_hits,
                           total, (uint64_t)nchannels, b.keys.keys_sorted, b.keys.positions, (uint32_t *)d_hit_t_first, d_hit_offsets);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, ((size_t)total + 1) * sizeof(uint32_t), stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_daq_digitize_gates(chroma_ctx *ctx, uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window,
                              const chroma_daq_trigger *trigger, const chroma_daq_digitizer *digitizer, uint64_t seed, uint32_t acquisition,
                              const uint32_t *d_offsets, const int32_t *d_channel, const uint32_t *d_bin, const uint32_t *d_q_int, uint64_t npulses,
                              const uint32_t *d_trig_offsets, const uint32_t *d_trig_bin, uint64_t ntriggers, const uint32_t *d_hit_offsets,
                              const int32_t *d_hit_channel, uint64_t nhits, uint64_t first_hit, uint64_t nhits_call, uint64_t sample_capacity,
                              uint16_t *d_adc, uint32_t *d_trace_flags)
{
    if (!ctx || !window || !trigger || !digitizer || !d_offsets || !d_trig_offsets || !d_hit_offsets || (npulses && (!d_channel || !d_bin || !d_q_int)) ||
        (ntriggers && !d_trig_bin) || (nhits && !d_hit_channel) || (nhits_call && (!d_adc || !d_trace_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = daq_digitize::check(nrows, nchannels, window, trigger, digitizer, npulses, ntriggers, nhits, first_hit, nhits_call, sample_capacity))
        return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (nhits_call == 0) return CHROMA_OK;
    hipStream_t stream = ctx->stream;
    const CallScope scope(ctx);
    DaqDigitizeView v;
    for (uint32_t j = 0; j < 64u; j++) v.noise_cdf[j] = j < digitizer->nnoise ? digitizer->noise_cdf[j] : 0xffffffffu;
    v.nnoise = digitizer->nnoise; v.noise_lo = digitizer->noise_lo;
    v.ntaps = digitizer->ntaps; v.shift = digitizer->shift; v.pedestal = digitizer->pedestal; v.bits = digitizer->bits;
    int32_t *d_taps = nullptr;          // the block: the taps
    int rc = carve_call_scratch(scope, [&](Carver &c) { d_taps = c.take<int32_t>(digitizer->ntaps); }); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_taps, digitizer->taps, (size_t)digitizer->ntaps * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));          // (the caller's taps are his again when the call returns)
    v.taps = d_taps;
    const uint32_t ntraces = (uint32_t)nhits_call;          // (<= nhits < 2^32)
    hipLaunchKernelGGL(k_daq_digitize, dim3((ntraces - 1u) / DAQ_DIGITIZE_WAVES + 1u), dim3(DAQ_DIGITIZE_BLOCK), 0, stream, v, nrows, nchannels,
                       trigger->pre, trigger->pre + trigger->post, seed, acquisition, d_offsets, d_channel, d_bin, d_q_int, (uint32_t)npulses, d_trig_offsets,
                       d_trig_bin, (uint32_t)ntriggers, d_hit_offsets, d_hit_channel, (uint32_t)first_hit, ntraces, d_adc, d_trace_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

int chroma_daq_reduce_traces(chroma_ctx *ctx, const chroma_daq_reducer *reducer, uint32_t G, uint64_t ntraces, const uint16_t *d_adc,
                             uint64_t found_capacity, uint32_t *d_found_offsets, int32_t *d_trace_base, uint32_t *d_reduced_flags,
                             uint32_t *d_found_start, uint32_t *d_found_width, uint32_t *d_found_peak, uint32_t *d_found_peak_sample,
                             int64_t *d_found_integral, uint32_t *d_found_time, uint32_t *d_found_flags, uint64_t *nfound)
{
    if (!ctx || !reducer || !nfound || (ntraces && (!d_adc || !d_found_offsets || !d_trace_base || !d_reduced_flags)) ||
        (ntraces && found_capacity && (!d_found_start || !d_found_width || !d_found_peak || !d_found_peak_sample || !d_found_integral || !d_found_time || !d_found_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = daq_reduce::check(reducer, G, ntraces)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    *nfound = 0;
    if (ntraces == 0) return CHROMA_OK;
    hipStream_t stream = ctx->stream;
    const CallScope scope(ctx);
    const uint32_t n = (uint32_t)ntraces;          // (< 2^31 - 1)
    size_t scan_bytes = 0;
    int rc = scan_workspace_bytes((size_t)n + 1, stream, &scan_bytes); if (rc) return rc;
    void *d_scan = nullptr;          // the block: the scan's workspace
    rc = carve_call_scratch(scope, [&](Carver &c) { d_scan = c.take<char>(scan_bytes); }); if (rc) return rc;
    // count (a wave per trace, and one for the word behind the counts), scan in place, fill
    hipLaunchKernelGGL(k_daq_reduce_count, dim3(n / DAQ_REDUCE_WAVES + 1u), dim3(DAQ_REDUCE_BLOCK), 0, stream, *reducer, G, n, d_adc, d_found_offsets,
                       d_trace_base, d_reduced_flags);
    HIP_TRY(hipGetLastError());
    rc = exclusive_sum(d_scan, scan_bytes, d_found_offsets, d_found_offsets, (size_t)n + 1, stream); if (rc) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_found_offsets + n, sizeof(total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *nfound = total;
    if (total > found_capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu found pulses, the traces hold %u", (unsigned long long)found_capacity, total);
    if (total) {
        const DaqFoundArrays out{d_found_start, d_found_width, d_found_peak, d_found_peak_sample, d_found_integral, d_found_time, d_found_flags};
        hipLaunchKernelGGL(k_daq_reduce_fill, dim3((n - 1u) / DAQ_REDUCE_WAVES + 1u), dim3(DAQ_REDUCE_BLOCK), 0, stream, *reducer, G, n, d_adc, d_found_offsets, out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return CHROMA_OK;
}

}  // extern "C"
