// kernels_daq.h -- DAQ (chroma/cuda/daq.cu): one acquisition, ndaq side by side, a batch's per-event acquisitions and their compaction.
// One of the kernel families of libchroma_hip.so; included by daq_calls.hip alone, so that each kernel is compiled once.
// (interp_table, which the draws go through, is device_common.h's: k_probe of kernels_render.h calls it too.)
#pragma once

__global__ void k_daq_reset(float maxtime, uint32_t n, uint32_t *time_ints, uint32_t *q_ints, uint32_t *histories)
{
    uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n) {
        time_ints[id] = __float_as_uint(maxtime);
        q_ints[id] = 0u;
        histories[id] = 0u;
    }
}

// run_daq (daq.cu:35-86)
__global__ void k_run_daq(GeoView g, chroma_daq_tables tab, int first_photon, int nphotons, uint32_t detection_state,
                          const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles,
                          const float *weights, uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight,
                          uint32_t *earliest_time_int, uint32_t *channel_q_int, uint32_t *channel_histories)
{
    int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nphotons) return;
    int photon_id = id + first_photon;
    int triangle_id = last_hit_triangles[photon_id];
    if (triangle_id <= -1) return;
    uint32_t history = photon_histories[photon_id];
    int channel_index = g.solid_id_to_channel_index[g.solid_id_map[triangle_id]];
    if (channel_index < 0 || !(history & detection_state)) return;
    cm_rng rng;
    cm_rng_init(&rng, seed, id_base + (uint64_t)photon_id, 0);
    rng.stream = 1u + acquisition;
    float weight = weights[photon_id] * global_weight;
    if (cm_rng_uniform(&rng) < weight) {
        float time = photon_times[photon_id] + interp_table(cm_rng_uniform(&rng), tab.time_cdf_len, tab.d_time_cdf_y, tab.d_time_cdf_x);
        float charge = interp_table(cm_rng_uniform(&rng), tab.charge_cdf_len, tab.d_charge_cdf_y, tab.d_charge_cdf_x);
        uint32_t charge_int = cm_f2u32(cm_roundf(charge / tab.charge_unit));
        atomicMin(earliest_time_int + channel_index, __float_as_uint(time));
        atomicAdd(channel_q_int + channel_index, charge_int);
        atomicOr(channel_histories + channel_index, history);
    }
}

// run_daq_many (daq.cu:88-150): ndaq independent acquisitions of the same photons side by side, copy i
// in channels [i * stride, (i + 1) * stride); a copy adds a unit normal jitter to the hit time.  The
// reference gives a photon a block and its copies the block's threads; here a thread is one (photon,
// copy) pair and copy i draws from words 8 i ... of the photon's DAQ stream, so copies are independent
// and the result does not depend on the launch shape.
__global__ void k_run_daq_many(GeoView g, chroma_daq_tables tab, int first_photon, int nphotons, uint32_t detection_state,
                               const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles,
                               const float *weights, uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight,
                               int ndaq, int channel_stride,
                               uint32_t *earliest_time_int, uint32_t *channel_q_int, uint32_t *channel_histories)
{
    long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)nphotons * ndaq) return;
    int photon_id = (int)(id / ndaq) + first_photon, copy = (int)(id % ndaq);
    int triangle_id = last_hit_triangles[photon_id];
    if (triangle_id <= -1) return;
    uint32_t history = photon_histories[photon_id];
    int channel_index = g.solid_id_to_channel_index[g.solid_id_map[triangle_id]];
    if (channel_index < 0 || !(history & detection_state)) return;
    cm_rng rng;
    cm_rng_init(&rng, seed, id_base + (uint64_t)photon_id, 8u * (uint32_t)copy);
    rng.stream = 1u + acquisition;
    float weight = weights[photon_id] * global_weight;
    int channel_offset = channel_index + copy * channel_stride;
    if (cm_rng_uniform(&rng) < weight) {
        float jitter = cm_rng_normal(&rng);
        float time = photon_times[photon_id] + jitter +
                     interp_table(cm_rng_uniform(&rng), tab.time_cdf_len, tab.d_time_cdf_y, tab.d_time_cdf_x);
        float charge = interp_table(cm_rng_uniform(&rng), tab.charge_cdf_len, tab.d_charge_cdf_y, tab.d_charge_cdf_x);
        uint32_t charge_int = cm_f2u32(cm_roundf(charge / tab.charge_unit));
        atomicMin(earliest_time_int + channel_offset, __float_as_uint(time));
        atomicAdd(channel_q_int + channel_offset, charge_int);
        atomicOr(channel_histories + channel_offset, history);
    }
}

// The per-event acquisitions of a batch as one launch: the events are `nrows + 1` ascending photon bounds (device copy of
// the caller's), row r the photons [bounds[r], bounds[r + 1]) -- empty rows allowed -- and a photon of row r does what
// k_run_daq does for it in the acquisition numbered acquisition + r, into word r * channel_stride + channel.  The grid covers
// [bounds[0], bounds[nrows]); nothing outside it is read.
// the row of photon `id`, given bounds[lo] <= id < bounds[hi]: the one r with bounds[r] <= id < bounds[r + 1]
__device__ inline uint32_t daq_row_of(const uint32_t *bounds, uint32_t lo, uint32_t hi, uint32_t id)
{
    while (hi - lo > 1) {
        const uint32_t half = (lo + hi) / 2;
        if (bounds[half] <= id) lo = half; else hi = half;
    }
    return lo;
}

#define DAQ_EVENTS_BLOCK 256
__global__ __launch_bounds__(DAQ_EVENTS_BLOCK) void
k_run_daq_events(GeoView g, chroma_daq_tables tab, uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                 const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles,
                 const float *weights, uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight,
                 uint32_t channel_stride, uint32_t *earliest_time_int, uint32_t *channel_q_int, uint32_t *channel_histories)
{
    // A block's photons are consecutive: the rows of its first and of its last photon, found once (two lanes, the full
    // range each), bracket the row of every photon of the block -- zero or one step for most, the whole range only when
    // events are single photons.
    __shared__ uint32_t s_row[2];
    const uint32_t end = bounds[nrows];
    const uint32_t block_first = bounds[0] + blockIdx.x * DAQ_EVENTS_BLOCK;          // (< end: the grid is sized so)
    if (threadIdx.x < 2) {
        const uint32_t block_last = min(block_first + (DAQ_EVENTS_BLOCK - 1), end - 1u);
        s_row[threadIdx.x] = daq_row_of(bounds, 0u, nrows, threadIdx.x == 0 ? block_first : block_last);
    }
    __syncthreads();
    const uint32_t photon_id = block_first + threadIdx.x;
    if (photon_id >= end) return;
    int triangle_id = last_hit_triangles[photon_id];
    if (triangle_id <= -1) return;
    uint32_t history = photon_histories[photon_id];
    int channel_index = g.solid_id_to_channel_index[g.solid_id_map[triangle_id]];
    if (channel_index < 0 || !(history & detection_state)) return;
    const uint32_t row = daq_row_of(bounds, s_row[0], s_row[1] + 1u, photon_id);
    cm_rng rng;
    cm_rng_init(&rng, seed, id_base + (uint64_t)photon_id, 0);
    rng.stream = 1u + acquisition + row;
    float weight = weights[photon_id] * global_weight;
    if (cm_rng_uniform(&rng) < weight) {
        float time = photon_times[photon_id] + interp_table(cm_rng_uniform(&rng), tab.time_cdf_len, tab.d_time_cdf_y, tab.d_time_cdf_x);
        float charge = interp_table(cm_rng_uniform(&rng), tab.charge_cdf_len, tab.d_charge_cdf_y, tab.d_charge_cdf_x);
        uint32_t charge_int = cm_f2u32(cm_roundf(charge / tab.charge_unit));
        const uint32_t word = row * channel_stride + (uint32_t)channel_index;
        atomicMin(earliest_time_int + word, __float_as_uint(time));
        atomicAdd(channel_q_int + word, charge_int);
        atomicOr(channel_histories + word, history);
    }
}

// The touched words of nrows rows of nchannels channels (history != 0), compacted in (row, channel) order: a flag per word
// (and a 0 behind the last, which the exclusive sum turns into the total), hipCUB's exclusive sum over them in place, then
// every touched word written to its position.  offsets[r] is the position of row r's first word, offsets[nrows] the total.
__global__ void k_daq_events_flag(uint32_t nwords, uint32_t nchannels, uint32_t channel_stride, const uint32_t *histories, uint32_t *flags)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id > nwords) return;
    uint32_t touched = 0u;
    if (id < nwords) {
        const uint32_t row = id / nchannels;
        touched = histories[row * channel_stride + (id - row * nchannels)] != 0u;
    }
    flags[id] = touched;
}

__global__ void k_daq_events_scatter(uint32_t nwords, uint32_t nchannels, uint32_t channel_stride, float charge_unit,
                                     const uint32_t *time_ints, const uint32_t *q_ints, const uint32_t *histories,
                                     const uint32_t *positions, uint64_t capacity, uint32_t *offsets, int32_t *channel_out,
                                     uint32_t *t_out, float *q_out, uint32_t *flags_out)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id > nwords) return;
    const uint32_t position = positions[id];
    const uint32_t row = id / nchannels, channel = id - row * nchannels;
    if (channel == 0u) offsets[row] = position;                 // (id == nwords: row == nrows, the total)
    if (id == nwords) return;
    const uint32_t word = row * channel_stride + channel;
    const uint32_t history = histories[word];
    if (history == 0u || position >= capacity) return;
    channel_out[position] = (int32_t)channel;
    t_out[position] = time_ints[word];                          // the time bits as they are
    q_out[position] = (float)q_ints[word] * charge_unit;        // as k_daq_convert
    flags_out[position] = history;
}

__global__ void k_daq_convert(uint32_t n, float charge_unit, const uint32_t *time_ints, const uint32_t *q_ints, float *t_out, float *q_out)
{
    uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n) {
        t_out[id] = __uint_as_float(time_ints[id]);
        q_out[id] = (float)q_ints[id] * charge_unit;
    }
}

