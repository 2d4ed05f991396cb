// kernels_daq_pulses.h -- the time-binned DAQ: per (event, channel, time bin) the pulses of the photoelectrons that k_run_daq_events
// accumulates per (event, channel), kept sparse (chroma_daq_count_pulses / chroma_daq_acquire_pulses; the contract is in
// include/chroma_hip.h).  One of the kernel families of libchroma_hip.so; included by daq_calls.hip alone, behind
// kernels_daq.h (daq_row_of; interp_table is device_common.h's).
//
// The pipeline of an acquisition of n accepted in-window photons:
//   k_daq_pulses_emit     a lane per photon of the window: gate, time, charge and bin as k_run_daq_events draws them; the accepted
//                         in-window photons compacted (ballots, and ONE add per block of 1024 photons) as a 64-bit key
//                         (row * nchannels + channel) * nbins + bin and (charge count, time bits, history); early and late
//                         photons counted per row, one add per block, or per (wave, row) where rows change within the block
//   a radix sort of (key, position) over the bits the largest key needs (hipCUB)
//   k_daq_pulses_heads    a flag per sorted photon: the first of its key (and a 0 behind the last, which the exclusive sum turns
//                         into the number of pulses); hipCUB's exclusive sum over them in place
//   k_daq_pulses_open     the first photon of every key writes its pulse's channel and bin and the neutral elements of the sums
//   k_daq_pulses_reduce   a lane per sorted photon: the photons of one key are reduced within the wave by segment, and the last
//                         lane of a segment adds the wave's share to the pulse -- integer add, or and (on the order-preserving
//                         image of the time's bits) min, so a key that runs over many waves costs one set of atomics per wave
//   k_daq_pulses_finish   a lane per pulse: the minimum back to float bits; a lane per row: its offset, the lower bound of the
//                         row's first key among the sorted keys
// Sums and ORs of integers and the minimum do not depend on the order in which they are taken: the output is deterministic.
#pragma once

#define DAQ_PULSES_BLOCK 256

// the order-preserving image of a float's bits (a < b as floats <=> image(a) < image(b) as unsigned; -0 ranks below +0) and back
__device__ inline uint32_t daq_time_image(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ inline uint32_t daq_time_bits(uint32_t image) { return (image & 0x80000000u) ? (image & 0x7fffffffu) : ~image; }

// what becomes of one photon of the window
enum { DAQ_PULSE_NONE = 0, DAQ_PULSE_IN = 1, DAQ_PULSE_EARLY = 2, DAQ_PULSE_LATE = 3 };
struct DaqPulsePhoton { uint32_t row, channel, bin, charge_int, time_bits, history; };

// The photon `photon_id` as k_run_daq_events treats it -- the same rejects, the same three draws in the same order -- and its
// place in the window.  bounds[row_lo] <= photon_id < bounds[row_hi].
__device__ inline int daq_pulse_photon(const GeoView &g, const chroma_daq_tables &tab, const chroma_daq_window &win, const uint32_t *bounds,
                                       uint32_t row_lo, uint32_t row_hi, uint32_t photon_id, uint32_t detection_state,
                                       const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles,
                                       const float *weights, uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight,
                                       DaqPulsePhoton &out)
{
    const int triangle_id = last_hit_triangles[photon_id];
    if (triangle_id <= -1) return DAQ_PULSE_NONE;
    const uint32_t history = photon_histories[photon_id];
    const int channel_index = g.solid_id_to_channel_index[g.solid_id_map[triangle_id]];
    if (channel_index < 0 || !(history & detection_state)) return DAQ_PULSE_NONE;
    out.row = daq_row_of(bounds, row_lo, row_hi, photon_id);
    cm_rng rng;
    cm_rng_init(&rng, seed, id_base + (uint64_t)photon_id, 0);
    rng.stream = 1u + acquisition + out.row;
    const float weight = weights[photon_id] * global_weight;
    if (!(cm_rng_uniform(&rng) < weight)) return DAQ_PULSE_NONE;
    const float time = photon_times[photon_id] + interp_table(cm_rng_uniform(&rng), tab.time_cdf_len, tab.d_time_cdf_y, tab.d_time_cdf_x);
    const float charge = interp_table(cm_rng_uniform(&rng), tab.charge_cdf_len, tab.d_charge_cdf_y, tab.d_charge_cdf_x);
    out.channel = (uint32_t)channel_index;
    out.charge_int = cm_f2u32(cm_roundf(charge / tab.charge_unit));
    out.time_bits = __float_as_uint(time);
    out.history = history;
    const float x = (time - win.t0) / win.dt;
    if (x >= 0.0f && x < (float)win.nbins) {
        out.bin = (uint32_t)cm_floorf(x);
        return DAQ_PULSE_IN;
    }
    return time < win.t0 ? DAQ_PULSE_EARLY : DAQ_PULSE_LATE;          // (a NaN time: late)
}

// A block takes DAQ_PULSES_ITEMS runs of DAQ_PULSES_BLOCK consecutive photons, lane t the photon t of each run, and adds what it
// found to a shared word ONCE: the accepted photons of a batch are a few per wave, and one add per wave onto one word is what
// the walk of the photons then waits for.
#define DAQ_PULSES_ITEMS 4
#define DAQ_PULSES_SPAN (DAQ_PULSES_BLOCK * DAQ_PULSES_ITEMS)
#define DAQ_PULSES_WAVES (DAQ_PULSES_BLOCK / 64)

// the rows that bracket a block's photons, as in k_run_daq_events
__device__ inline void daq_pulses_block_rows(uint32_t nrows, const uint32_t *bounds, uint32_t block_first, uint32_t end, uint32_t *s_row)
{
    if (threadIdx.x < 2) {
        const uint32_t block_last = min(block_first + (DAQ_PULSES_SPAN - 1), end - 1u);
        s_row[threadIdx.x] = daq_row_of(bounds, 0u, nrows, threadIdx.x == 0 ? block_first : block_last);
    }
    __syncthreads();
}

// chroma_daq_count_pulses: the accepted in-window photons of the window, one add per block
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) void
k_daq_pulses_count(GeoView g, chroma_daq_tables tab, chroma_daq_window win, uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                   const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles, const float *weights,
                   uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight, uint32_t *naccepted)
{
    __shared__ uint32_t s_row[2], s_count[DAQ_PULSES_WAVES];
    const uint32_t end = bounds[nrows];
    const uint32_t block_first = bounds[0] + blockIdx.x * DAQ_PULSES_SPAN;          // (< end: the grid is sized so)
    daq_pulses_block_rows(nrows, bounds, block_first, end, s_row);
    uint32_t count = 0u;          // (of the wave)
#pragma unroll
    for (int k = 0; k < DAQ_PULSES_ITEMS; k++) {
        const uint32_t photon_id = block_first + k * DAQ_PULSES_BLOCK + threadIdx.x;
        DaqPulsePhoton p;
        int what = DAQ_PULSE_NONE;
        if (photon_id < end)
            what = daq_pulse_photon(g, tab, win, bounds, s_row[0], s_row[1] + 1u, photon_id, detection_state, photon_times, photon_histories,
                                    last_hit_triangles, weights, seed, id_base, acquisition, global_weight, p);
        count += (uint32_t)__popcll(__ballot(what == DAQ_PULSE_IN));
    }
    if ((threadIdx.x & 63u) == 0u) s_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (int w = 0; w < DAQ_PULSES_WAVES; w++) total += s_count[w];
        if (total) atomicAdd(naccepted, total);
    }
}

// The emit.  `room`: the entries of keys, order, charge_ints, time_bits and histories (the count of k_daq_pulses_count for the same
// arguments, so every position is below it; checked all the same).  outside: 2 * nrows words, zeroed by the caller.
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void          // (its four runs unrolled: held to the scalar registers of 8 waves)
k_daq_pulses_emit(GeoView g, chroma_daq_tables tab, chroma_daq_window win, uint32_t nrows, const uint32_t *bounds, uint32_t detection_state,
                  const float *photon_times, const uint32_t *photon_histories, const int32_t *last_hit_triangles, const float *weights,
                  uint64_t seed, uint64_t id_base, uint32_t acquisition, float global_weight, uint32_t room, uint32_t *cursor,
                  uint64_t *keys, uint32_t *order, uint32_t *charge_ints, uint32_t *time_bits, uint32_t *histories, uint32_t *outside)
{
    __shared__ uint32_t s_row[2], s_count[DAQ_PULSES_WAVES], s_early[DAQ_PULSES_WAVES], s_late[DAQ_PULSES_WAVES], s_base;
    const uint32_t end = bounds[nrows];
    const uint32_t block_first = bounds[0] + blockIdx.x * DAQ_PULSES_SPAN;          // (< end: the grid is sized so)
    daq_pulses_block_rows(nrows, bounds, block_first, end, s_row);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool one_row = s_row[0] == s_row[1];          // the block's photons are all of one row: its early and late photons in one add each
    DaqPulsePhoton p[DAQ_PULSES_ITEMS];
    int what[DAQ_PULSES_ITEMS];
    uint32_t count = 0u, nearly = 0u, nlate = 0u;          // (of the wave)
#pragma unroll
    for (int k = 0; k < DAQ_PULSES_ITEMS; k++) {
        const uint32_t photon_id = block_first + k * DAQ_PULSES_BLOCK + threadIdx.x;
        p[k].row = 0u;
        what[k] = DAQ_PULSE_NONE;
        if (photon_id < end)
            what[k] = daq_pulse_photon(g, tab, win, bounds, s_row[0], s_row[1] + 1u, photon_id, detection_state, photon_times, photon_histories,
                                       last_hit_triangles, weights, seed, id_base, acquisition, global_weight, p[k]);
        count += (uint32_t)__popcll(__ballot(what[k] == DAQ_PULSE_IN));
        // early and late per row
        unsigned long long left = __ballot(what[k] >= DAQ_PULSE_EARLY);
        if (left) {
            const unsigned long long early = __ballot(what[k] == DAQ_PULSE_EARLY), late = __ballot(what[k] == DAQ_PULSE_LATE);
            if (one_row) {
                nearly += (uint32_t)__popcll(early);
                nlate += (uint32_t)__popcll(late);
                left = 0ull;
            }
            // (rows change within the block: the wave's photons of one row counted by a ballot, one add per (wave, row) that has any)
            while (left) {
                const int leader = __ffsll((long long)left) - 1;
                const uint32_t row = (uint32_t)__shfl((int)p[k].row, leader);
                const unsigned long long same = __ballot(what[k] >= DAQ_PULSE_EARLY && p[k].row == row);
                if (lane == (uint32_t)leader) {
                    const uint32_t e = (uint32_t)__popcll(early & same), l = (uint32_t)__popcll(late & same);
                    if (e) atomicAdd(outside + 2u * (size_t)row, e);
                    if (l) atomicAdd(outside + 2u * (size_t)row + 1u, l);
                }
                left &= ~same;
            }
        }
    }
    if (lane == 0u) { s_count[wave] = count; s_early[wave] = nearly; s_late[wave] = nlate; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u, e = 0u, l = 0u;
        for (int w = 0; w < DAQ_PULSES_WAVES; w++) { total += s_count[w]; e += s_early[w]; l += s_late[w]; }
        s_base = total ? atomicAdd(cursor, total) : 0u;
        if (e) atomicAdd(outside + 2u * (size_t)s_row[0], e);
        if (l) atomicAdd(outside + 2u * (size_t)s_row[0] + 1u, l);
    }
    __syncthreads();
    // the accepted in-window photons of the block behind one another from that one add: wave by wave, run by run, lane by lane
    uint32_t base = s_base;
    for (uint32_t w = 0; w < wave; w++) base += s_count[w];
#pragma unroll
    for (int k = 0; k < DAQ_PULSES_ITEMS; k++) {
        const unsigned long long in = __ballot(what[k] == DAQ_PULSE_IN);
        const uint32_t position = base + (uint32_t)__popcll(in & ((1ull << lane) - 1ull));
        if (what[k] == DAQ_PULSE_IN && position < room) {
            keys[position] = ((uint64_t)p[k].row * g.nchannels + p[k].channel) * win.nbins + p[k].bin;
            order[position] = position;
            charge_ints[position] = p[k].charge_int;
            time_bits[position] = p[k].time_bits;
            histories[position] = p[k].history;
        }
        base += (uint32_t)__popcll(in);
    }
}

// heads[i] = 1 where sorted photon i is the first of its key, heads[n] = 0
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) void
k_daq_pulses_heads(uint32_t n, const uint64_t *keys, uint32_t *heads)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    heads[i] = (i < n && (i == 0u || keys[i] != keys[i - 1u])) ? 1u : 0u;
}

// the pulse of sorted photon i, from the exclusive sum of the heads: the heads before it, itself included, less one
__device__ inline uint32_t daq_pulse_of(const uint64_t *keys, const uint32_t *positions, uint32_t i)
{
    return positions[i] - ((i == 0u || keys[i] != keys[i - 1u]) ? 0u : 1u);
}

__global__ __launch_bounds__(DAQ_PULSES_BLOCK) void
k_daq_pulses_open(uint32_t n, uint32_t nchannels, uint32_t nbins, const uint64_t *keys, const uint32_t *positions,
                                  int32_t *channel_out, uint32_t *bin_out, uint32_t *npe_out, uint32_t *q_out, uint32_t *t_out,
                                  uint32_t *flags_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (i != 0u && key == keys[i - 1u]) return;
    const uint32_t pulse = positions[i];
    const uint64_t word = key / nbins;
    channel_out[pulse] = (int32_t)(word % nchannels);
    bin_out[pulse] = (uint32_t)(key - word * nbins);
    npe_out[pulse] = 0u;
    q_out[pulse] = 0u;
    t_out[pulse] = 0xffffffffu;          // (above the image of every time)
    flags_out[pulse] = 0u;
}

__global__ __launch_bounds__(DAQ_PULSES_BLOCK) void
k_daq_pulses_reduce(uint32_t n, const uint64_t *keys, const uint32_t *positions, const uint32_t *order, const uint32_t *charge_ints,
                    const uint32_t *time_bits, const uint32_t *histories, uint32_t *npe_out, uint32_t *q_out, uint32_t *t_out,
                    uint32_t *flags_out)
{
    const uint32_t i = blockIdx.x * DAQ_PULSES_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    // (a lane behind the last photon: a pulse of its own that is never written)
    uint32_t pulse = 0xffffffffu, npe = 0u, q = 0u, t = 0xffffffffu, flags = 0u;
    if (live) {
        pulse = daq_pulse_of(keys, positions, i);
        const uint32_t from = order[i];
        npe = 1u;
        q = charge_ints[from];
        t = daq_time_image(time_bits[from]);
        flags = histories[from];
    }
    // the inclusive scan by segment: after it the last lane of a segment holds the segment's photons of this wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t pulse_d = (uint32_t)__shfl_up((int)pulse, d);
        const uint32_t npe_d = (uint32_t)__shfl_up((int)npe, d), q_d = (uint32_t)__shfl_up((int)q, d);
        const uint32_t t_d = (uint32_t)__shfl_up((int)t, d), flags_d = (uint32_t)__shfl_up((int)flags, d);
        if (lane >= (uint32_t)d && pulse_d == pulse) {
            npe += npe_d;
            q += q_d;
            t = min(t, t_d);
            flags |= flags_d;
        }
    }
    const uint32_t pulse_next = (uint32_t)__shfl_down((int)pulse, 1);
    if (live && (lane == 63u || pulse_next != pulse)) {
        atomicAdd(npe_out + pulse, npe);
        atomicAdd(q_out + pulse, q);
        atomicMin(t_out + pulse, t);
        atomicOr(flags_out + pulse, flags);
    }
}

// t_first back to float bits (a lane per pulse) and the rows' offsets (a lane per row and one for the total): offsets[r] is
// the pulse of the first sorted photon whose key is not below row r's first key, positions[n] for none
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) void
k_daq_pulses_finish(uint32_t n, uint32_t npulses, uint32_t nrows, uint64_t keys_per_row, const uint64_t *keys,
                                    const uint32_t *positions, uint32_t *t_out, uint32_t *offsets)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < npulses) t_out[id] = daq_time_bits(t_out[id]);
    if (id <= nrows) {
        const uint64_t first_key = (uint64_t)id * keys_per_row;
        uint32_t lo = 0u, hi = n;                                   // the first i in [0, n] with keys[i] >= first_key
        while (lo < hi) {
            const uint32_t half = lo + (hi - lo) / 2u;
            if (keys[half] < first_key) lo = half + 1u; else hi = half;
        }
        offsets[id] = positions[lo];          // (positions[lo] counts the heads before lo: lo is a head, or n)
    }
}
