// kernels_daq_trigger.h -- the trigger of the time-binned DAQ: a multiplicity (NHIT) or photoelectron (NPE) sum over a sliding
// coincidence window of the pulses chroma_daq_acquire_pulses wrote, a level trigger with lockout on it, and per firing the pulses
// of its readout gate reduced per channel (chroma_daq_trigger_pulses; the contract is in include/chroma_hip.h).  One of the kernel
// families of libchroma_hip.so; included by daq_calls.hip alone, behind kernels_daq_pulses.h (daq_time_image, and
// k_daq_pulses_heads / _open / _finish, which the gated hits reuse as they stand).
//
// The pipeline of a call over npulses pulses of nrows rows:
//   k_daq_trigger_edges   a lane per pulse: its row (a search of the offsets, bracketed per block), and its share of the
//                         differences D[row][bin] of the sum -- NPE: +npe at p, -npe at p + W; NHIT: the intervals [p, p + W) of one
//                         channel united by one look at the entry before, +1 at max(p, p' + W), -1 at p + W.  Lanes of a wave that
//                         follow one another onto one word are reduced first, the last of them adds
//   k_daq_trigger_count   a wave per row, 64 bins at a time: the inclusive scan of D (written back: D becomes the sum S), a ballot of
//                         S >= threshold, the lockout resolved on the mask; the row's number of firings
//   an exclusive sum of those (hipCUB): every row's place among the triggers, in (row, bin) order
//   k_daq_trigger_fire    the same walk over S: the firing bins and their sums, written at the row's place
//   k_daq_trigger_gates   a lane per pulse: the last trigger of its row at or before bin + pre (a binary search), whose gate holds the
//                         pulse or none does (H >= pre + post: the gates of a row do not overlap); a flag per gated pulse
//   an exclusive sum of the flags; k_daq_trigger_compact: the gated pulses as key trigger * nchannels + channel and their index
//   a radix sort of (key, index) over the bits the largest key needs; k_daq_pulses_heads, an exclusive sum, k_daq_pulses_open (as
//   one bin per key); k_daq_trigger_reduce: the pulses of one key reduced within the wave by segment, the last lane of a segment
//   adds the wave's share; k_daq_pulses_finish: the minimum back to float bits, the triggers' offsets among the hits
// Everything is integer sums, ORs and minima: the output does not depend on the order in which they are taken.
#pragma once

#define DAQ_TRIGGER_BLOCK 256
#define DAQ_TRIGGER_WAVES (DAQ_TRIGGER_BLOCK / 64)
#define DAQ_TRIGGER_NONE 0xffffffffu

// The row of pulse i among offsets[lo .. hi + 1]: the last r in [lo, hi] with offsets[r] <= i, if i < offsets[r + 1] (NONE
// otherwise: a pulse the offsets put in no row).  Reads offsets[lo + 1 .. hi + 1] only, whatever they hold.
__device__ inline uint32_t daq_trigger_row_of(const uint32_t *offsets, uint32_t lo, uint32_t hi, uint32_t i)
{
    while (lo < hi) {
        const uint32_t half = lo + (hi - lo + 1u) / 2u;
        if (offsets[half] <= i) lo = half; else hi = half - 1u;
    }
    return (offsets[lo] <= i && i < offsets[lo + 1u]) ? lo : DAQ_TRIGGER_NONE;
}

// value onto D[word] for every lane whose word is not NONE: lanes that follow one another onto one word are summed first.  (The
// words of a wave are not sorted -- the pulses are in channel order, the words in bin order -- so a run is told by its first
// lane, not by equal words: the scan takes from a lane only if that lane is of the same run.)
__device__ inline void daq_trigger_add(uint32_t *D, uint32_t word, uint32_t value, uint32_t lane)
{
    const uint32_t word_before = (uint32_t)__shfl_up((int)word, 1);
    const unsigned long long heads = __ballot(lane == 0u || word_before != word);
    const uint32_t first = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));          // (lane 0 is a head: never 0 bits)
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t value_d = (uint32_t)__shfl_up((int)value, d);
        if (lane >= first + (uint32_t)d) value += value_d;
    }
    const uint32_t word_next = (uint32_t)__shfl_down((int)word, 1);
    if (word != DAQ_TRIGGER_NONE && (lane == 63u || word_next != word) && value) atomicAdd(D + word, value);
}

// D: nrows * nbins words, zeroed by the caller (unsigned, wrapping: a sum S is exact below 2^32).  rows: a word per pulse, its row
// or NONE for a pulse that counts for nothing (no row, a bin beyond the window, a channel outside [0, nchannels)).
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_edges(uint32_t npulses, uint32_t nrows, uint32_t nchannels, uint32_t nbins, uint32_t kind, uint32_t width, const uint32_t *offsets,
                    const int32_t *channel, const uint32_t *bin, const uint32_t *npe, uint32_t *rows, uint32_t *D)
{
    __shared__ uint32_t s_row[2];
    const uint32_t block_first = blockIdx.x * DAQ_TRIGGER_BLOCK;          // (< npulses: the grid is sized so)
    if (threadIdx.x < 2) {
        // the last row that begins at or before the block's first and last pulse (row 0 if none does)
        const uint32_t i = threadIdx.x == 0 ? block_first : min(block_first + (DAQ_TRIGGER_BLOCK - 1), npulses - 1u);
        uint32_t lo = 0u, hi = nrows - 1u;
        while (lo < hi) {
            const uint32_t half = lo + (hi - lo + 1u) / 2u;
            if (offsets[half] <= i) lo = half; else hi = half - 1u;
        }
        s_row[threadIdx.x] = lo;
    }
    __syncthreads();
    const uint32_t i = block_first + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t up = DAQ_TRIGGER_NONE, down = DAQ_TRIGGER_NONE, value = 0u;
    if (i < npulses) {
        const uint32_t lo = min(s_row[0], s_row[1]), hi = max(s_row[0], s_row[1]);          // (ordered, whatever the offsets hold)
        uint32_t row = daq_trigger_row_of(offsets, lo, hi, i);
        const int32_t c = channel[i];
        const uint32_t p = bin[i];
        if (p >= nbins || c < 0 || (uint32_t)c >= nchannels) row = DAQ_TRIGGER_NONE;
        rows[i] = row;
        if (row != DAQ_TRIGGER_NONE) {
            uint32_t from = p;
            value = 1u;
            if (kind == CHROMA_TRIGGER_NPE) value = npe[i];
            else if (i > offsets[row] && channel[i - 1u] == c && bin[i - 1u] < nbins) from = max(p, bin[i - 1u] + width);
            const uint32_t to = p + width;          // (bins and widths of 17 bits at the most)
            if (from < to) {
                const uint32_t base = row * nbins;
                if (from < nbins) up = base + from;
                if (to < nbins) down = base + to;
            }
        }
    }
    daq_trigger_add(D, up, value, lane);
    daq_trigger_add(D, down, 0u - value, lane);
}

// The walk of one row by one wave.  FIRE false: D holds the differences; their inclusive scan S is written back over them and
// the firings are counted (the return value, wave-uniform).  FIRE true: D holds S; firing k of the row goes to bin_out[k] and
// sum_out[k].
template <bool FIRE>
__device__ inline uint32_t daq_trigger_walk(uint32_t nbins, uint32_t threshold, uint32_t holdoff, uint32_t *S, uint32_t lane, uint32_t *bin_out,
                                            uint32_t *sum_out)
{
    uint32_t carry = 0u, next = 0u, fired = 0u;
    for (uint32_t first = 0u; first < nbins; first += 64u) {
        const uint32_t b = first + lane;
        uint32_t s = b < nbins ? S[b] : 0u;
        if (!FIRE) {
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t s_d = (uint32_t)__shfl_up((int)s, d);
                if (lane >= (uint32_t)d) s += s_d;
            }
            s += carry;
            carry = (uint32_t)__shfl((int)s, 63);
            if (b < nbins) S[b] = s;
        }
        unsigned long long mask = __ballot(b < nbins && s >= threshold);
        // the lockout, on the mask: the bins before `next` do not fire, the lowest bin left does and moves `next` on
        while (mask) {
            if (next > first) {
                const uint32_t skip = next - first;
                mask = skip >= 64u ? 0ull : mask & ~((1ull << skip) - 1ull);
                if (!mask) break;
            }
            const uint32_t at = (uint32_t)__ffsll((long long)mask) - 1u;
            if (FIRE && lane == at) { bin_out[fired] = b; sum_out[fired] = s; }
            fired++;
            next = first + at + holdoff;          // (holdoff >= 1: the bin itself is behind the lockout)
        }
    }
    return fired;
}

// counts: nrows + 1 words, the last 0 (the exclusive sum turns it into the number of triggers)
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_count(uint32_t nrows, uint32_t nbins, uint32_t threshold, uint32_t holdoff, uint32_t *D, uint32_t *counts)
{
    const uint32_t row = blockIdx.x * DAQ_TRIGGER_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (row > nrows) return;          // (whole waves)
    if (row == nrows) { if (lane == 0u) counts[row] = 0u; return; }
    const uint32_t fired = daq_trigger_walk<false>(nbins, threshold, holdoff, D + (size_t)row * nbins, lane, nullptr, nullptr);
    if (lane == 0u) counts[row] = fired;
}

// room: the entries of trig_bin and trig_sum (the count's total, so every place is below it; a row that would pass it is left out)
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_fire(uint32_t nrows, uint32_t nbins, uint32_t threshold, uint32_t holdoff, uint32_t *S, const uint32_t *trig_offsets, uint32_t room,
                   uint32_t *trig_bin, uint32_t *trig_sum)
{
    const uint32_t row = blockIdx.x * DAQ_TRIGGER_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (row >= nrows) return;
    const uint32_t from = trig_offsets[row], to = trig_offsets[row + 1u];
    if (from >= to || to > room) return;
    daq_trigger_walk<true>(nbins, threshold, holdoff, S + (size_t)row * nbins, lane, trig_bin + from, trig_sum + from);
}

// pulse_trigger[i]: the trigger whose gate [b - pre, b + post) holds pulse i, or NONE; gated[i]: 1 or 0, gated[npulses] = 0
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_gates(uint32_t npulses, uint32_t pre, uint32_t post, const uint32_t *rows, const uint32_t *bin, const uint32_t *trig_offsets,
                    const uint32_t *trig_bin, uint32_t *pulse_trigger, uint32_t *gated)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > npulses) return;
    uint32_t trigger = DAQ_TRIGGER_NONE;
    const uint32_t row = i < npulses ? rows[i] : DAQ_TRIGGER_NONE;
    if (row != DAQ_TRIGGER_NONE) {
        const uint32_t p = bin[i], first = trig_offsets[row];
        uint32_t lo = first, hi = trig_offsets[row + 1u];          // the first trigger of [lo, hi) whose bin is beyond p + pre
        while (lo < hi) {
            const uint32_t half = lo + (hi - lo) / 2u;
            if (trig_bin[half] <= p + pre) lo = half + 1u; else hi = half;
        }
        if (lo > first && p < trig_bin[lo - 1u] + post) trigger = lo - 1u;
    }
    if (i < npulses) pulse_trigger[i] = trigger;
    gated[i] = trigger != DAQ_TRIGGER_NONE ? 1u : 0u;
}

// positions: the exclusive sum of the gated flags
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_compact(uint32_t npulses, uint32_t nchannels, const uint32_t *pulse_trigger, const int32_t *channel, const uint32_t *positions,
                      uint32_t room, uint64_t *keys, uint32_t *order)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npulses) return;
    const uint32_t trigger = pulse_trigger[i], position = positions[i];
    if (trigger == DAQ_TRIGGER_NONE || position >= room) return;
    keys[position] = (uint64_t)trigger * nchannels + (uint32_t)channel[i];
    order[position] = i;
}

// k_daq_pulses_reduce over pulses in place of photons: what a gated pulse brings is its own npe, charge count, time and flags
__global__ __launch_bounds__(DAQ_TRIGGER_BLOCK) void
k_daq_trigger_reduce(uint32_t n, const uint64_t *keys, const uint32_t *positions, const uint32_t *order, const uint32_t *npe_in,
                     const uint32_t *q_in, const uint32_t *t_in, const uint32_t *flags_in, uint32_t *npe_out, uint32_t *q_out, uint32_t *t_out,
                     uint32_t *flags_out)
{
    const uint32_t i = blockIdx.x * DAQ_TRIGGER_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    uint32_t hit = 0xffffffffu, npe = 0u, q = 0u, t = 0xffffffffu, flags = 0u;
    if (live) {
        hit = daq_pulse_of(keys, positions, i);
        const uint32_t from = order[i];
        npe = npe_in[from];
        q = q_in[from];
        t = daq_time_image(t_in[from]);
        flags = flags_in[from];
    }
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t hit_d = (uint32_t)__shfl_up((int)hit, d);
        const uint32_t npe_d = (uint32_t)__shfl_up((int)npe, d), q_d = (uint32_t)__shfl_up((int)q, d);
        const uint32_t t_d = (uint32_t)__shfl_up((int)t, d), flags_d = (uint32_t)__shfl_up((int)flags, d);
        if (lane >= (uint32_t)d && hit_d == hit) {
            npe += npe_d;
            q += q_d;
            t = min(t, t_d);
            flags |= flags_d;
        }
    }
    const uint32_t hit_next = (uint32_t)__shfl_down((int)hit, 1);
    if (live && (lane == 63u || hit_next != hit)) {
        atomicAdd(npe_out + hit, npe);
        atomicAdd(q_out + hit, q);
        atomicMin(t_out + hit, t);
        atomicOr(flags_out + hit, flags);
    }
}
