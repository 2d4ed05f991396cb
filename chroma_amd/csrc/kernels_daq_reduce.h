// kernels_daq_reduce.h -- the trace reduction of the time-binned DAQ: the pulses found in the traces chroma_daq_digitize_gates left
// on the device, with their charge and their constant-fraction time (chroma_daq_reduce_traces; the contract is in
// include/chroma_hip.h, the arithmetic of one trace and one pulse in daq_reduce_common.h).  One of the kernel families of
// libchroma_hip.so; included by daq_calls.hip alone.
//
// A wave per trace, four traces per block, no LDS.  Lanes take 64 consecutive samples a round (16-bit, lane-consecutive loads);
// the baseline is the first round's leading lanes, summed across the wave.  A ballot of y >= T gives the round's samples above
// threshold as a 64-bit mask, and the runs are walked in wave-uniform bit arithmetic: the first set bit at or behind a cursor opens
// a run, the first clear one closes it, and a run that is open at the end of a round stays open in scalar registers -- run 65 of a
// trace is no different from run 1.  Samples behind the trace's end are clear bits, and a trace whose length is a multiple of 64
// gets one more round of them, so every run closes inside the loop.  The count pass (FILL = false) counts the runs that are long
// enough and writes the trace's base and flag word.  The fill pass walks the same way and keeps one pulse pending: its window ends
// where the next pulse begins, so it is emitted when that is known or the trace ends.  Emitting takes the whole wave over the
// pulse's window (windows are disjoint: a trace is read twice at the most, from cache): lane-strided sums and a running (peak,
// first sample) per lane, gathered across the wave; then 64 samples at a time downwards from the peak, the highest lane below the
// constant-fraction level by ballot.  Lane 0 stores the pulse.
#pragma once

#include "daq_reduce_common.h"

#define DAQ_REDUCE_BLOCK 256
#define DAQ_REDUCE_WAVES (DAQ_REDUCE_BLOCK / 64)

// the per-pulse arrays of chroma_daq_reduce_traces
struct DaqFoundArrays {
    uint32_t *start, *width, *peak, *peak_sample;
    int64_t *integral;
    uint32_t *time, *flags;
};

// across the wave (every lane gets the result)
__device__ __forceinline__ uint32_t daq_reduce_sum(uint32_t x) { for (int d = 32; d; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d); return x; }
__device__ __forceinline__ uint32_t daq_reduce_min(uint32_t x) { for (int d = 32; d; d >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, d)); return x; }
__device__ __forceinline__ uint32_t daq_reduce_max(uint32_t x) { for (int d = 32; d; d >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, d)); return x; }
__device__ __forceinline__ int32_t daq_reduce_max(int32_t x) { for (int d = 32; d; d >>= 1) x = max(x, __shfl_xor(x, d)); return x; }
__device__ __forceinline__ int64_t daq_reduce_sum(int64_t x)
{
    for (int d = 32; d; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)x >> 32), d);
        x += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return x;
}

// The pulse [a, e) of the trace `v`, whose window ends at the start `a_next` of the pulse behind it (G: none) and begins at
// `*stop_before`, the end of the window before it, at the earliest: stored at `at` by lane 0.  Wave-uniform arguments.
__device__ __forceinline__ void daq_reduce_emit(const chroma_daq_reducer &r, const daq_reduce::Level &l, uint32_t G, const uint16_t *v, uint32_t lane,
                                                uint32_t a, uint32_t e, uint32_t a_next, uint32_t *stop_before, const DaqFoundArrays &out, uint32_t at)
{
    const uint32_t stop = daq_reduce::window_stop(r, e, a_next, G), begin = daq_reduce::window_begin(r, a, *stop_before);
    *stop_before = stop;
    int64_t sum = 0;
    int32_t best = INT32_MIN;
    uint32_t best_s = 0xffffffffu;
    for (uint32_t c = begin; c < stop; c += 64u) {          // (begin <= a < e <= stop)
        const uint32_t s = c + lane;
        if (s < stop) {
            const int32_t y = daq_reduce::y_of(r, l, v[s]);
            sum += y;
            if (s >= a && s < e && y > best) { best = y; best_s = s; }          // (a lane's samples ascend: its first one at its best)
        }
    }
    const int32_t top = daq_reduce_max(best);          // (>= T >= 1)
    const uint32_t peak_sample = (uint32_t)__builtin_amdgcn_readfirstlane((int)daq_reduce_min(best == top ? best_s : 0xffffffffu));
    const uint32_t peak = (uint32_t)__builtin_amdgcn_readfirstlane(top);
    const int64_t integral = daq_reduce_sum(sum);
    const int32_t L = daq_reduce::cfd_level(r, peak);
    // s_c: behind the last sample of [begin, peak_sample] below L, or begin
    uint32_t s_c = begin;
    for (int32_t hi = (int32_t)peak_sample;; hi -= 64) {
        const int32_t s = hi - 63 + (int32_t)lane;
        const bool below = s >= (int32_t)begin && daq_reduce::y_of(r, l, v[s]) < L;
        const uint64_t mask = __ballot(below);
        if (mask) { s_c = (uint32_t)(hi - (int32_t)__clzll((long long)mask)) + 1u; break; }
        if (hi - 63 <= (int32_t)begin) break;
    }
    const uint32_t before = s_c ? s_c - 1u : 0u;
    const int32_t y0 = daq_reduce::y_of(r, l, v[before]), y1 = daq_reduce::y_of(r, l, v[s_c]);
    const bool at_edge = s_c == begin && (begin == 0u || y0 >= L);
    if (lane == 0u) {
        out.start[at] = a; out.width[at] = e - a; out.peak[at] = peak; out.peak_sample[at] = peak_sample;
        out.integral[at] = integral;
        out.time[at] = at_edge ? 256u * s_c : daq_reduce::cfd_time(s_c, L, y0, y1);
        out.flags[at] = (at_edge ? daq_reduce::TIME_AT_EDGE : 0u) | (a == 0u ? daq_reduce::OPEN_AT_START : 0u) | (e == G ? daq_reduce::OPEN_AT_END : 0u);
    }
}

// The walk of one trace by one wave.  FILL = false: counts[trace] = its pulses (counts[ntraces] = 0, for the scan), its base and
// its flag word.  FILL = true: its pulses from offsets[trace] on.
template <bool FILL>
__device__ __forceinline__ void daq_reduce_trace(const chroma_daq_reducer &r, uint32_t G, uint32_t ntraces, const uint16_t *adc, uint32_t *offsets,
                                                 int32_t *trace_base, uint32_t *reduced_flags, const DaqFoundArrays &out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t trace = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * DAQ_REDUCE_WAVES + (threadIdx.x >> 6)));
    if (!FILL && trace == ntraces && lane == 0u) offsets[ntraces] = 0u;
    if (trace >= ntraces) return;          // (whole waves)
    const uint16_t *v = adc + (size_t)trace * G;
    uint32_t sum = 0u;
    if (r.nbaseline) {
        const bool mine = lane < r.nbaseline;          // (nbaseline <= 64 and <= G)
        const uint32_t x = mine ? v[lane] : 0u;
        sum = daq_reduce_sum(x);
        if (!FILL) {
            const uint32_t lowest = daq_reduce_min(mine ? x : 0xffffffffu), highest = daq_reduce_max(x);
            if (lane == 0u) reduced_flags[trace] = daq_reduce::trace_flags(r, lowest, highest);
        }
    } else if (!FILL && lane == 0u) {
        reduced_flags[trace] = 0u;
    }
    daq_reduce::Level l = daq_reduce::level(r, sum);
    l.base = __builtin_amdgcn_readfirstlane(l.base);
    if (!FILL && lane == 0u) trace_base[trace] = l.base;
    uint32_t n = 0u, a_open = 0u, pending_a = 0u, pending_e = 0u, stop_before = 0u;
    bool open = false, pending = false;
    const uint32_t first = FILL ? offsets[trace] : 0u;
    for (uint32_t s0 = 0u; s0 <= G; s0 += 64u) {          // (s0 == G: a round of nothing, which closes a run that is open at the end)
        const uint32_t s = s0 + lane;
        const uint64_t mask = __ballot(s < G && daq_reduce::y_of(r, l, v[s < G ? s : 0u]) >= l.T);
        for (uint32_t cur = 0u;;) {
            const uint64_t left = (open ? ~mask : mask) & (~0ull << cur);
            if (!left) break;
            cur = (uint32_t)__ffsll((long long)left) - 1u;
            open = !open;
            if (open) { a_open = s0 + cur; continue; }
            const uint32_t e = s0 + cur;
            if (e - a_open < r.min_width) continue;          // (its samples are ordinary samples)
            if (FILL) {
                if (pending) daq_reduce_emit(r, l, G, v, lane, pending_a, pending_e, a_open, &stop_before, out, first + n - 1u);
                pending = true; pending_a = a_open; pending_e = e;
            }
            n++;
        }
    }
    if (FILL) {
        if (pending) daq_reduce_emit(r, l, G, v, lane, pending_a, pending_e, G, &stop_before, out, first + n - 1u);
    } else if (lane == 0u) {
        offsets[trace] = n;
    }
}

__global__ __launch_bounds__(DAQ_REDUCE_BLOCK) void
k_daq_reduce_count(chroma_daq_reducer r, uint32_t G, uint32_t ntraces, const uint16_t *adc, uint32_t *counts, int32_t *trace_base, uint32_t *reduced_flags)
{
    daq_reduce_trace<false>(r, G, ntraces, adc, counts, trace_base, reduced_flags, DaqFoundArrays{});
}

__global__ __launch_bounds__(DAQ_REDUCE_BLOCK) void
k_daq_reduce_fill(chroma_daq_reducer r, uint32_t G, uint32_t ntraces, const uint16_t *adc, uint32_t *offsets, DaqFoundArrays out)
{
    daq_reduce_trace<true>(r, G, ntraces, adc, offsets, nullptr, nullptr, out);
}
