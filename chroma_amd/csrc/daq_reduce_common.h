// daq_reduce_common.h -- the trace reduction of the time-binned DAQ: the arithmetic of ONE trace and of ONE found pulse, written
// once for the device kernels (kernels_daq_reduce.h) and for the host loop (daq_reduce_host.cpp).  The contract is in
// include/chroma_hip.h ("trace reduction").  Everything is integer: sums of int32 values below 2^22 in 64 bits, compares and one
// unsigned 32-bit floor division, so the two sides produce the same bits whatever the order of the sums.
#pragma once

#include <stdint.h>

#include "daq_noise_common.h"          // (DAQ_NOISE_FN, and the public header)

namespace daq_reduce {

constexpr uint32_t MAX_SAMPLES = 65536u;          // the samples of a trace
constexpr uint32_t MAX_BASELINE = 64u;            // the samples a baseline is measured over: one round of a wave
constexpr uint32_t TIME_AT_EDGE = 1u, OPEN_AT_START = 2u, OPEN_AT_END = 4u;          // the bits of a found pulse's flag word
constexpr uint32_t BASELINE_BUSY = 1u;            // the bit of a trace's flag word

// What a trace's samples are measured against: N = max(nbaseline, 1), base = the sum of the baseline samples (or the pedestal),
// T = N * threshold
struct Level { int32_t N, base, T; };

DAQ_NOISE_FN Level level(const chroma_daq_reducer &r, uint32_t baseline_sum)
{
    Level l;
    l.N = (int32_t)(r.nbaseline ? r.nbaseline : 1u);
    l.base = (int32_t)(r.nbaseline ? baseline_sum : r.pedestal);
    l.T = l.N * (int32_t)r.threshold;
    return l;
}

// y(s) of the sample v: |y| < 2^22 (N <= 64, v < 2^16, base <= 64 * 65535)
DAQ_NOISE_FN int32_t y_of(const chroma_daq_reducer &r, const Level &l, uint16_t v) { return r.polarity * (l.N * (int32_t)v - l.base); }

// the trace's flag word from the smallest and the largest baseline sample (nbaseline > 0)
DAQ_NOISE_FN uint32_t trace_flags(const chroma_daq_reducer &r, uint32_t lowest, uint32_t highest)
{
    return (r.nbaseline && highest - lowest > r.baseline_spread) ? BASELINE_BUSY : 0u;
}

// The integration window [begin, stop) of the pulse [a, e): `stop_before` is the stop of the pulse before it (0 for the first),
// `a_next` the start of the pulse behind it (G for the last).  64-bit sums: lead and lag reach 65535.
DAQ_NOISE_FN uint32_t window_stop(const chroma_daq_reducer &r, uint32_t e, uint32_t a_next, uint32_t G)
{
    const uint64_t reach = (uint64_t)e + r.lag;
    const uint32_t limit = a_next < G ? a_next : G;
    return reach < limit ? (uint32_t)reach : limit;
}

DAQ_NOISE_FN uint32_t window_begin(const chroma_daq_reducer &r, uint32_t a, uint32_t stop_before)
{
    const uint32_t from = a > r.lead ? a - r.lead : 0u;
    return from > stop_before ? from : stop_before;
}

// L = max(1, (peak * cfd) >> 8): peak < 2^22 and cfd <= 256, so the product is below 2^31
DAQ_NOISE_FN int32_t cfd_level(const chroma_daq_reducer &r, uint32_t peak)
{
    const uint32_t l = (peak * r.cfd) >> 8;
    return (int32_t)(l ? l : 1u);
}

// The time of a crossing between sample s_c - 1 (y0 < L) and sample s_c (y1 >= L), in 1/256 of a sample: the fraction is in
// (0, 256], and (L - y0) * 256 < 2^23 * 2^8
DAQ_NOISE_FN uint32_t cfd_time(uint32_t s_c, int32_t L, int32_t y0, int32_t y1)
{
    return 256u * (s_c - 1u) + ((uint32_t)(L - y0) * 256u) / (uint32_t)(y1 - y0);
}

// What both calls refuse, NULL arrays apart
static inline const char *check(const chroma_daq_reducer *r, uint32_t G, uint64_t ntraces)
{
    if (r->polarity != 1 && r->polarity != -1) return "DAQ reducer: the polarity is +1 or -1";
    if (G < 1 || G > MAX_SAMPLES) return "DAQ reducer: a trace has 1 .. 65536 samples";
    if (r->nbaseline > MAX_BASELINE || r->nbaseline > G) return "DAQ reducer: the baseline is measured over 0 .. 64 samples, the trace's at the most";
    if (r->pedestal > 65535u) return "DAQ reducer: the pedestal is 0 .. 65535";
    if (r->threshold < 1 || r->threshold > 65535u) return "DAQ reducer: the threshold is 1 .. 65535 ADC counts";
    if (r->min_width < 1 || r->min_width > 65536u) return "DAQ reducer: the shortest pulse has 1 .. 65536 samples";
    if (r->lead > 65535u || r->lag > 65535u) return "DAQ reducer: lead and lag are 0 .. 65535 samples";
    if (r->cfd < 1 || r->cfd > 256u) return "DAQ reducer: the constant fraction is 1 .. 256 in 1/256";
    if (ntraces >= 0x7fffffffull || ntraces * G >= 0x100000000ull) return "DAQ reducer: more samples than 32-bit indices hold, pass fewer traces";
    return nullptr;
}

}  // namespace daq_reduce
