// daq_reduce_host.cpp -- chroma_daq_reduce_host: the trace reduction of the time-binned DAQ as plain loops over trace, sample and
// pulse on the host, over the same functions as the device kernels (daq_reduce_common.h).  What the CPU tests run, what
// EventTriggers.reduce computes from saved traces, and the reduction of a machine without a GPU.
#include <stdint.h>
#include <vector>

#include "daq_reduce_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

namespace {

struct Run { uint32_t a, e; };

// y(s) of every sample into `y`, the trace's base and flag word; the pulses, in order, into `pulses`
void walk(const chroma_daq_reducer &r, uint32_t G, const uint16_t *v, std::vector<int32_t> &y, std::vector<Run> &pulses, int32_t *base, uint32_t *flags)
{
    uint32_t sum = 0u, lowest = 0xffffffffu, highest = 0u;
    for (uint32_t s = 0; s < r.nbaseline; s++) {
        sum += v[s];
        lowest = v[s] < lowest ? v[s] : lowest;
        highest = v[s] > highest ? v[s] : highest;
    }
    const daq_reduce::Level l = daq_reduce::level(r, sum);
    *base = l.base;
    *flags = daq_reduce::trace_flags(r, lowest, highest);
    pulses.clear();
    uint32_t a = 0u;
    bool open = false;
    for (uint32_t s = 0; s <= G; s++) {
        const bool above = s < G && (y[s] = daq_reduce::y_of(r, l, v[s])) >= l.T;
        if (above && !open) { a = s; open = true; }
        if (!above && open) {
            open = false;
            if (s - a >= r.min_width) pulses.push_back(Run{a, s});
        }
    }
}

}  // namespace

extern "C" {

int chroma_daq_reduce_host(const chroma_daq_reducer *reducer, uint32_t G, uint64_t ntraces, const uint16_t *adc, uint64_t found_capacity,
                           uint32_t *found_offsets, int32_t *trace_base, uint32_t *reduced_flags, uint32_t *found_start, uint32_t *found_width,
                           uint32_t *found_peak, uint32_t *found_peak_sample, int64_t *found_integral, uint32_t *found_time, uint32_t *found_flags,
                           uint64_t *nfound)
{
    if (!reducer || !nfound || (ntraces && (!adc || !found_offsets || !trace_base || !reduced_flags)) ||
        (ntraces && found_capacity && (!found_start || !found_width || !found_peak || !found_peak_sample || !found_integral || !found_time || !found_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = daq_reduce::check(reducer, G, ntraces)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    *nfound = 0;
    if (ntraces == 0) return CHROMA_OK;
    const chroma_daq_reducer &r = *reducer;
    std::vector<int32_t> y(G);
    std::vector<Run> pulses;
    uint32_t total = 0u;
    for (uint64_t t = 0; t < ntraces; t++) {
        walk(r, G, adc + t * G, y, pulses, &trace_base[t], &reduced_flags[t]);
        found_offsets[t] = total;
        total += (uint32_t)pulses.size();
    }
    found_offsets[ntraces] = total;
    *nfound = total;
    if (total > found_capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu found pulses, the traces hold %u", (unsigned long long)found_capacity, total);
    for (uint64_t t = 0; t < ntraces; t++) {
        int32_t base; uint32_t flags;
        walk(r, G, adc + t * G, y, pulses, &base, &flags);
        uint32_t stop_before = 0u;
        for (size_t j = 0; j < pulses.size(); j++) {
            const uint32_t a = pulses[j].a, e = pulses[j].e, at = found_offsets[t] + (uint32_t)j;
            const uint32_t stop = daq_reduce::window_stop(r, e, j + 1 < pulses.size() ? pulses[j + 1].a : G, G);
            const uint32_t begin = daq_reduce::window_begin(r, a, stop_before);
            stop_before = stop;
            int64_t integral = 0;
            for (uint32_t s = begin; s < stop; s++) integral += y[s];
            uint32_t peak_sample = a;
            for (uint32_t s = a + 1u; s < e; s++)
                if (y[s] > y[peak_sample]) peak_sample = s;
            const uint32_t peak = (uint32_t)y[peak_sample];
            const int32_t L = daq_reduce::cfd_level(r, peak);
            uint32_t s_c = peak_sample;
            while (s_c > begin && y[s_c - 1u] >= L) s_c--;
            uint32_t f = (a == 0u ? daq_reduce::OPEN_AT_START : 0u) | (e == G ? daq_reduce::OPEN_AT_END : 0u), time;
            if (s_c == begin && (begin == 0u || y[begin - 1u] >= L)) { time = 256u * s_c; f |= daq_reduce::TIME_AT_EDGE; }
            else time = daq_reduce::cfd_time(s_c, L, y[s_c - 1u], y[s_c]);
            found_start[at] = a; found_width[at] = e - a; found_peak[at] = peak; found_peak_sample[at] = peak_sample;
            found_integral[at] = integral; found_time[at] = time; found_flags[at] = f;
        }
    }
    return CHROMA_OK;
}

}  // extern "C"
