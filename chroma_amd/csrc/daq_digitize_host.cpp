// daq_digitize_host.cpp -- chroma_daq_digitize_host: the digitiser of the time-binned DAQ as a plain loop over trace, sample and
// pulse on the host, over the same per-sample functions as the device kernel (daq_digitize_common.h).  What the CPU tests run,
// what EventTriggers.digitize computes from saved pulses and triggers, and the digitiser of a machine without a GPU.
#include <stdint.h>

#include "daq_digitize_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

extern "C" {

int chroma_daq_digitize_host(uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window, const chroma_daq_trigger *trigger,
                             const chroma_daq_digitizer *digitizer, uint64_t seed, uint32_t acquisition, const uint32_t *offsets,
                             const int32_t *channel, const uint32_t *bin, const uint32_t *q_int, uint64_t npulses, const uint32_t *trig_offsets,
                             const uint32_t *trig_bin, uint64_t ntriggers, const uint32_t *hit_offsets, const int32_t *hit_channel, uint64_t nhits,
                             uint64_t first_hit, uint64_t nhits_call, uint64_t sample_capacity, uint16_t *adc, uint32_t *trace_flags)
{
    if (!window || !trigger || !digitizer || !offsets || !trig_offsets || !hit_offsets || (npulses && (!channel || !bin || !q_int)) ||
        (ntriggers && !trig_bin) || (nhits && !hit_channel) || (nhits_call && (!adc || !trace_flags)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = daq_digitize::check(nrows, nchannels, window, trigger, digitizer, npulses, ntriggers, nhits, first_hit, nhits_call, sample_capacity))
        return set_error(CHROMA_ERR_INVALID, "%s", why);
    const uint32_t pre = trigger->pre, G = trigger->pre + trigger->post;
    for (uint64_t trace = 0; trace < nhits_call; trace++) {
        const daq_digitize::Trace t = daq_digitize::locate((uint32_t)(first_hit + trace), nrows, nchannels, pre, G, digitizer->ntaps, offsets, channel, bin,
                                                           (uint32_t)npulses, trig_offsets, trig_bin, (uint32_t)ntriggers, hit_offsets, hit_channel);
        daq_noise::Stream stream = daq_noise::open(seed, 1u + acquisition + t.row, t.channel);
        uint32_t flags = 0u;
        for (uint32_t s = 0; s < G; s++) {
            const int64_t B = t.B0 + (int64_t)s;
            uint64_t acc = 0ull;
            for (uint32_t p = t.first; p < t.end; p++) acc += daq_digitize::term(B, bin[p], q_int[p], digitizer->taps, digitizer->ntaps);
            int32_t e = 0;
            if (digitizer->nnoise) e = daq_digitize::noise_value(daq_digitize::noise_word(&stream, B), digitizer->noise_cdf, digitizer->nnoise, digitizer->noise_lo);
            adc[trace * G + s] = daq_digitize::sample(acc, digitizer->shift, digitizer->pedestal, e, digitizer->bits, &flags);
        }
        trace_flags[trace] = flags;
    }
    return CHROMA_OK;
}

}  // extern "C"
