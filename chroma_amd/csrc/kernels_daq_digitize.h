// kernels_daq_digitize.h -- the digitiser of the time-binned DAQ: a shaped ADC trace per gated hit of chroma_daq_trigger_pulses
// (chroma_daq_digitize_gates; the contract is in include/chroma_hip.h, the arithmetic of one sample in daq_digitize_common.h).
// One of the kernel families of libchroma_hip.so; included by daq_calls.hip alone.
//
// A wave per trace, four traces per block.  The block first copies the tap table into LDS (a lane's tap index is its own, so
// the table cannot come through scalar loads).  A wave then finds its place -- the trigger of its hit by a search of the hit
// offsets, the row of the trigger by a search of the trigger offsets, and the run of its (row, channel)'s pulses in reach of
// the trace by two (channel, bin) searches within the row -- all on wave-uniform values.  Lanes take 64 consecutive samples
// at a time; the pulses in reach of those 64 are loaded 64 at a time, lane p the p-th, and handed round the wave lane by lane
// (v_readlane: no LDS), every lane adding q * taps[d] where its d exists.  The noise word of a sample is one Philox block per
// lane, the noise table comes in the kernel's arguments (scalar loads), the stores are 16-bit and lane-consecutive, and the clip
// flags of the trace are gathered by ballot.  Sums are 64-bit and wrapping: their order does not show.
#pragma once

#include "daq_digitize_common.h"

#define DAQ_DIGITIZE_BLOCK 256
#define DAQ_DIGITIZE_WAVES (DAQ_DIGITIZE_BLOCK / 64)

// what a launch needs of a chroma_daq_digitizer: the noise table by value, the taps on the device
struct DaqDigitizeView {
    uint32_t noise_cdf[64];
    uint32_t nnoise;
    int32_t noise_lo;
    uint32_t ntaps, shift;
    int32_t pedestal;
    uint32_t bits;
    const int32_t *taps;
};

__global__ __launch_bounds__(DAQ_DIGITIZE_BLOCK) void
k_daq_digitize(DaqDigitizeView dig, uint32_t nrows, uint32_t nchannels, uint32_t pre, uint32_t G, uint64_t seed, uint32_t acquisition,
               const uint32_t *offsets, const int32_t *channel, const uint32_t *bin, const uint32_t *q_int, uint32_t npulses,
               const uint32_t *trig_offsets, const uint32_t *trig_bin, uint32_t ntriggers, const uint32_t *hit_offsets, const int32_t *hit_channel,
               uint32_t first_hit, uint32_t nhits_call, uint16_t *adc, uint32_t *trace_flags)
{
    __shared__ int32_t s_taps[daq_digitize::MAX_TAPS];
    for (uint32_t t = threadIdx.x; t < dig.ntaps; t += DAQ_DIGITIZE_BLOCK) s_taps[t] = dig.taps[t];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t trace = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * DAQ_DIGITIZE_WAVES + (threadIdx.x >> 6)));
    if (trace >= nhits_call) return;          // (whole waves, behind the block's only barrier)
    const daq_digitize::Trace t = daq_digitize::locate(first_hit + trace, nrows, nchannels, pre, G, dig.ntaps, offsets, channel, bin, npulses,
                                                       trig_offsets, trig_bin, ntriggers, hit_offsets, hit_channel);
    daq_noise::Stream stream = daq_noise::open(seed, 1u + acquisition + t.row, t.channel);
    uint16_t *out = adc + (size_t)trace * G;
    uint32_t flags = 0u;
    for (uint32_t s0 = 0u; s0 < G; s0 += 64u) {
        const uint32_t s = s0 + lane;
        const int64_t B = t.B0 + (int64_t)s;
        // the pulses of the run in reach of these 64 samples (a trace of 64 samples or fewer: the run itself)
        uint32_t from = t.first, to = t.end;
        if (G > 64u) {
            from = daq_digitize::lower_bound(channel, bin, t.first, t.end, (int32_t)t.channel, t.B0 + (int64_t)s0 - (int64_t)dig.ntaps + 1);
            to = daq_digitize::lower_bound(channel, bin, from, t.end, (int32_t)t.channel, t.B0 + (int64_t)s0 + 64);
        }
        from = (uint32_t)__builtin_amdgcn_readfirstlane((int)from);
        to = (uint32_t)__builtin_amdgcn_readfirstlane((int)to);
        uint64_t acc = 0ull;
        for (uint32_t base = from; base < to; base += 64u) {
            const uint32_t p = base + lane;
            const uint32_t p_bin = p < to ? bin[p] : 0u, p_q = p < to ? q_int[p] : 0u;
            const uint32_t n = min(64u, to - base);
            for (uint32_t j = 0u; j < n; j++) {
                const uint32_t bin_j = (uint32_t)__builtin_amdgcn_readlane((int)p_bin, (int)j);
                const uint32_t q_j = (uint32_t)__builtin_amdgcn_readlane((int)p_q, (int)j);
                acc += daq_digitize::term(B, bin_j, q_j, s_taps, dig.ntaps);
            }
        }
        if (s < G) {
            int32_t e = 0;
            if (dig.nnoise) e = daq_digitize::noise_value(daq_digitize::noise_word(&stream, B), dig.noise_cdf, dig.nnoise, dig.noise_lo);
            out[s] = daq_digitize::sample(acc, dig.shift, dig.pedestal, e, dig.bits, &flags);
        }
    }
    const bool high = __ballot(flags & daq_digitize::CLIPPED_HIGH) != 0ull, low = __ballot(flags & daq_digitize::CLIPPED_LOW) != 0ull;
    if (lane == 0u) trace_flags[trace] = (high ? daq_digitize::CLIPPED_HIGH : 0u) | (low ? daq_digitize::CLIPPED_LOW : 0u);
}
