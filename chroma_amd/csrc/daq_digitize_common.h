// daq_digitize_common.h -- the digitiser of the time-binned DAQ: the arithmetic of ONE sample of a trace, written once for the
// device kernel (kernels_daq_digitize.h) and for the host loop (daq_digitize_host.cpp).  The contract is in
// include/chroma_hip.h ("digitiser").  Everything is integer: a 64-bit wrapping sum of 32 x 32 -> 64 bit products, an arithmetic
// shift, integer compares and a clip, so the two sides produce the same bits whatever the order of the sum.
#pragma once

#include <stdint.h>

#include "daq_noise_common.h"

namespace daq_digitize {

constexpr uint32_t MAX_TAPS = 1024u;             // the entries of a tap table
constexpr uint32_t MAX_NOISE = 64u;              // the entries of a noise table
constexpr uint32_t MAX_SAMPLES = 65536u;         // the samples of a trace
constexpr uint32_t BIN_OFFSET = 65536u;          // what makes a signed bin number a word index: B + 65536 >= 0 (pre <= 65536)
constexpr uint32_t BLOCK_HIGH = 0x80000000u;     // the top bit of the digitiser's Philox blocks: the dark noise has blocks 0 .. 48
constexpr uint32_t CLIPPED_HIGH = 1u, CLIPPED_LOW = 2u;          // the bits of a trace's flag word
constexpr uint32_t NONE = 0xffffffffu;

// What pulse (bin, q) adds to the sum of the sample of bin B: q * taps[B - bin] if the tap exists.  B is a signed bin number in
// 64 bits, so no value of a trigger's bin makes the difference wrap.
DAQ_NOISE_FN uint64_t term(int64_t B, uint32_t bin, uint32_t q, const int32_t *taps, uint32_t ntaps)
{
    const int64_t d = B - (int64_t)bin;
    if (d < 0 || d >= (int64_t)ntaps) return 0ull;
    return (uint64_t)((int64_t)q * (int64_t)taps[d]);
}

// The noise word of (stream, channel, bin B): word u & 3 of block BLOCK_HIGH | u >> 2 of the channel's pseudo-photon, u = B + 65536.
// The Stream keeps the block, so a caller that walks consecutive bins draws one block per four.
DAQ_NOISE_FN uint32_t noise_word(daq_noise::Stream *s, int64_t B)
{
    const uint32_t u = (uint32_t)(B + (int64_t)BIN_OFFSET);
    const uint32_t block = BLOCK_HIGH | (u >> 2);
    if (block != s->block) {
        uint32_t out[4];
        cm_philox4x32_10(block, s->stream, s->channel, daq_noise::ID_HIGH, s->key0, s->key1, out);
        s->b0 = out[0]; s->b1 = out[1]; s->b2 = out[2]; s->b3 = out[3];
        s->block = block;
    }
    const uint32_t b0 = s->b0, b1 = s->b1, b2 = s->b2, b3 = s->b3;
    const uint32_t at = u & 3u;
    return at == 0u ? b0 : at == 1u ? b1 : at == 2u ? b2 : b3;
}

// e(s): noise_lo plus the entries of the (non-decreasing) table that the word reaches
DAQ_NOISE_FN int32_t noise_value(uint32_t w, const uint32_t *noise_cdf, uint32_t nnoise, int32_t noise_lo)
{
    return noise_lo + (int32_t)daq_noise::count(w, noise_cdf, nnoise);
}

// v(s) from the wrapped sum and the noise value; ORs CLIPPED_HIGH or CLIPPED_LOW into *flags.  The shifted sum is first limited to
// +- 2^40, far outside every clip range, so that adding to a sum near the ends of int64 (shift 0) cannot overflow: no result changes.
DAQ_NOISE_FN uint16_t sample(uint64_t acc, uint32_t shift, int32_t pedestal, int32_t e, uint32_t bits, uint32_t *flags)
{
    const int64_t limit = (int64_t)1 << 40;
    int64_t signal = (int64_t)acc >> shift;
    signal = signal > limit ? limit : signal < -limit ? -limit : signal;
    const int64_t v = (int64_t)pedestal + signal + (int64_t)e;
    const int64_t top = ((int64_t)1 << bits) - 1;
    if (v > top) { *flags |= CLIPPED_HIGH; return (uint16_t)top; }
    if (v < 0) { *flags |= CLIPPED_LOW; return (uint16_t)0; }
    return (uint16_t)v;
}

// The last k of [0, n) with offsets[k] <= i, if i < offsets[k + 1]; NONE otherwise (and when n is 0).  Reads offsets[0 .. n]
// only, whatever they hold.
DAQ_NOISE_FN uint32_t segment_of(const uint32_t *offsets, uint32_t n, uint32_t i)
{
    if (n == 0u) return NONE;
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t half = lo + (hi - lo + 1u) / 2u;
        if (offsets[half] <= i) lo = half; else hi = half - 1u;
    }
    return (offsets[lo] <= i && i < offsets[lo + 1u]) ? lo : NONE;
}

// The first p of [lo, hi) whose (channel, bin) is not below (c, x), hi if none is: the pulses of a row are in (channel, bin)
// order.  Reads entries of [lo, hi) only.
DAQ_NOISE_FN uint32_t lower_bound(const int32_t *channel, const uint32_t *bin, uint32_t lo, uint32_t hi, int32_t c, int64_t x)
{
    while (lo < hi) {
        const uint32_t half = lo + (hi - lo) / 2u;
        const int32_t ch = channel[half];
        if (ch < c || (ch == c && (int64_t)bin[half] < x)) lo = half + 1u; else hi = half;
    }
    return lo;
}

// A trace's place: its trigger, its row, its channel, the bin of sample 0 and the run [first, end) of the row's pulses of its
// channel in the bins [B0 - ntaps + 1, B0 + G - 1] (empty for a trace without signal).
struct Trace { uint32_t row, channel, first, end; int64_t B0; };

DAQ_NOISE_FN Trace locate(uint32_t hit, uint32_t nrows, uint32_t nchannels, uint32_t pre, uint32_t G, uint32_t ntaps, const uint32_t *offsets,
                          const int32_t *channel, const uint32_t *bin, uint32_t npulses, const uint32_t *trig_offsets, const uint32_t *trig_bin,
                          uint32_t ntriggers, const uint32_t *hit_offsets, const int32_t *hit_channel)
{
    Trace t;
    const uint32_t k = segment_of(hit_offsets, ntriggers, hit);
    const uint32_t r = k != NONE ? segment_of(trig_offsets, nrows, k) : NONE;
    const int32_t c = hit_channel[hit];
    t.row = r != NONE ? r : 0u;
    t.channel = (uint32_t)c;
    t.B0 = (int64_t)(k != NONE ? trig_bin[k] : 0u) - (int64_t)pre;
    t.first = t.end = 0u;
    if (r != NONE && c >= 0 && (uint32_t)c < nchannels) {
        const uint32_t lo = offsets[r] < npulses ? offsets[r] : npulses, to = offsets[r + 1u] < npulses ? offsets[r + 1u] : npulses;
        const uint32_t hi = to > lo ? to : lo;
        t.first = lower_bound(channel, bin, lo, hi, c, t.B0 - (int64_t)ntaps + 1);
        t.end = lower_bound(channel, bin, t.first, hi, c, t.B0 + (int64_t)G);
    }
    return t;
}

// What both calls refuse (host side), NULL arrays apart
static inline const char *check(uint32_t nrows, uint32_t nchannels, const chroma_daq_window *window, const chroma_daq_trigger *trigger,
                                const chroma_daq_digitizer *dig, uint64_t npulses, uint64_t ntriggers, uint64_t nhits, uint64_t first_hit,
                                uint64_t nhits_call, uint64_t sample_capacity)
{
    if (nrows < 1 || nchannels < 1 || nchannels > 0x7fffffffu) return "need at least one row and 1 .. 2^31 - 1 channels";
    if (!(window->dt > 0.0f) || !(window->dt <= 3.4028234663852886e38f) || !(window->t0 >= -3.4028234663852886e38f && window->t0 <= 3.4028234663852886e38f) ||
        window->nbins < 1 || window->nbins > 65536)
        return "DAQ window: need a finite t0, a finite positive dt and 1 .. 65536 bins";
    if (trigger->kind != CHROMA_TRIGGER_NHIT && trigger->kind != CHROMA_TRIGGER_NPE) return "DAQ trigger: unknown kind";
    const uint64_t G = (uint64_t)trigger->pre + trigger->post;
    if (trigger->threshold < 1 || trigger->width < 1 || trigger->width > window->nbins || trigger->post < 1 || trigger->holdoff < (G > 1 ? G : 1))
        return "DAQ trigger: need a threshold of at least 1, a width of 1 .. nbins bins, post >= 1 and holdoff >= max(1, pre + post)";
    if ((uint64_t)nrows * window->nbins >= 0x80000000ull) return "more than 31-bit (row, bin) indices hold, pass fewer rows";
    if (G > MAX_SAMPLES) return "DAQ digitiser: a gate of more than 65536 samples";
    if (dig->ntaps < 1 || dig->ntaps > MAX_TAPS || !dig->taps) return "DAQ digitiser: need a tap table of 1 .. 1024 entries";
    if (dig->shift > 31) return "DAQ digitiser: the shift is 0 .. 31";
    if (dig->bits < 1 || dig->bits > 16) return "DAQ digitiser: samples have 1 .. 16 bits";
    if (dig->nnoise > MAX_NOISE || (dig->nnoise && !dig->noise_cdf)) return "DAQ digitiser: need a noise table of 0 .. 64 entries";
    for (uint32_t j = 1u; j < dig->nnoise; j++)
        if (dig->noise_cdf[j] < dig->noise_cdf[j - 1u]) return "DAQ digitiser: the noise table descends";
    if (npulses > 0xffffffffull || ntriggers > 0xffffffffull || nhits > 0xffffffffull) return "DAQ digitiser: more than 32-bit indices hold";
    if (first_hit > nhits || nhits_call > nhits - first_hit) return "DAQ digitiser: the slice ends beyond the hits";
    if (sample_capacity / G < nhits_call) return "DAQ digitiser: room for fewer samples than the slice's traces have";
    return nullptr;
}

}  // namespace daq_digitize
