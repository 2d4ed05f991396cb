// daq_noise_common.h -- PMT dark noise of the time-binned DAQ: what ONE (row, channel) word of an acquisition draws, written once
// for the device kernels (kernels_daq_noise.h) and for the host loop (daq_noise_host.cpp).  The contract is in
// include/chroma_hip.h ("dark noise").  Like steps_common.h it is plain arithmetic under CM_FN: integer compares, one 64-bit
// product, and single IEEE single-precision operations, and both sides are compiled with -ffp-contract=off, so the two produce
// the same bits.  interp_table (device_common.h) is restated here with the same operation order, because the host side
// cannot include it.
#pragma once

#include <stdint.h>

#include "../../include/chroma_math.h"
#include "../../include/chroma_hip.h"

// (always inlined: a Stream lives in registers only where no call takes its address)
#define DAQ_NOISE_FN __attribute__((always_inline)) CM_FN

namespace daq_noise {

constexpr uint32_t ID_HIGH = 0xffffffffu;          // the pseudo-photon of channel c: ID_HIGH << 32 | c
constexpr uint32_t MAX_COUNT = 64u;                // the entries of a count table
constexpr uint32_t ALWAYS = 0x80000000u;           // the accept word that keeps every candidate

// The words of the pseudo-photon's stream, taken in ascending order: word w is word w & 3 of Philox block w >> 2.  The block is
// held in four scalars and picked by selects (never indexed by a variable: it stays in registers).
struct Stream {
    uint32_t key0, key1, stream, channel;
    uint32_t b0, b1, b2, b3;
    uint32_t block;          // the block held, 0xffffffff = none
};

DAQ_NOISE_FN Stream open(uint64_t seed, uint32_t stream, uint32_t channel)
{
    Stream s;
    s.key0 = (uint32_t)seed; s.key1 = (uint32_t)(seed >> 32);
    s.stream = stream; s.channel = channel;
    s.b0 = s.b1 = s.b2 = s.b3 = 0u;
    s.block = 0xffffffffu;
    return s;
}

DAQ_NOISE_FN uint32_t word(Stream *s, uint32_t w)
{
    const uint32_t block = w >> 2;
    if (block != s->block) {
        uint32_t out[4];
        cm_philox4x32_10(block, s->stream, s->channel, ID_HIGH, s->key0, s->key1, out);
        s->b0 = out[0]; s->b1 = out[1]; s->b2 = out[2]; s->b3 = out[3];
        s->block = block;
    }
    const uint32_t b0 = s->b0, b1 = s->b1, b2 = s->b2, b3 = s->b3;          // (all four read, then picked: no load behind a select)
    const uint32_t at = w & 3u;
    return at == 0u ? b0 : at == 1u ? b1 : at == 2u ? b2 : b3;
}

// the candidates of a word: the entries of the (non-decreasing) table that word 0 reaches
DAQ_NOISE_FN uint32_t count(uint32_t word0, const uint32_t *count_cdf, uint32_t ncount)
{
    uint32_t k = 0u;
    for (uint32_t j = 0u; j < ncount; j++) k += (word0 >= count_cdf[j]) ? 1u : 0u;
    return k;
}

// the thinning of a candidate against the largest rate (accept: 0 never .. 2^31 always)
DAQ_NOISE_FN bool kept(uint32_t a, uint32_t accept) { return (a >> 1) < accept; }

// interp_table (device_common.h)
DAQ_NOISE_FN float interp_table(float x, int n, const float *xp, const float *fp)
{
    int lower = 0;
    int upper = n - 1;
    if (x <= xp[lower]) return fp[lower];
    if (x >= xp[upper]) return fp[upper];
    while (lower < upper - 1) {
        int half = (lower + upper) / 2;
        if (x < xp[half]) upper = half; else lower = half;
    }
    float df = fp[upper] - fp[lower];
    float dx = xp[upper] - xp[lower];
    return fp[lower] + df * (x - xp[lower]) / dx;
}

struct Photoelectron { uint32_t bin, time_bits, charge_int; };

// A kept candidate from its words b and c: the bin is the high word of b * nbins (always inside the window), the time lies in
// it by the next 24 bits of that product, the charge is a photon's.  The bin is the DRAWN one, whatever rounding makes of the time.
DAQ_NOISE_FN Photoelectron photoelectron(const chroma_daq_tables &tab, const chroma_daq_window &win, uint32_t b, uint32_t c)
{
    Photoelectron pe;
    const uint64_t p = (uint64_t)b * win.nbins;
    pe.bin = (uint32_t)(p >> 32);
    const float f = (float)((uint32_t)p >> 8) * 5.9604644775390625e-08f;          // (2^-24: exact)
    const float time = win.t0 + ((float)pe.bin + f) * win.dt;
    __builtin_memcpy(&pe.time_bits, &time, sizeof(uint32_t));
    const float charge = interp_table(cm_u32_to_uniform(c), tab.charge_cdf_len, tab.d_charge_cdf_y, tab.d_charge_cdf_x);
    pe.charge_int = cm_f2u32(cm_roundf(charge / tab.charge_unit));
    return pe;
}

// what the calls refuse of a chroma_daq_noise (host side)
static inline const char *check(const chroma_daq_noise *noise)
{
    if (!noise->count_cdf || !noise->d_accept) return "DAQ noise: null array";
    if (noise->ncount < 1u || noise->ncount > MAX_COUNT) return "DAQ noise: the count table has 1 .. 64 entries";
    for (uint32_t j = 1u; j < noise->ncount; j++)
        if (noise->count_cdf[j] < noise->count_cdf[j - 1u]) return "DAQ noise: the count table descends";
    if (!noise->flag || (noise->flag & (noise->flag - 1u))) return "DAQ noise: the flag is one history bit";
    return nullptr;
}

}  // namespace daq_noise
