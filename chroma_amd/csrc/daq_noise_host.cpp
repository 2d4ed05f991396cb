// daq_noise_host.cpp -- chroma_daq_noise_host: the dark noise of the time-binned DAQ as a plain loop over the (row, channel) words
// on the host, over the same per-word functions as the device kernels (daq_noise_common.h).  What the CPU tests run, what the GPU
// tests build their comparand from, and the sampler of a machine without a GPU.
#include <stdint.h>

#include <cmath>

#include "daq_noise_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

extern "C" {

int chroma_daq_noise_host(const chroma_daq_tables *tables, const chroma_daq_window *window, const chroma_daq_noise *noise, uint32_t nrows,
                          uint32_t nchannels, uint64_t seed, uint32_t acquisition, uint64_t capacity, uint32_t *row, uint32_t *channel,
                          uint32_t *bin, uint32_t *time_bits, uint32_t *charge_int, uint64_t *n)
{
    if (!tables || !window || !noise || !n || (capacity && (!row || !channel || !bin || !time_bits || !charge_int)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nrows < 1 || nchannels < 1) return set_error(CHROMA_ERR_INVALID, "need at least one row and one channel");
    if (!(window->dt > 0.0f) || !std::isfinite(window->dt) || !std::isfinite(window->t0) || window->nbins < 1 || window->nbins > 65536)
        return set_error(CHROMA_ERR_INVALID, "DAQ window: need a finite t0, a finite positive dt and 1 .. 65536 bins");
    if (tables->charge_cdf_len < 2 || !tables->d_charge_cdf_x || !tables->d_charge_cdf_y || !(tables->charge_unit > 0.0f))
        return set_error(CHROMA_ERR_INVALID, "DAQ tables: need a charge CDF of at least 2 points and a positive charge unit");
    if (const char *why = daq_noise::check(noise)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    uint64_t total = 0;
    for (uint32_t r = 0; r < nrows; r++)
        for (uint32_t c = 0; c < nchannels; c++) {
            const uint32_t accept = noise->d_accept[c];
            if (!accept) continue;
            daq_noise::Stream s = daq_noise::open(seed, 1u + acquisition + r, c);
            const uint32_t k = daq_noise::count(daq_noise::word(&s, 0u), noise->count_cdf, noise->ncount);
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t a = daq_noise::word(&s, 1u + 3u * j), b = daq_noise::word(&s, 2u + 3u * j), d = daq_noise::word(&s, 3u + 3u * j);
                if (!daq_noise::kept(a, accept)) continue;
                if (total < capacity) {
                    const daq_noise::Photoelectron pe = daq_noise::photoelectron(*tables, *window, b, d);
                    row[total] = r; channel[total] = c; bin[total] = pe.bin; time_bits[total] = pe.time_bits; charge_int[total] = pe.charge_int;
                }
                total++;
            }
        }
    *n = total;
    if (total > capacity) return set_error(CHROMA_ERR_INVALID, "room for %llu noise photoelectrons, the rows hold %llu", (unsigned long long)capacity,
                                           (unsigned long long)total);
    return CHROMA_OK;
}

}  // extern "C"
