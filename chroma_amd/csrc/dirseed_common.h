// dirseed_common.h -- the direction seed: a hit's unit vector seen from the vertex, a point's renormalisation, the cosine bin and
// what both calls refuse, written once for the device kernels (kernels_dirseed.h) and for the host loops (dirseed_host.cpp).  The
// contract is in include/chroma_hip.h ("direction seed").  The distance, the time bin, the tie-rule keys, the lattice and the
// cutting of a batch into launches are the vertex seed's (seed_common.h).  Everything that shows is integer: the truncating
// divisions take a double's quotient as an estimate and settle it in integers, as the floor square root does.
#pragma once

#include "seed_common.h"

namespace dirseed {

constexpr int32_t ONE = 1 << 14;                   // a unit direction's length, and the scale of a cosine
constexpr int32_t MAX_COMPONENT = 1 << 15;         // of a candidate, and of a lattice point: ONE + 2 * MAX_STEP
constexpr uint32_t MIN_LOG2_NCOS = 4u, MAX_LOG2_NCOS = 8u, MAX_STEP = 1u << 13, MAX_FIRST = 1040u, MAX_WIDTH = 2048u;
constexpr uint32_t RECORD_OUTSIDE = 0xffffu;       // the weight of an OUTSIDE hit's record (an INSIDE hit's is 0 .. 255)

// trunc(x * 16384 / d) for |x| < 2^26 and 1 <= d < 2^26: the magnitudes' quotient, below 2^40, from a double estimate (both
// operands are exact; the quotient, however it is rounded, is off by less than one) settled by two compares
SEED_FN int32_t q14_div(int64_t x, uint64_t d)
{
    const uint64_t n = (uint64_t)(x < 0 ? -x : x) << 14;
    uint64_t q = (uint64_t)((double)n / (double)d);
    if (q * d > n) q--;
    else if ((q + 1u) * d <= n) q++;
    return x < 0 ? -(int32_t)q : (int32_t)q;
}

// A hit's unit vector: (dx, dy, dz) / d in Q14, d = seed::distance's floor square root of the squared length (d >= 1; then every
// |component| <= d, so the quotients are within ONE)
SEED_FN void unit_of_hit(int64_t dx, int64_t dy, int64_t dz, uint64_t d, int32_t *nx, int32_t *ny, int32_t *nz)
{
    *nx = q14_div(dx, d); *ny = q14_div(dy, d); *nz = q14_div(dz, d);
}

// A point's unit vector: (0, 0, 0) for a point shorter than 1; components within MAX_COMPONENT, so a . a <= 3 * 2^30
SEED_FN void unit_of_point(int32_t ax, int32_t ay, int32_t az, int32_t *ux, int32_t *uy, int32_t *uz)
{
    const uint64_t L = seed::isqrt_floor((uint64_t)((int64_t)ax * ax) + (uint64_t)((int64_t)ay * ay) + (uint64_t)((int64_t)az * az));
    if (L == 0u) { *ux = *uy = *uz = 0; return; }
    *ux = q14_div(ax, L); *uy = q14_div(ay, L); *uz = q14_div(az, L);
}

// the cosine of two unit vectors, -16384 .. 16383: the dot product fits int32 (3 * 2^28), the shift is arithmetic
SEED_FN int32_t cosine(int32_t nx, int32_t ny, int32_t nz, int32_t ux, int32_t uy, int32_t uz)
{
    const int32_t c = (nx * ux + ny * uy + nz * uz) >> 14;
    return c < -ONE ? -ONE : c > ONE - 1 ? ONE - 1 : c;
}
// its bin among the 2^m of the profile
SEED_FN uint32_t cos_bin(int32_t c, uint32_t log2_ncos) { return (uint32_t)(c + ONE) >> (15u - log2_ncos); }

// The per-hit work, done once per hit: false for an OUTSIDE hit; else the weight 0 .. 255 and the unit vector.  `timing` is read
// only with times (`timed`: `time` the hit's; tau0 and bin the fit's)
SEED_FN bool hit_record(const chroma_direction_seeder &p, const chroma_vertex_seeder *timing, uint32_t nchannels, const int32_t *channel_pos, int32_t channel,
                        bool timed, int32_t time, uint32_t weight, int32_t vx, int32_t vy, int32_t vz, int32_t tau0, uint32_t bin, uint32_t *w, int32_t *nx,
                        int32_t *ny, int32_t *nz)
{
    if (channel < 0 || (uint32_t)channel >= nchannels) return false;
    const int32_t cx = channel_pos[3 * (size_t)channel], cy = channel_pos[3 * (size_t)channel + 1], cz = channel_pos[3 * (size_t)channel + 2];
    const uint64_t d = seed::distance(cx, cy, cz, vx, vy, vz);
    if (d == 0u) return false;
    if (timed) {
        const uint32_t b = seed::bin_of(time, seed::time_of_flight(d, timing->slowness), tau0, timing->bin_ticks, timing->nbins * timing->bin_ticks);
        if (b == seed::OUTSIDE) return false;
        const uint64_t lo = (uint64_t)bin + p.first;
        if (b < lo || b >= lo + p.width) return false;
    }
    *w = weight < seed::MAX_WEIGHT ? weight : seed::MAX_WEIGHT;
    unit_of_hit((int64_t)cx - vx, (int64_t)cy - vy, (int64_t)cz - vz, d, nx, ny, nz);
    return true;
}

SEED_FN bool component_ok(int32_t c) { return c >= -MAX_COMPONENT && c <= MAX_COMPONENT; }

// What both calls refuse of the seeder, the timing, the counts and the offsets (NULL arrays and the coordinates apart)
static inline const char *check(const chroma_direction_seeder *p, const chroma_vertex_seeder *timing, uint32_t nchannels, uint32_t ncand, uint32_t nfits,
                                const uint32_t *offsets)
{
    if (nchannels > 0xffffffffu / 3u) return "direction seed: more channel coordinates than 32-bit indices hold";
    if (p->log2_ncos < MIN_LOG2_NCOS || p->log2_ncos > MAX_LOG2_NCOS) return "direction seed: the profile has 2^4 .. 2^8 entries";
    if (p->step > MAX_STEP) return "direction seed: the step is 0 .. 2^13";
    if (p->nlevels > seed::MAX_LEVELS) return "direction seed: 0 .. 8 levels";
    if (p->first > MAX_FIRST) return "direction seed: the window begins 0 .. 1040 bins behind the seed's";
    if (p->width < 1 || p->width > MAX_WIDTH) return "direction seed: the window has 1 .. 2048 bins";
    uint32_t top = 0u;
    for (uint32_t k = 0; k < (1u << p->log2_ncos); k++) top = p->profile[k] > top ? p->profile[k] : top;
    if (top < 1u) return "direction seed: the profile is all zeros";
    if (timing) {
        if (timing->slowness < 1 || timing->slowness > seed::MAX_SLOWNESS) return "direction seed: the slowness is 1 .. 2^24";
        if (timing->bin_ticks < 1 || timing->bin_ticks > seed::MAX_BIN_TICKS) return "direction seed: a bin has 1 .. 2^20 ticks";
        if (timing->nbins < 1 || timing->nbins > seed::MAX_BINS) return "direction seed: 1 .. 1024 bins";
    }
    if (ncand < 1 || ncand > seed::MAX_CAND) return "direction seed: 1 .. 2^20 candidates";
    if (nfits == 0) return nullptr;
    if (nfits > 0x7fffffffu) return "direction seed: 2^31 - 1 fits at the most";
    if (offsets[0] != 0u) return "direction seed: the offsets start at 0";
    for (uint32_t f = 0; f < nfits; f++) {
        if (offsets[f + 1] < offsets[f]) return "direction seed: the offsets descend";
        if (offsets[f + 1] - offsets[f] > seed::MAX_FIT_HITS) return "direction seed: a fit holds 65535 hits at the most";
    }
    return nullptr;
}

}  // namespace dirseed
