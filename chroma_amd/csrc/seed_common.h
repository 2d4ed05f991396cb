// seed_common.h -- the vertex seed: the arithmetic of ONE hit at ONE position, the key a maximum is taken over and the level
// lattice, written once for the device kernels (kernels_seed.h) and for the host loops (seed_host.cpp).  The contract is in
// include/chroma_hip.h ("vertex seed").  Everything that shows is integer: the one floating-point operation, the square root's
// estimate, is corrected to the floor in integers, so the two sides produce the same bits whatever their square roots round to.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/chroma_math.h"
#include "../../include/chroma_hip.h"

#define SEED_FN __attribute__((always_inline)) CM_FN

namespace seed {

constexpr uint32_t MAX_BINS = 1024u, MAX_SHAPE = 16u, MAX_LEVELS = 8u, MAX_WEIGHT = 255u;
constexpr uint32_t MAX_CAND = 1u << 20, MAX_FIT_HITS = 65535u, MAX_STEP = 1u << 21, MAX_SLOWNESS = 1u << 24, MAX_BIN_TICKS = 1u << 20;
constexpr int32_t MAX_COORD = 1 << 23;
constexpr uint32_t LATTICE = 125u, CENTRE = 62u;
constexpr uint32_t OUTSIDE = 0xffffffffu;          // bin_of's answer for a hit outside, and the staged weight of a hit without a channel

// floor(sqrt(D2)) from an estimate that is the floor or one beside it: two compares settle it
SEED_FN uint64_t isqrt_settle(uint64_t D2, uint64_t d)
{
    if (d * d > D2) d--;
    else if ((d + 1u) * (d + 1u) <= D2) d++;
    return d;
}
// floor(sqrt(D2)), D2 < 2^53: the double is exact and its square root, however it is rounded, is off by far less than one from the
// true one, so its truncation is the floor or one beside it
SEED_FN uint64_t isqrt_floor(uint64_t D2) { return isqrt_settle(D2, (uint64_t)sqrt((double)D2)); }

// d of a channel at (cx, cy, cz) and a position (x, y, z): coordinates within 2^24 + 2^23 of each other's, so D2 < 2^53
SEED_FN uint64_t distance(int32_t cx, int32_t cy, int32_t cz, int32_t x, int32_t y, int32_t z)
{
    const int64_t dx = (int64_t)cx - x, dy = (int64_t)cy - y, dz = (int64_t)cz - z;
    return isqrt_floor((uint64_t)(dx * dx) + (uint64_t)(dy * dy) + (uint64_t)(dz * dz));
}

SEED_FN int64_t time_of_flight(uint64_t d, uint32_t slowness) { return (int64_t)((d * slowness + 32768u) >> 16); }

// the bin of a hit at `time` whose light flew `tof` ticks, or OUTSIDE.  span = nbins * bin_ticks <= 2^30: what is inside
// divides in 32 bits
SEED_FN uint32_t bin_of(int32_t time, int64_t tof, int32_t tau0, uint32_t bin_ticks, uint32_t span)
{
    const int64_t r = (int64_t)time - tof - (int64_t)tau0;
    if (r < 0 || r >= (int64_t)span) return OUTSIDE;
    return (uint32_t)r / bin_ticks;
}

// Maxima with a rule for ties are maxima of one 64-bit key: the score above, the complement of what the LOWEST of wins below
SEED_FN uint64_t key_of(uint32_t score, uint32_t lowest_wins) { return ((uint64_t)score << 32) | (uint32_t)~lowest_wins; }
SEED_FN uint32_t key_score(uint64_t key) { return (uint32_t)(key >> 32); }
SEED_FN uint32_t key_index(uint64_t key) { return ~(uint32_t)key; }
// among the points of a level the centre comes first, then the others by m
SEED_FN uint32_t lattice_rank(uint32_t m) { return m == CENTRE ? 0u : m + 1u; }
SEED_FN uint32_t lattice_point(uint32_t rank) { return rank == 0u ? CENTRE : rank - 1u; }

// point m of the level whose spacing is s, about (bx, by, bz)
SEED_FN void lattice(uint32_t m, uint32_t s, int32_t bx, int32_t by, int32_t bz, int32_t *x, int32_t *y, int32_t *z)
{
    *x = bx + ((int32_t)(m % 5u) - 2) * (int32_t)s;
    *y = by + ((int32_t)(m / 5u % 5u) - 2) * (int32_t)s;
    *z = bz + ((int32_t)(m / 25u) - 2) * (int32_t)s;
}
// (of a chroma_vertex_seeder, or of a chroma_direction_seeder: dirseed_common.h)
template <class Seeder> SEED_FN uint32_t level_spacing(const Seeder &p, uint32_t level) { return p.step >> (level - 1u); }

SEED_FN bool coordinate_ok(int32_t c) { return c >= -MAX_COORD && c <= MAX_COORD; }

// A launch holds fewer than 2^32 threads (HIP does not support gridDim.x * blockDim.x >= 2^32): so many blocks of `block` threads
constexpr uint32_t launch_blocks(uint32_t block) { return (uint32_t)(0xffffffffull / block); }
// the fits one level-0 launch of at most `limit` blocks takes: whole fits of `groups` blocks each, one at the least (a fit has
// 2^17 groups at the most, far fewer than a launch holds; a smaller `limit` is a test's)
static inline uint32_t fits_a_launch(uint32_t groups, uint32_t limit) { return limit / groups ? limit / groups : 1u; }

// What both calls refuse of the seeder, the counts and the two host arrays (NULL arrays and the coordinates apart)
static inline const char *check(const chroma_vertex_seeder *p, uint32_t nchannels, uint32_t ncand, uint32_t nfits, const uint32_t *offsets, bool scores)
{
    if (nchannels > 0xffffffffu / 3u) return "vertex seed: more channel coordinates than 32-bit indices hold";
    if (p->slowness < 1 || p->slowness > MAX_SLOWNESS) return "vertex seed: the slowness is 1 .. 2^24";
    if (p->bin_ticks < 1 || p->bin_ticks > MAX_BIN_TICKS) return "vertex seed: a bin has 1 .. 2^20 ticks";
    if (p->nbins < 1 || p->nbins > MAX_BINS) return "vertex seed: 1 .. 1024 bins";
    if (p->nshape < 1 || p->nshape > MAX_SHAPE) return "vertex seed: the shape has 1 .. 16 entries";
    if (p->step > MAX_STEP) return "vertex seed: the step is 0 .. 2^21";
    if (p->nlevels > MAX_LEVELS) return "vertex seed: 0 .. 8 levels";
    uint32_t top = 0u;
    for (uint32_t j = 0; j < p->nshape; j++) {
        if (p->shape[j] > 255u) return "vertex seed: a shape entry is 0 .. 255";
        top = p->shape[j] > top ? p->shape[j] : top;
    }
    if (top < 1u) return "vertex seed: the shape is all zeros";
    if (ncand < 1 || ncand > MAX_CAND) return "vertex seed: 1 .. 2^20 candidates";
    if (nfits == 0) return nullptr;
    if (nfits > 0x7fffffffu) return "vertex seed: 2^31 - 1 fits at the most";
    if (offsets[0] != 0u) return "vertex seed: the offsets start at 0";
    for (uint32_t f = 0; f < nfits; f++) {
        if (offsets[f + 1] < offsets[f]) return "vertex seed: the offsets descend";
        if (offsets[f + 1] - offsets[f] > MAX_FIT_HITS) return "vertex seed: a fit holds 65535 hits at the most";
    }
    if (scores && (uint64_t)nfits * ncand >= 0x100000000ull) return "vertex seed: more scores than 32-bit indices hold, pass fewer fits";
    return nullptr;
}

}  // namespace seed
