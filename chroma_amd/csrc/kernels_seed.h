// kernels_seed.h -- the vertex seed (chroma_vertex_seed; the contract is in include/chroma_hip.h, the arithmetic of one hit and
// the level lattice in seed_common.h).  One of the kernel families of libchroma_hip.so; included by seed_calls.hip alone.
//
// A wave per (fit, position), eight waves to a block, and a block's waves share ONE fit.  The block stages the fit's hits in LDS
// in chunks of 512 as (x, y, z, time, weight) arrays -- the channel's position gathered once per block and chunk, not once per
// position; a hit without a channel is staged with the weight OUTSIDE -- and every wave then takes the chunk 64 hits a round
// against its own position: distance, time of flight, bin, and an integer LDS add into the wave's own histogram of nbins + K
// words (the K words behind the last bin stay zero, so the shape reads past the end without a compare).  Hits per fit are bounded
// by nothing but the contract: the chunks loop.  The scan takes 64 start bins a round, K LDS reads each, keeps (A, first s) per lane
// as one 64-bit key (seed_common.h) and takes the maximum across the wave.
//
// k_seed_scores: level 0.  Blocks (fit, eight candidates); lane 0 of a wave stores the score when the caller asked for it and
// sends the key (score, candidate) to the fit's 64-bit word with a vector atomic max: the greatest score, the lowest index.
// k_seed_refine: levels 1 .. L, a block per fit, all levels inside the one launch: level_score[0] from the fit's word, per level
// sixteen rounds of eight lattice points, each wave's key folded into the level's maximum through LDS, then the FINAL point once
// more (its bin and its OUTSIDE hits); thread 0 stores the fit's results with ordinary stores.
//
// LDS per block, both kernels: 8 x 1040 histogram words, 5 x 512 staged words, 16 shape words and the refinement's few: SEED_LDS_BYTES
// at the most, three blocks to a CU.  No scratch.
#pragma once

#include "seed_common.h"
#include "seed_wave.h"

#define SEED_BLOCK 512
#define SEED_WAVES (SEED_BLOCK / 64)
#define SEED_CHUNK 512
#define SEED_HIST (seed::MAX_BINS + seed::MAX_SHAPE)
#define SEED_LDS_BYTES (4 * (SEED_WAVES * SEED_HIST + 5 * SEED_CHUNK + 16 + 32))

struct SeedHits { const int32_t *channel, *time; const uint32_t *weight; };

struct SeedLds {
    uint32_t hist[SEED_WAVES][SEED_HIST];
    int32_t x[SEED_CHUNK], y[SEED_CHUNK], z[SEED_CHUNK], time[SEED_CHUNK];
    uint32_t weight[SEED_CHUNK];
    uint32_t shape[16];
};

__device__ __forceinline__ void seed_load_shape(const chroma_vertex_seeder &p, SeedLds &lds)
{
    if (threadIdx.x < 16u) lds.shape[threadIdx.x] = threadIdx.x < p.nshape ? p.shape[threadIdx.x] : 0u;
}

// The key (score, bin) of this wave's position (x, y, z) for the fit whose `n` hits begin at `first`, and its OUTSIDE hits:
// every wave of the block calls it together (the staging is the block's), every lane gets the results.  A wave without work
// passes any position and ignores what comes back.
__device__ __forceinline__ uint64_t seed_evaluate(const chroma_vertex_seeder &p, uint32_t nchannels, const int32_t *channel_pos, const SeedHits &hits,
                                                  uint32_t first, uint32_t n, int32_t tau0, int32_t x, int32_t y, int32_t z, SeedLds &lds, uint32_t *outside)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t span = p.nbins * p.bin_ticks, words = p.nbins + p.nshape;
    uint32_t *H = lds.hist[wave];
    for (uint32_t b = lane; b < words; b += 64u) H[b] = 0u;
    seed_wave_sync();
    uint32_t out = 0u;
    for (uint32_t base = 0u; base < n; base += SEED_CHUNK) {          // (n is the block's: every wave makes every round)
        const uint32_t count = n - base < SEED_CHUNK ? n - base : SEED_CHUNK;
        __syncthreads();          // (the chunk before is used up)
        if (threadIdx.x < count) {
            const uint32_t i = first + base + threadIdx.x;
            const int32_t c = hits.channel[i];
            const bool known = c >= 0 && (uint32_t)c < nchannels;
            const uint32_t w = hits.weight[i];
            lds.x[threadIdx.x] = known ? channel_pos[3 * (size_t)c] : 0;
            lds.y[threadIdx.x] = known ? channel_pos[3 * (size_t)c + 1] : 0;
            lds.z[threadIdx.x] = known ? channel_pos[3 * (size_t)c + 2] : 0;
            lds.time[threadIdx.x] = hits.time[i];
            lds.weight[threadIdx.x] = known ? (w < seed::MAX_WEIGHT ? w : seed::MAX_WEIGHT) : seed::OUTSIDE;
        }
        __syncthreads();
        for (uint32_t i = lane; i < count; i += 64u) {
            const uint32_t w = lds.weight[i];
            uint32_t b = seed::OUTSIDE;
            if (w != seed::OUTSIDE) {
                const uint64_t d = seed::distance(lds.x[i], lds.y[i], lds.z[i], x, y, z);
                b = seed::bin_of(lds.time[i], seed::time_of_flight(d, p.slowness), tau0, p.bin_ticks, span);
            }
            if (b == seed::OUTSIDE) out++;
            else atomicAdd(&H[b], w);          // (b < nbins)
        }
    }
    seed_wave_sync();
    uint64_t best = 0u;
    for (uint32_t s = lane; s < p.nbins; s += 64u) {          // (a lane's s ascend: the first of its equals has the greater key)
        uint32_t A = 0u;
        for (uint32_t j = 0; j < p.nshape; j++) A += lds.shape[j] * H[s + j];
        const uint64_t key = seed::key_of(A, s);
        best = key > best ? key : best;
    }
    seed_wave_sync();          // (the histogram is read before the next position clears it)
    *outside = seed_wave_sum(out);
    return seed_wave_max(best);
}

// The validation pass: *bad = 1 when one of the n coordinates is beyond 2^23
__global__ __launch_bounds__(256) void k_seed_check(const int32_t *coords, uint32_t n, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && !seed::coordinate_ok(coords[i])) *bad = 1u;
}

// Level 0: block b is the candidates [8 (b % groups), + 8) of fit fit_base + b / groups
__global__ __launch_bounds__(SEED_BLOCK) void
k_seed_scores(chroma_vertex_seeder p, uint32_t nchannels, const int32_t *channel_pos, uint32_t ncand, const int32_t *cand, uint32_t groups, uint32_t fit_base,
              const uint32_t *offsets, const int32_t *tau0, SeedHits hits, unsigned long long *best0, uint32_t *scores)
{
    __shared__ SeedLds lds;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t fit = fit_base + blockIdx.x / groups, c = (blockIdx.x % groups) * SEED_WAVES + wave;
    const uint32_t first = offsets[fit], n = offsets[fit + 1] - first;
    const uint32_t at = c < ncand ? c : ncand - 1u;
    seed_load_shape(p, lds);
    __syncthreads();
    uint32_t outside;
    const uint64_t key = seed_evaluate(p, nchannels, channel_pos, hits, first, n, tau0[fit], cand[3 * (size_t)at], cand[3 * (size_t)at + 1],
                                       cand[3 * (size_t)at + 2], lds, &outside);
    if (c < ncand && lane == 0u) {
        if (scores) scores[(size_t)fit * ncand + c] = seed::key_score(key);
        atomicMax(&best0[fit], (unsigned long long)seed::key_of(seed::key_score(key), c));
    }
}

struct SeedResults { int32_t *best_pos; uint32_t *best_score, *best_bin, *best_cand, *outside, *level_score; };

// Levels 1 .. L: block b is fit fit_base + b
__global__ __launch_bounds__(SEED_BLOCK) void
k_seed_refine(chroma_vertex_seeder p, uint32_t nchannels, const int32_t *channel_pos, uint32_t ncand, const int32_t *cand, uint32_t fit_base,
              const uint32_t *offsets, const int32_t *tau0, SeedHits hits, const unsigned long long *best0, SeedResults out)
{
    __shared__ SeedLds lds;
    __shared__ unsigned long long wave_key[SEED_WAVES];
    __shared__ unsigned long long level_key;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t fit = fit_base + blockIdx.x;
    const uint32_t first = offsets[fit], n = offsets[fit + 1] - first;
    const int32_t t0 = tau0[fit];
    const uint64_t k0 = best0[fit];
    const uint32_t c0 = seed::key_index(k0) < ncand ? seed::key_index(k0) : 0u;          // (every fit's word has had a key: the index is a candidate's)
    int32_t x = cand[3 * (size_t)c0], y = cand[3 * (size_t)c0 + 1], z = cand[3 * (size_t)c0 + 2];
    seed_load_shape(p, lds);
    __syncthreads();
    uint32_t *ls = out.level_score + (size_t)fit * (p.nlevels + 1u);
    if (threadIdx.x == 0u) ls[0] = seed::key_score(k0);
    uint32_t outside;
    for (uint32_t l = 1u; l <= p.nlevels; l++) {
        const uint32_t s = seed::level_spacing(p, l);
        if (threadIdx.x == 0u) level_key = 0ull;
        for (uint32_t m0 = 0u; m0 < seed::LATTICE; m0 += SEED_WAVES) {
            const uint32_t m = m0 + wave;
            int32_t px, py, pz;
            seed::lattice(m < seed::LATTICE ? m : seed::CENTRE, s, x, y, z, &px, &py, &pz);
            const uint64_t key = seed_evaluate(p, nchannels, channel_pos, hits, first, n, t0, px, py, pz, lds, &outside);
            if (lane == 0u) wave_key[wave] = m < seed::LATTICE ? seed::key_of(seed::key_score(key), seed::lattice_rank(m)) : 0ull;
            __syncthreads();
            if (threadIdx.x == 0u) {
                unsigned long long k = level_key;
                for (uint32_t w = 0; w < SEED_WAVES; w++) k = wave_key[w] > k ? wave_key[w] : k;
                level_key = k;
            }
            __syncthreads();
        }
        const uint64_t k = level_key;          // (every thread reads it before thread 0 clears it: the barrier of the next evaluation is behind the clear,
        __syncthreads();                       //  so one more here)
        seed::lattice(seed::lattice_point(seed::key_index(k)), s, x, y, z, &x, &y, &z);
        if (threadIdx.x == 0u) ls[l] = seed::key_score(k);
    }
    const uint64_t last = seed_evaluate(p, nchannels, channel_pos, hits, first, n, t0, x, y, z, lds, &outside);
    if (threadIdx.x == 0u) {
        out.best_pos[3 * (size_t)fit] = x; out.best_pos[3 * (size_t)fit + 1] = y; out.best_pos[3 * (size_t)fit + 2] = z;
        out.best_score[fit] = seed::key_score(last); out.best_bin[fit] = seed::key_index(last);
        out.best_cand[fit] = c0; out.outside[fit] = outside;
    }
}
