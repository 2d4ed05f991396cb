// kernels_dirseed.h -- the direction seed (chroma_direction_seed; the contract is in include/chroma_hip.h, the arithmetic in
// dirseed_common.h over seed_common.h).  One of the kernel families of libchroma_hip.so; included by dirseed_calls.hip alone.
//
// k_dir_prepare: a thread per hit, the per-hit work ONCE -- the fit by a search in the offsets, the channel's position, the distance,
// the time cut and the three divisions -- into an 8-byte record {int16 x, y, z; uint16 weight, dirseed::RECORD_OUTSIDE for an OUTSIDE hit},
// and the fit's `inside` and `outside` by vector atomics.  What follows reads records only.
// k_dir_scores: level 0.  Blocks (fit, eight candidates), a wave per candidate; the block stages the fit's records in LDS in chunks
// of 512 (an OUTSIDE record with the weight 0: it adds nothing) and the profile once; a wave takes a chunk 64 hits a round: three
// multiplies, a shift, a clamp, one LDS profile read, one multiply-add into a per-lane sum (a lane has 1024 hits at the most:
// 1024 * 255 * 255 < 2^32).  The wave's sum goes as key (score, candidate) to the fit's 64-bit word by a vector atomic max.
// k_dir_refine: levels 1 .. L, a block per fit, all levels in the one launch: per level sixteen rounds of eight lattice points
// folded through LDS, then a pass over the records for cos_hist (LDS adds into 2^m words); thread 0 stores the fit's results with
// ordinary stores.  A fit of 512 hits or fewer is staged once for all its points.
//
// LDS per block: 512 records (4096 bytes) and the profile (256); k_dir_refine adds cos_hist's 256 words and the few of the fold:
// DIRSEED_LDS_BYTES at the most.  No scratch.
#pragma once

#include "dirseed_common.h"
#include "seed_wave.h"

#define DIRSEED_BLOCK 512
#define DIRSEED_WAVES (DIRSEED_BLOCK / 64)
#define DIRSEED_CHUNK 512
#define DIRSEED_PREPARE_BLOCK 256
#define DIRSEED_LDS_BYTES (8 * DIRSEED_CHUNK + 256 + 4 * 256 + 8 * DIRSEED_WAVES + 16)

struct DirLds {
    uint2 record[DIRSEED_CHUNK];
    uint8_t profile[256];
};

struct DirHits { const int32_t *channel, *time; const uint32_t *weight; };

// The validation pass: *bad = 1 when one of the n values is beyond `bound` in magnitude
__global__ __launch_bounds__(256) void k_dir_check(const int32_t *values, uint32_t n, int32_t bound, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && (values[i] < -bound || values[i] > bound)) *bad = 1u;
}

// Hit hit_base + the thread's index (below nhits = offsets[nfits]): its fit is the last whose offset is not beyond it
__global__ __launch_bounds__(DIRSEED_PREPARE_BLOCK) void
k_dir_prepare(chroma_direction_seeder p, chroma_vertex_seeder timing, uint32_t nchannels, const int32_t *channel_pos, uint32_t nfits, const uint32_t *offsets,
              const int32_t *tau0, const int32_t *vertex, const uint32_t *bin, DirHits hits, uint32_t hit_base, uint32_t nhits, uint2 *records,
              uint32_t *inside, uint32_t *outside)
{
    const uint32_t at = blockIdx.x * DIRSEED_PREPARE_BLOCK + threadIdx.x;
    if (at >= nhits - hit_base) return;
    const uint32_t i = hit_base + at;
    uint32_t lo = 0u, hi = nfits;          // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t f = lo;
    const bool timed = hits.time != nullptr;
    const int32_t time = timed ? hits.time[i] : 0;
    uint32_t w = dirseed::RECORD_OUTSIDE;
    int32_t nx = 0, ny = 0, nz = 0;
    const bool in = dirseed::hit_record(p, &timing, nchannels, channel_pos, hits.channel[i], timed, time, hits.weight[i], vertex[3 * (size_t)f],
                                        vertex[3 * (size_t)f + 1], vertex[3 * (size_t)f + 2], timed ? tau0[f] : 0, timed ? bin[f] : 0u, &w, &nx, &ny, &nz);
    if (!in) { w = dirseed::RECORD_OUTSIDE; nx = ny = nz = 0; }
    records[i] = make_uint2(((uint32_t)nx & 0xffffu) | ((uint32_t)ny << 16), ((uint32_t)nz & 0xffffu) | (w << 16));
    if (!in) atomicAdd(&outside[f], 1u);
    else if (w) atomicAdd(&inside[f], w);
}

__device__ __forceinline__ void dir_load_profile(const chroma_direction_seeder &p, DirLds &lds)
{
    if (threadIdx.x < 256u) lds.profile[threadIdx.x] = threadIdx.x < (1u << p.log2_ncos) ? p.profile[threadIdx.x] : (uint8_t)0;
}

// a chunk's record as it is staged: an OUTSIDE hit with the weight 0
__device__ __forceinline__ uint2 dir_staged(uint2 r) { return (r.y >> 16) == dirseed::RECORD_OUTSIDE ? make_uint2(0u, 0u) : r; }
__device__ __forceinline__ int32_t dir_x(uint2 r) { return (int32_t)(int16_t)(r.x & 0xffffu); }
__device__ __forceinline__ int32_t dir_y(uint2 r) { return (int32_t)r.x >> 16; }
__device__ __forceinline__ int32_t dir_z(uint2 r) { return (int32_t)(int16_t)(r.y & 0xffffu); }
__device__ __forceinline__ uint32_t dir_w(uint2 r) { return r.y >> 16; }

// The block's chunk [base, base + count) of the fit whose records begin at `first`, into LDS (every thread of the block calls it)
__device__ __forceinline__ void dir_stage(const uint2 *records, uint32_t first, uint32_t base, uint32_t count, DirLds &lds)
{
    __syncthreads();          // (the chunk before is used up)
    if (threadIdx.x < count) lds.record[threadIdx.x] = dir_staged(records[(size_t)first + base + threadIdx.x]);
    __syncthreads();
}

// score(f, u) of this wave's unit vector u for the fit whose `n` records begin at `first`: every wave of the block calls it together
// (the staging is the block's), every lane gets the result.  `resident`: the fit's one chunk is staged already.  A wave without
// work passes any vector and ignores what comes back.
__device__ __forceinline__ uint32_t dir_evaluate(uint32_t log2_ncos, const uint2 *records, uint32_t first, uint32_t n, bool resident, int32_t ux, int32_t uy,
                                                 int32_t uz, DirLds &lds)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t sum = 0u;
    for (uint32_t base = 0u; base < n; base += DIRSEED_CHUNK) {          // (n is the block's: every wave makes every round)
        const uint32_t count = n - base < DIRSEED_CHUNK ? n - base : DIRSEED_CHUNK;
        if (!resident) dir_stage(records, first, base, count, lds);
        for (uint32_t i = lane; i < count; i += 64u) {
            const uint2 r = lds.record[i];
            const uint32_t k = dirseed::cos_bin(dirseed::cosine(dir_x(r), dir_y(r), dir_z(r), ux, uy, uz), log2_ncos);
            sum += dir_w(r) * lds.profile[k];
        }
    }
    sum = seed_wave_sum(sum);
    return (ux | uy | uz) ? sum : 0u;
}

// Level 0: block b is the candidates [8 (b % groups), + 8) of fit fit_base + b / groups
__global__ __launch_bounds__(DIRSEED_BLOCK) void
k_dir_scores(chroma_direction_seeder p, uint32_t ncand, const int32_t *cand, uint32_t groups, uint32_t fit_base, const uint32_t *offsets, const uint2 *records,
             unsigned long long *best0)
{
    __shared__ DirLds lds;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t fit = fit_base + blockIdx.x / groups, c = (blockIdx.x % groups) * DIRSEED_WAVES + wave;
    const uint32_t first = offsets[fit], n = offsets[fit + 1] - first;
    const uint32_t at = c < ncand ? c : ncand - 1u;
    int32_t ux, uy, uz;
    dirseed::unit_of_point(cand[3 * (size_t)at], cand[3 * (size_t)at + 1], cand[3 * (size_t)at + 2], &ux, &uy, &uz);
    dir_load_profile(p, lds);          // (dir_evaluate's first barrier is behind it; without hits nothing reads it)
    const uint32_t score = dir_evaluate(p.log2_ncos, records, first, n, false, ux, uy, uz, lds);
    if (c < ncand && lane == 0u) atomicMax(&best0[fit], (unsigned long long)seed::key_of(score, c));
}

struct DirResults { int32_t *best_dir; uint32_t *best_score, *best_cand, *level_score, *cos_hist; };

// Levels 1 .. L: block b is fit fit_base + b
__global__ __launch_bounds__(DIRSEED_BLOCK) void
k_dir_refine(chroma_direction_seeder p, uint32_t ncand, const int32_t *cand, uint32_t fit_base, const uint32_t *offsets, const uint2 *records,
             const unsigned long long *best0, DirResults out)
{
    __shared__ DirLds lds;
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long wave_key[DIRSEED_WAVES];
    __shared__ unsigned long long level_key;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t fit = fit_base + blockIdx.x;
    const uint32_t first = offsets[fit], n = offsets[fit + 1] - first;
    const uint64_t k0 = best0[fit];
    const uint32_t c0 = seed::key_index(k0) < ncand ? seed::key_index(k0) : 0u;          // (every fit's word has had a key: the index is a candidate's)
    int32_t x, y, z;
    dirseed::unit_of_point(cand[3 * (size_t)c0], cand[3 * (size_t)c0 + 1], cand[3 * (size_t)c0 + 2], &x, &y, &z);
    const bool resident = n <= DIRSEED_CHUNK;
    dir_load_profile(p, lds);
    if (resident) dir_stage(records, first, 0u, n, lds);
    else __syncthreads();
    uint32_t *ls = out.level_score + (size_t)fit * (p.nlevels + 1u);
    if (threadIdx.x == 0u) ls[0] = seed::key_score(k0);
    uint32_t score = seed::key_score(k0);
    for (uint32_t l = 1u; l <= p.nlevels; l++) {
        const uint32_t s = seed::level_spacing(p, l);
        if (threadIdx.x == 0u) level_key = 0ull;
        for (uint32_t m0 = 0u; m0 < seed::LATTICE; m0 += DIRSEED_WAVES) {
            const uint32_t m = m0 + wave;
            int32_t ux = x, uy = y, uz = z;          // (the centre as it is)
            if (m < seed::LATTICE && m != seed::CENTRE) {
                seed::lattice(m, s, x, y, z, &ux, &uy, &uz);
                dirseed::unit_of_point(ux, uy, uz, &ux, &uy, &uz);
            }
            const uint32_t got = dir_evaluate(p.log2_ncos, records, first, n, resident, ux, uy, uz, lds);
            if (lane == 0u) wave_key[wave] = m < seed::LATTICE ? seed::key_of(got, seed::lattice_rank(m)) : 0ull;
            __syncthreads();
            if (threadIdx.x == 0u) {
                unsigned long long k = level_key;
                for (uint32_t w = 0; w < DIRSEED_WAVES; w++) k = wave_key[w] > k ? wave_key[w] : k;
                level_key = k;
            }
            __syncthreads();
        }
        const uint64_t k = level_key;          // (every thread reads it before thread 0 clears it for the next level)
        __syncthreads();
        const uint32_t winner = seed::lattice_point(seed::key_index(k));
        if (winner != seed::CENTRE) {
            seed::lattice(winner, s, x, y, z, &x, &y, &z);
            dirseed::unit_of_point(x, y, z, &x, &y, &z);
        }
        score = seed::key_score(k);
        if (threadIdx.x == 0u) ls[l] = score;
    }
    if (out.cos_hist) {
        const uint32_t ncos = 1u << p.log2_ncos;
        if (threadIdx.x < 256u) hist[threadIdx.x] = 0u;
        __syncthreads();
        for (uint32_t base = 0u; base < n; base += DIRSEED_CHUNK) {
            const uint32_t count = n - base < DIRSEED_CHUNK ? n - base : DIRSEED_CHUNK;
            if (!resident) dir_stage(records, first, base, count, lds);
            if (threadIdx.x < count) {
                const uint2 r = lds.record[threadIdx.x];
                if (dir_w(r)) atomicAdd(&hist[dirseed::cos_bin(dirseed::cosine(dir_x(r), dir_y(r), dir_z(r), x, y, z), p.log2_ncos)], dir_w(r));
            }
        }
        __syncthreads();
        if (threadIdx.x < ncos) out.cos_hist[((size_t)fit << p.log2_ncos) + threadIdx.x] = hist[threadIdx.x];
    }
    if (threadIdx.x == 0u) {
        out.best_dir[3 * (size_t)fit] = x; out.best_dir[3 * (size_t)fit + 1] = y; out.best_dir[3 * (size_t)fit + 2] = z;
        out.best_score[fit] = score; out.best_cand[fit] = c0;
    }
}
