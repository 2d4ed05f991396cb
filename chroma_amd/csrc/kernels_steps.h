// kernels_steps.h -- photons from charged-particle steps on the device (chroma_steps_count / chroma_steps_generate,
// steps_calls.hip, which alone includes it).  What a segment and a photon compute is steps_common.h, shared with the host loops of steps_host.cpp.
#pragma once

#include "steps_common.h"

#define STEPS_BLOCK 256

// One thread per segment: counts[2 s] Cherenkov and counts[2 s + 1] scintillation photons (what the scan turns into the
// photons' offsets); counts[2 n] = 0, so that the exclusive sum leaves the total there.  The 64-bit total is added up beside
// it, one atomic per wave: the offsets are 32 bits wide and the caller has to know when they would not do.
__global__ void __launch_bounds__(STEPS_BLOCK)
k_steps_count(steps::Source src, chroma_step_segments segs, uint64_t seed, uint32_t *counts, unsigned long long *total)
{
    const uint64_t s = (uint64_t)blockIdx.x * STEPS_BLOCK + threadIdx.x;
    uint32_t n_ch = 0, n_sc = 0;
    if (s < segs.n) {
        steps::segment_counts(src, steps::load_segment(segs, s), seed, segs.segment_base + s, &n_ch, &n_sc);
        counts[2 * s] = n_ch;
        counts[2 * s + 1] = n_sc;
    }
    if (s == 0) counts[2 * segs.n] = 0u;
    const unsigned long long sum = wave_sum_u64((unsigned long long)n_ch + n_sc);
    if (lane_id() == 0 && sum) atomicAdd(total, sum);
}

// One thread per photon.  The thread finds its run by binary search in the scanned offsets -- neighbouring lanes mostly land
// in the same segment, so its record is one address for the wave -- and builds the photon in registers.  What is left is the
// kernel's real work, 64 bytes of stores per photon: the seven 4-byte arrays are one dword per lane at consecutive addresses as
// they stand; the three float3 arrays would be 12-byte strides, so the block turns them through LDS and writes each as
// 3 x STEPS_BLOCK consecutive dwords.
__global__ void __launch_bounds__(STEPS_BLOCK)
k_steps_generate(steps::Source src, chroma_step_segments segs, uint64_t seed, const uint32_t *offsets, PhotonView out, uint32_t total)
{
    __shared__ float s_vec[3][3 * STEPS_BLOCK];
    const uint32_t first = blockIdx.x * STEPS_BLOCK;               // (the grid is ceil(total / STEPS_BLOCK): no overflow)
    const uint32_t i = first + threadIdx.x;
    const bool on = i < total;
    if (on) {
        const uint32_t run = steps::find_run(offsets, 2u * (uint32_t)segs.n, i);
        const uint32_t s = run >> 1;
        const uint32_t seg_first = offsets[2 * s];
        const steps::Segment g = steps::load_segment(segs, s);
        const steps::PhotonOut p = steps::make_photon(src, g, seed, segs.segment_base + s, i - seg_first, offsets[2 * s + 1] - seg_first);
        float *v = &s_vec[0][3 * threadIdx.x];
        v[0] = p.pos.x; v[1] = p.pos.y; v[2] = p.pos.z;
        v = &s_vec[1][3 * threadIdx.x];
        v[0] = p.dir.x; v[1] = p.dir.y; v[2] = p.dir.z;
        v = &s_vec[2][3 * threadIdx.x];
        v[0] = p.pol.x; v[1] = p.pol.y; v[2] = p.pol.z;
        out.wavelengths[i] = p.wavelength;
        out.t[i] = p.t;
        out.flags[i] = p.flags;
        out.last_hit_triangles[i] = -1;
        out.weights[i] = 1.0f;
        out.evidx[i] = g.evidx;
        out.rng_counters[i] = 0u;
    }
    __syncthreads();
    const uint32_t left = total - first;                            // photons of this block ...
    const uint32_t nfloats = 3u * (left < STEPS_BLOCK ? left : STEPS_BLOCK);
    const size_t base = 3 * (size_t)first;
    for (uint32_t k = threadIdx.x; k < nfloats; k += STEPS_BLOCK) {
        out.pos[base + k] = s_vec[0][k];
        out.dir[base + k] = s_vec[1][k];
        out.pol[base + k] = s_vec[2][k];
    }
}

// ---- a medium per segment (chroma_steps_count_media / chroma_steps_generate_media) ----
// The two kernels above with the Source built per thread: row medium[s] of the device-resident table (steps::media_source,
// base pointers and strides; nothing is copied).  Neighbouring lanes share a segment or lie on one track, so in most waves the
// row is the same for all lanes and the table reads stay one address per wave.
__global__ void __launch_bounds__(STEPS_BLOCK)
k_steps_count_media(steps::Media media, chroma_step_segments segs, const int32_t *medium, uint64_t seed, uint32_t *counts,
                    unsigned long long *total)
{
    const uint64_t s = (uint64_t)blockIdx.x * STEPS_BLOCK + threadIdx.x;
    uint32_t n_ch = 0, n_sc = 0;
    if (s < segs.n) {
        const int32_t m = medium[s];
        if (steps::medium_ok(media, m))
            steps::segment_counts(steps::media_source(media, (uint32_t)m), steps::load_segment(segs, s), seed, segs.segment_base + s, &n_ch, &n_sc);
        counts[2 * s] = n_ch;
        counts[2 * s + 1] = n_sc;
    }
    if (s == 0) counts[2 * segs.n] = 0u;
    const unsigned long long sum = wave_sum_u64((unsigned long long)n_ch + n_sc);
    if (lane_id() == 0 && sum) atomicAdd(total, sum);
}

// k_steps_generate's store scheme as it stands.  A photon's segment has a row of the table, or the count call would have given
// it no photon; offsets that were counted with another medium array are not trusted with an address all the same: such a
// photon is written as zeros.
__global__ void __launch_bounds__(STEPS_BLOCK)
k_steps_generate_media(steps::Media media, chroma_step_segments segs, const int32_t *medium, uint64_t seed, const uint32_t *offsets,
                       PhotonView out, uint32_t total)
{
    __shared__ float s_vec[3][3 * STEPS_BLOCK];
    const uint32_t first = blockIdx.x * STEPS_BLOCK;               // (the grid is ceil(total / STEPS_BLOCK): no overflow)
    const uint32_t i = first + threadIdx.x;
    const bool on = i < total;
    if (on) {
        const uint32_t run = steps::find_run(offsets, 2u * (uint32_t)segs.n, i);
        const uint32_t s = run >> 1;
        const uint32_t seg_first = offsets[2 * s];
        const steps::Segment g = steps::load_segment(segs, s);
        const int32_t m = medium[s];
        steps::PhotonOut p = {};
        if (steps::medium_ok(media, m))
            p = steps::make_photon(steps::media_source(media, (uint32_t)m), g, seed, segs.segment_base + s, i - seg_first, offsets[2 * s + 1] - seg_first);
        float *v = &s_vec[0][3 * threadIdx.x];
        v[0] = p.pos.x; v[1] = p.pos.y; v[2] = p.pos.z;
        v = &s_vec[1][3 * threadIdx.x];
        v[0] = p.dir.x; v[1] = p.dir.y; v[2] = p.dir.z;
        v = &s_vec[2][3 * threadIdx.x];
        v[0] = p.pol.x; v[1] = p.pol.y; v[2] = p.pol.z;
        out.wavelengths[i] = p.wavelength;
        out.t[i] = p.t;
        out.flags[i] = p.flags;
        out.last_hit_triangles[i] = -1;
        out.weights[i] = 1.0f;
        out.evidx[i] = g.evidx;
        out.rng_counters[i] = 0u;
    }
    __syncthreads();
    const uint32_t left = total - first;                            // photons of this block ...
    const uint32_t nfloats = 3u * (left < STEPS_BLOCK ? left : STEPS_BLOCK);
    const size_t base = 3 * (size_t)first;
    for (uint32_t k = threadIdx.x; k < nfloats; k += STEPS_BLOCK) {
        out.pos[base + k] = s_vec[0][k];
        out.dir[base + k] = s_vec[1][k];
        out.pol[base + k] = s_vec[2][k];
    }
}
