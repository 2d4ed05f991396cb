// kernels_particles.h -- the charged-particle stepper on the device (chroma_particles_*, steps_calls.hip, which alone includes
// it).  What a particle computes in one iteration is particles_common.h, shared with the host loops of particles_host.cpp.
#pragma once

#include "particles_common.h"

#define PARTICLES_BLOCK 256

// the particle of a queue slot: a queue holds its tail (entries + 1) in word 0 and the ids behind it, as the propagate loop's
// does; without one, slot i is particle i
__device__ inline uint32_t queued_particle(const uint32_t *queue, uint32_t slot) { return queue ? queue[1u + slot] : slot; }

// The live particles' rays as the dense arrays chroma_intersect_mesh's pipeline takes: origin, direction, last_hit per slot
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_rays(chroma_particle_arrays p, const uint32_t *queue, uint32_t nlive, float *origin, float *direction, int32_t *last_hit)
{
    const uint32_t slot = blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    if (slot >= nlive) return;
    const size_t i = queued_particle(queue, slot);
    for (int c = 0; c < 3; c++) {
        origin[3 * (size_t)slot + c] = p.pos[3 * i + c];
        direction[3 * (size_t)slot + c] = p.dir[3 * i + c];
    }
    last_hit[slot] = p.last_hit[i];
}

// The medium a ray starts in, from the triangle its cast met: k_locate_material's rule (fill_state's) with the ray's own direction
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_medium(GeoView g, uint32_t nlive, const int32_t *triangle, const float *direction_in, int32_t outside, int32_t *medium)
{
    const uint32_t slot = blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    if (slot >= nlive) return;
    const int tri = triangle[slot];
    if (tri < 0 || (uint32_t)tri >= g.ntriangles) { medium[slot] = outside; return; }
    v3 direction = load3(direction_in, slot);
    direction = direction / norm(direction);
    const TriPhys r = load_tri_phys(g, (size_t)g.tri_to_dev[tri]);
    const uint32_t inner = 0xFF & (r.code >> 24), outer = 0xFF & (r.code >> 16);
    medium[slot] = (int32_t)((dot(r.normal, -direction) > 0.0f) ? outer : inner);
}

// One thread per live particle: one iteration (particles::advance_particle) on the slot's cast and medium -- no cast arrays: no
// triangle ahead, no medium array: `outside` -- and the particles still alive appended to the next queue, one atomic per wave.
// The order of that queue is the atomics'; no particle's result depends on it.
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_advance(particles::Table table, chroma_particle_options options, uint64_t seed, chroma_particle_arrays p, const uint32_t *queue,
                    uint32_t nlive, const float *distance, const int32_t *triangle, const int32_t *medium, chroma_particle_points points,
                    uint32_t *next_queue)
{
    const uint32_t slot = blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    bool alive = false;
    uint32_t i = 0;
    if (slot < nlive) {
        i = queued_particle(queue, slot);
        particles::advance_particle(table, options, seed, p, i, distance ? distance[slot] : cm_inff(), triangle ? triangle[slot] : -1,
                                    medium ? medium[slot] : options.outside, points);
        alive = p.status[i] == CHROMA_PARTICLE_ALIVE;
    }
    if (!next_queue) return;
    const unsigned long long mask = __ballot(alive);
    if (!mask) return;
    const unsigned lane = lane_id(), leader = (unsigned)__ffsll((long long)mask) - 1u;
    uint32_t first = 0;
    if (lane == leader) first = atomicAdd(next_queue, (uint32_t)__popcll(mask));          // (the tail: 1 for an empty queue)
    first = __shfl(first, (int)leader);
    if (alive) next_queue[first + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = i;
}

// counts[i] = the points of particle i less `less` (1: its segments), counts[n] = 0 for the exclusive sum to leave the total
// there, and the 64-bit total beside it
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_counts(chroma_particle_arrays p, uint32_t max_steps, uint32_t less, uint32_t *counts, unsigned long long *total)
{
    const uint64_t i = (uint64_t)blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    uint32_t mine = 0;
    if (i < p.n) counts[i] = mine = particles::points_of(p.nsteps[i], max_steps) - less;
    if (i == 0) counts[p.n] = 0u;
    const unsigned long long sum = wave_sum_u64(mine);
    if (lane_id() == 0 && sum) atomicAdd(total, sum);
}

// One thread per flat point or segment: its particle by binary search in the scanned counts, then the copy out of the matrix.
// A count that does not fit the matrix (offsets of other particle arrays) is not trusted with an address.
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_gather_points(chroma_particle_points matrix, uint32_t n, uint32_t max_steps, const uint32_t *offsets, chroma_particle_points out, uint32_t total)
{
    const uint32_t j = blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    if (j >= total) return;
    const uint32_t i = steps::find_run(offsets, n, j), k = j - offsets[i];
    if (k <= max_steps) particles::gather_point(matrix, n, i, k, out, j);
}
__global__ void __launch_bounds__(PARTICLES_BLOCK)
k_particles_gather_segments(chroma_particle_points matrix, chroma_particle_arrays p, uint32_t max_steps, const uint32_t *offsets,
                            particles::SegmentsOut out, uint32_t total)
{
    const uint32_t j = blockIdx.x * PARTICLES_BLOCK + threadIdx.x;
    if (j >= total) return;
    const uint32_t i = steps::find_run(offsets, (uint32_t)p.n, j), k = j - offsets[i];
    if (k < max_steps) particles::gather_segment(matrix, p, i, k, out, j);
}
