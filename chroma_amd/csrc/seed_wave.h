// seed_wave.h -- what a wave of the seed kernels does across its lanes: the ordering of its own LDS traffic, a 64-bit maximum and a
// 32-bit sum.  Included by kernels_seed.h (the vertex seed) and kernels_dirseed.h (the direction seed).
#pragma once

#include <stdint.h>

// what orders a wave's own LDS traffic: its clears before its adds before its reads, across lanes
__device__ __forceinline__ void seed_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t seed_wave_max(uint64_t k)
{
    for (int d = 32; d; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), d);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}
__device__ __forceinline__ uint32_t seed_wave_sum(uint32_t x) { for (int d = 32; d; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d); return x; }
