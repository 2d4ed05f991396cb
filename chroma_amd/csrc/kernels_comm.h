// kernels_comm.h -- the local half of the OR reduction across GPUs (chroma_allreduce_daq): RCCL has no bitwise OR.
// One of the kernel families of libchroma_hip.so; included by comm.hip alone, so that each kernel is compiled once.
#pragma once

__global__ void k_or_gathered(uint32_t *out, const uint32_t *gathered, uint32_t n, int nranks)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t acc = 0;
    for (int r = 0; r < nranks; r++) acc |= gathered[(size_t)r * n + i];
    out[i] = acc;
}
