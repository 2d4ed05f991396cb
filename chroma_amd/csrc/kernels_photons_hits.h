// kernels_photons_hits.h -- photon-array kernels of chroma/cuda/propagate.cu (duplicate, count, copy, select), hit extraction.
// One of the kernel families of libchroma_hip.so; included by kernel_calls.hip alone, so that each kernel is compiled once.
#pragma once

// photon_duplicate (chroma/cuda/propagate.cu:13-52)
__global__ void k_photon_duplicate(PhotonView pv, int first_photon, int nthreads, int copies, int stride)
{
    int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nthreads) return;
    size_t photon_id = (size_t)first_photon + id;
    for (int i = 1; i <= copies; i++) copy_photon(pv, photon_id, pv, photon_id + (size_t)stride * i);
}

// count_photons (propagate.cu:54-79): grid-stride, one atomic per block
__global__ __launch_bounds__(256) void
k_count_photons(const uint32_t *flags, int first_photon, int nthreads, uint32_t target_flag, uint32_t *counter)
{
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nthreads; id += (long long)gridDim.x * blockDim.x)
        mine += (flags[first_photon + id] & target_flag) != 0;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane_id() == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_total) atomicAdd(counter, s_total);
}

__device__ inline uint32_t wave_reserve(uint32_t *counter, bool pred, bool &any)
{
    unsigned long long mask = __ballot(pred);
    any = mask != 0ull;
    if (!any) return 0;
    unsigned lane = lane_id();
    unsigned leader = (unsigned)__ffsll((long long)mask) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, (int)leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// copy_photons (propagate.cu:81-114): one atomic per block of COPY_ITEMS * 256 photons, as k_copy_hits below
__global__ __launch_bounds__(256) void
k_copy_photons(PhotonView src, PhotonView dst, int first_photon, int nthreads, uint32_t target_flag, uint32_t *counter)
{
    __shared__ uint32_t s_wave[256 / WAVE + 1];
    const long long base = (long long)blockIdx.x * (16 * 256);
    const unsigned lane = lane_id(), wave = threadIdx.x / WAVE;
    uint32_t take = 0, mine = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const long long id = base + (long long)k * 256 + threadIdx.x;
        if (id < nthreads && (src.flags[first_photon + id] & target_flag)) { take |= 1u << k; mine++; }
    }
    uint32_t incl = mine;
    for (int off = 1; off < WAVE; off <<= 1) { uint32_t v = __shfl_up(incl, off); if ((int)lane >= off) incl += v; }
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (unsigned w = 0; w < 256 / WAVE; w++) { uint32_t c = s_wave[w]; s_wave[w] = total; total += c; }
        s_wave[256 / WAVE] = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    uint32_t off = s_wave[256 / WAVE] + s_wave[wave] + incl - mine;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (take & (1u << k)) copy_photon(src, (size_t)first_photon + (size_t)(base + (long long)k * 256 + threadIdx.x), dst, off++);
}

// copy_photon_queue (propagate.cu:116-144)
__global__ void k_copy_photon_queue(PhotonView src, PhotonView dst, int first_photon, int nthreads, const uint32_t *queue)
{
    int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nthreads) return;
    size_t offset = (size_t)first_photon + id;
    copy_photon(src, queue[offset], dst, offset);
}


// count_photon_hits (propagate.cu:147-174): grid-stride, one atomic per block
__global__ __launch_bounds__(256) void
k_count_hits(GeoView g, const uint32_t *flags, const int32_t *last_hit, int first_photon, int nphotons,
             uint32_t detection_state, uint32_t *counter)
{
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nphotons; id += (long long)gridDim.x * blockDim.x)
        mine += hit_channel(g, flags[first_photon + id], last_hit[first_photon + id], detection_state) >= 0;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane_id() == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_total) atomicAdd(counter, s_total);
}

// copy_photon_hits (propagate.cu:176-214).  A block looks at COPY_ITEMS * 256 photons and reserves its
// output span with ONE atomic (the reference's one atomic per detected photon -- or one per wave -- on a
// single word costs 18 ms for 1e8 photons: a hot word serves ~88 atomics per microsecond).
__global__ __launch_bounds__(256) void
k_copy_hits(GeoView g, PhotonView src, PhotonView dst, int32_t *channels, int first_photon, int nphotons,
            uint32_t detection_state, uint32_t *counter)
{
    __shared__ uint32_t s_wave[256 / WAVE + 1];
    const long long base = (long long)blockIdx.x * (COPY_ITEMS * 256);
    const unsigned lane = lane_id(), wave = threadIdx.x / WAVE;
    int ch[COPY_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < COPY_ITEMS; k++) {
        const long long id = base + (long long)k * 256 + threadIdx.x;
        ch[k] = -1;
        if (id < nphotons) ch[k] = hit_channel(g, src.flags[first_photon + id], src.last_hit_triangles[first_photon + id], detection_state);
        mine += ch[k] >= 0;
    }
    // exclusive prefix of `mine` over the block: wave scan, then the waves' totals through LDS
    uint32_t incl = mine;
    for (int off = 1; off < WAVE; off <<= 1) { uint32_t v = __shfl_up(incl, off); if ((int)lane >= off) incl += v; }
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (unsigned w = 0; w < 256 / WAVE; w++) { uint32_t c = s_wave[w]; s_wave[w] = total; total += c; }
        s_wave[256 / WAVE] = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    uint32_t off = s_wave[256 / WAVE] + s_wave[wave] + incl - mine;
#pragma unroll
    for (int k = 0; k < COPY_ITEMS; k++) {
        if (ch[k] >= 0) {
            copy_photon(src, (size_t)first_photon + (size_t)(base + (long long)k * 256 + threadIdx.x), dst, off);
            channels[off] = ch[k];
            off++;
        }
    }
}

// per-channel hit count + earliest time (float bits; non-negative times only, cuda/daq.cu:5-20)
__global__ void k_channel_hits(GeoView g, const uint32_t *flags, const int32_t *last_hit, const float *t, uint64_t n,
                               uint32_t detection_state, uint32_t *hit_count, uint32_t *earliest)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int ch = -1;
    uint32_t tb = 0xFFFFFFFFu;
    if (i < n) {
        ch = hit_channel(g, flags[i], last_hit[i], detection_state);
        if (ch >= 0 && earliest) tb = __float_as_uint(t[i]);
    }
    // The hits of a wave that fall on ONE channel are added with one atomic (a detector of few channels -- the stress
    // geometry has one -- otherwise serialises every hit on a hot word: 4.4 ms for 3.9e5 hits); with thousands of
    // channels the lanes of a wave hardly ever agree, and each adds its own.
    const unsigned long long hitters = __ballot(ch >= 0);
    if (!hitters) return;
    const int first = __builtin_amdgcn_readlane(ch, (int)__builtin_ctzll(hitters));
    if (__ballot(ch >= 0 && ch != first) == 0ull) {
        uint32_t m = tb;
        for (int off = 32; off > 0; off >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off));
        if (lane_id() == (unsigned)__builtin_ctzll(hitters)) {
            atomicAdd(&hit_count[first], (uint32_t)__popcll(hitters));
            if (earliest) atomicMin(&earliest[first], m);
        }
    } else if (ch >= 0) {
        atomicAdd(&hit_count[ch], 1u);
        if (earliest) atomicMin(&earliest[ch], tb);
    }
}
