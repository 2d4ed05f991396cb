// kernels_daq_noise.h -- PMT dark noise of the time-binned DAQ (chroma_daq_count_pulses_noise / chroma_daq_acquire_pulses_noise;
// the contract is in include/chroma_hip.h, the draws of one word in daq_noise_common.h).  One of the kernel families of
// libchroma_hip.so; included by daq_calls.hip alone, behind kernels_daq_pulses.h.
//
// Noise photoelectrons are further entries of the pulses' pipeline: k_daq_noise_emit puts them, behind the same cursor, into the
// arrays k_daq_pulses_emit fills (key, position, charge count, time bits, history), and the sort, the heads, open, reduce and
// finish take them as they take photons.  A lane is one (row, channel) word of the call; nearly all words hold no noise, so a
// lane's work per word is one load of its channel's accept word, one Philox block and a few integer compares.
//
// The position of an entry comes from an atomic on the cursor and so may vary from run to run; the sort by key and the integer
// reductions behind it (add, or, and the minimum of the times' images) do not depend on the order of the entries of a key: the
// output is deterministic, as kernels_daq_pulses.h has it for the photons.
#pragma once

#include "daq_noise_common.h"

// what a launch needs of a chroma_daq_noise: the count table by value (the kernel's arguments: read through scalar loads)
struct DaqNoiseView {
    uint32_t count_cdf[64];
    uint32_t ncount;
    uint32_t flag;
    const uint32_t *accept;
};

// One lane's word: its row and channel, its stream with block 0 drawn, and its candidates.
struct DaqNoiseWord { uint32_t row, channel, accept, k; daq_noise::Stream stream; };

__device__ __forceinline__ DaqNoiseWord daq_noise_word(const DaqNoiseView &noise, uint32_t nchannels, uint32_t nwords, uint32_t w, uint64_t seed,
                                              uint32_t acquisition)
{
    DaqNoiseWord d;
    d.row = 0u; d.channel = 0u; d.accept = 0u; d.k = 0u;
    if (w < nwords) {
        d.row = w / nchannels;
        d.channel = w - d.row * nchannels;
        d.accept = noise.accept[d.channel];
    }
    d.stream = daq_noise::open(seed, 1u + acquisition + d.row, d.channel);
    if (d.accept) d.k = daq_noise::count(daq_noise::word(&d.stream, 0u), noise.count_cdf, noise.ncount);
    return d;
}

// The kept candidates of the wave's words, candidate by candidate: a ballot per round, as many rounds as the wave's longest
// word has candidates.  count: the wave's kept candidates.  row_noise (or NULL: not wanted, or the block lies in one row and adds
// its total once): the kept candidates per row, one add per (round, row) that has any.
__device__ __forceinline__ uint32_t daq_noise_count_wave(DaqNoiseWord &d, uint32_t lane, uint32_t *row_noise)
{
    uint32_t count = 0u;
    for (uint32_t j = 0u; __any(j < d.k); j++) {
        bool keep = false;
        if (j < d.k) keep = daq_noise::kept(daq_noise::word(&d.stream, 1u + 3u * j), d.accept);
        unsigned long long left = __ballot(keep);
        count += (uint32_t)__popcll(left);
        if (!row_noise) continue;
        while (left) {
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t row = (uint32_t)__shfl((int)d.row, leader);
            const unsigned long long same = __ballot(keep && d.row == row);
            if (lane == (uint32_t)leader) atomicAdd(row_noise + row, (uint32_t)__popcll(same));
            left &= ~same;
        }
    }
    return count;
}

// A block takes DAQ_NOISE_ITEMS runs of DAQ_PULSES_BLOCK consecutive words, lane t the word t of each run, and adds what it found to a
// shared word ONCE: with a block per 256 words a chunk of 1.7e7 words is 65 000 adds onto one address, which then cost more than
// the draws.
#define DAQ_NOISE_ITEMS 8
#define DAQ_NOISE_SPAN (DAQ_PULSES_BLOCK * DAQ_NOISE_ITEMS)

// chroma_daq_count_pulses_noise: the kept noise photoelectrons of the call's words, one add per block (64 bits: a word may
// hold 64 of them)
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void
k_daq_noise_count(DaqNoiseView noise, uint32_t nchannels, uint32_t nwords, uint64_t seed, uint32_t acquisition, unsigned long long *nkept)
{
    __shared__ uint32_t s_count[DAQ_PULSES_WAVES];
    const uint64_t block_first = (uint64_t)blockIdx.x * DAQ_NOISE_SPAN;          // (< nwords: the grid is sized so; a run may begin beyond 2^32)
    uint32_t count = 0u;          // (of the wave)
#pragma unroll 1
    for (uint32_t k = 0u; k < DAQ_NOISE_ITEMS; k++) {
        const uint64_t w = block_first + k * DAQ_PULSES_BLOCK + threadIdx.x;
        DaqNoiseWord d = daq_noise_word(noise, nchannels, nwords, (uint32_t)(w < nwords ? w : nwords), seed, acquisition);
        count += daq_noise_count_wave(d, threadIdx.x & 63u, nullptr);
    }
    if ((threadIdx.x & 63u) == 0u) s_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (int v = 0; v < DAQ_PULSES_WAVES; v++) total += s_count[v];
        if (total) atomicAdd(nkept, (unsigned long long)total);
    }
}

// The emit: the kept candidates of the block's words counted as above -- per wave, and per (wave, run) -- their places reserved by
// ONE add on the cursor k_daq_pulses_emit uses, then the runs of a wave that hold any drawn again and written: wave by wave, run by
// run, round by round, lane by lane.  `room`: the entries of the five arrays (every position is below it; checked all the same).
// row_noise: nrows words, zeroed by the caller.
__global__ __launch_bounds__(DAQ_PULSES_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void
k_daq_noise_emit(DaqNoiseView noise, chroma_daq_tables tab, chroma_daq_window win, uint32_t nchannels, uint32_t nwords, uint64_t seed,
                 uint32_t acquisition, uint32_t room, uint32_t *cursor, uint64_t *keys, uint32_t *order, uint32_t *charge_ints,
                 uint32_t *time_bits, uint32_t *histories, uint32_t *row_noise)
{
    __shared__ uint32_t s_count[DAQ_PULSES_WAVES], s_run[DAQ_PULSES_WAVES][DAQ_NOISE_ITEMS], s_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t block_first = (uint64_t)blockIdx.x * DAQ_NOISE_SPAN;          // (< nwords: the grid is sized so)
    const uint64_t block_last = min(block_first + (DAQ_NOISE_SPAN - 1u), (uint64_t)nwords - 1u);
    const uint32_t first_row = (uint32_t)block_first / nchannels;
    const bool one_row = first_row == (uint32_t)block_last / nchannels;          // the block's words are all of one row: its noise in one add
    uint32_t count = 0u;          // (of the wave)
#pragma unroll 1
    for (uint32_t k = 0u; k < DAQ_NOISE_ITEMS; k++) {
        const uint64_t w = block_first + k * DAQ_PULSES_BLOCK + threadIdx.x;
        DaqNoiseWord d = daq_noise_word(noise, nchannels, nwords, (uint32_t)(w < nwords ? w : nwords), seed, acquisition);
        const uint32_t found = daq_noise_count_wave(d, lane, one_row ? nullptr : row_noise);
        if (lane == 0u) s_run[wave][k] = found;
        count += found;
    }
    if (lane == 0u) s_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (int v = 0; v < DAQ_PULSES_WAVES; v++) total += s_count[v];
        s_base = total ? atomicAdd(cursor, total) : 0u;
        if (total && one_row) atomicAdd(row_noise + first_row, total);
    }
    __syncthreads();
    if (!count) return;          // (of the wave)
    uint32_t base = s_base;
    for (uint32_t v = 0; v < wave; v++) base += s_count[v];
#pragma unroll 1
    for (uint32_t k = 0u; k < DAQ_NOISE_ITEMS; k++) {
        if (!s_run[wave][k]) continue;          // (of the wave: most runs hold nothing and are not drawn again)
        const uint64_t w = block_first + k * DAQ_PULSES_BLOCK + threadIdx.x;
        DaqNoiseWord d = daq_noise_word(noise, nchannels, nwords, (uint32_t)(w < nwords ? w : nwords), seed, acquisition);
        const uint64_t word_key = ((uint64_t)d.row * nchannels + d.channel) * win.nbins;
        for (uint32_t j = 0u; __any(j < d.k); j++) {
            bool keep = false;
            if (j < d.k) keep = daq_noise::kept(daq_noise::word(&d.stream, 1u + 3u * j), d.accept);
            const unsigned long long in = __ballot(keep);
            const uint32_t position = base + (uint32_t)__popcll(in & ((1ull << lane) - 1ull));
            if (keep && position < room) {
                const uint32_t b = daq_noise::word(&d.stream, 2u + 3u * j), c = daq_noise::word(&d.stream, 3u + 3u * j);
                const daq_noise::Photoelectron pe = daq_noise::photoelectron(tab, win, b, c);
                keys[position] = word_key + pe.bin;
                order[position] = position;
                charge_ints[position] = pe.charge_int;
                time_bits[position] = pe.time_bits;
                histories[position] = noise.flag;
            }
            base += (uint32_t)__popcll(in);
        }
    }
}
