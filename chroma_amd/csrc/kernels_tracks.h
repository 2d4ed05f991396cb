// kernels_tracks.h -- photon tracks recorded on the device (chroma_propagate_tracks): k_track_row0, k_track_step,
// k_track_scatter_row0, k_track_scatter.
// One of the kernel families of libchroma_hip.so; included by chroma_hip.hip (one translation unit: the families share
// device helpers and launch-time constants, and are included in dependency order).
#pragma once

// ---- photon tracks ------------------------------------------------------------------------------------
// A track (chroma/gpu/photon.py:218-238, chroma/sim.py:102-114): row 0 is the photon before the first step, and every step
// whose input queue holds the photon adds one row, its state after that step.  The streaming kernels below run BETWEEN the
// steps of the split step loop and read what the step's kernels leave behind anyway (the output working set, the input queue,
// the caller's arrays); no kernel of a step knows of them.
//
// While the call runs, rows are TRACK ROWS: 64 bytes, four float4 (the photon record's layout, device_common.h, with the two
// words a track does not need put to use):
//   {position, wavelength} {direction, time} {polarization, weight} {flags, evidx, last hit as a triangle ID, photon id}
//   rows0 [nphotons]      row 0 of photon i at i
//   slab k [n_k]          the rows of step k, n_k = the photons in its input queue: the survivors at their slot of the output
//                         working set, the photons that ended in the step behind them in any order
//   nrows [nphotons + 2]  rows of photon i (steps taken + 1), and a 0 at [nphotons]: the exclusive sum at the end of the call
//                         turns these nphotons + 1 words, in place, into `offsets` (a call holds at most 2^32 - 1 rows);
//                         the word behind them, [nphotons + 1], is k_track_step's `cursor`, zeroed before every step
// chroma_tracks_gather then puts the row of step k of photon i at offsets[i] + k + 1 of the caller's arrays.
#define TRACK_BLOCK 256

// the first `count` records staged by a wave (record r at s + 4 r) to `count` consecutive rows from row `first`: whole
// kilobytes per store instruction instead of 64 partial lines (as k_load_working)
__device__ inline void wave_store_rows(float4 *rows, size_t first, const float4 *s, uint32_t count)
{
    __builtin_amdgcn_wave_barrier();
    for (uint32_t q = lane_id(); q < 4u * count; q += WAVE) rows[4 * first + q] = s[q];
    __builtin_amdgcn_wave_barrier();
}

// photon `id` of the caller's arrays as a track row
__device__ inline void stage_track_row(float4 *s, const PhotonView &pv, size_t id, uint32_t flags)
{
    const v3 pos = load3(pv.pos, id), dir = load3(pv.dir, id), pol = load3(pv.pol, id);
    s[0] = make_float4(pos.x, pos.y, pos.z, pv.wavelengths[id]);
    s[1] = make_float4(dir.x, dir.y, dir.z, pv.t[id]);
    s[2] = make_float4(pol.x, pol.y, pol.z, pv.weights[id]);
    s[3] = make_float4(__uint_as_float(flags), __uint_as_float(pv.evidx[id]), __int_as_float(pv.last_hit_triangles[id]),
                       __uint_as_float((uint32_t)id));
}

// Row 0 of every photon, before the first step.  nrows[i]: `alive_rows` (max_steps + 1: what a photon that never ends has;
// k_track_step overwrites it for one that does), or `ended_rows` for a photon that is terminal already -- it is in the first
// step's queue and left untouched (propagate.cu:258): two equal rows, or one when no step is taken.
__global__ __launch_bounds__(TRACK_BLOCK) void
k_track_row0(PhotonView pv, uint64_t n, float4 *rows0, uint32_t *nrows, uint32_t alive_rows, uint32_t ended_rows)
{
    __shared__ float4 s_stage[TRACK_BLOCK / WAVE][WAVE * 4];
    float4 *st = s_stage[threadIdx.x / WAVE];
    for (uint64_t base = (uint64_t)blockIdx.x * TRACK_BLOCK; base < n; base += (uint64_t)gridDim.x * TRACK_BLOCK) {
        const uint64_t wave_first = base + (threadIdx.x / WAVE) * WAVE, i = base + threadIdx.x;
        if (i < n) {
            const uint32_t flags = pv.flags[i];
            stage_track_row(st + 4 * lane_id(), pv, i, flags);
            nrows[i] = (flags & CHROMA_TERMINAL_MASK) ? ended_rows : alive_rows;
        }
        const uint32_t count = wave_first < n ? (uint32_t)min((uint64_t)WAVE, n - wave_first) : 0u;
        wave_store_rows(rows0, wave_first, st, count);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) nrows[n] = 0u;
}

// The rows of one step, after its last launch.  The survivors are the records of the output working set, copied float4 by
// float4 (their last row rewritten: the triangle record to its id as k_store_working does, the draw counter to evidx).  The
// photons that ended are the entries of the input queue whose flags in the caller's arrays are terminal NOW: a photon is
// queued only while it is alive, and a call that records tracks runs without final records, so k_physics has stored it
// to the arrays.  They go behind the survivors through `cursor` (zero at launch), one atomic per wave.  Every photon of the
// input queue is one or the other, so the slab's `capacity` (the size of that queue) is filled exactly; nothing is written
// beyond it whatever the queues hold.
__global__ __launch_bounds__(TRACK_BLOCK) void
k_track_step(GeoView g, PhotonView pv, const uint32_t *in_queue, const uint32_t *out_queue, const float4 *work_out, float4 *slab,
             uint32_t capacity, uint32_t *cursor, uint32_t *nrows, uint32_t step)
{
    __shared__ float4 s_stage[TRACK_BLOCK / WAVE][WAVE * 4];
    float4 *st = s_stage[threadIdx.x / WAVE];
    const uint32_t n_in = in_queue[0] - 1u, n_out = min(out_queue[0] - 1u, capacity);
    const size_t nq = 4 * (size_t)n_out;
    for (size_t q = (size_t)blockIdx.x * TRACK_BLOCK + threadIdx.x; q < nq; q += (size_t)gridDim.x * TRACK_BLOCK) {
        float4 v = work_out[q];
        if ((q & 3u) == 3u) {
            const uint32_t id = __float_as_uint(v.w);
            const int rec = __float_as_int(v.z);
            v.y = __uint_as_float(pv.evidx[id]);
            v.z = __int_as_float(rec >= 0 ? (int)g.dev_to_tri[rec] : -1);
        }
        slab[q] = v;
    }
    for (uint64_t base = (uint64_t)blockIdx.x * TRACK_BLOCK; base < n_in; base += (uint64_t)gridDim.x * TRACK_BLOCK) {
        const uint64_t j = base + threadIdx.x;
        uint32_t id = 0, flags = 0;
        if (j < n_in) {
            id = in_queue[1 + j];
            flags = pv.flags[id];
        }
        const bool ended = (flags & CHROMA_TERMINAL_MASK) != 0;
        const unsigned long long mask = __ballot(ended);
        if (mask == 0ull) continue;                       // (the same for the whole wave)
        const unsigned lane = lane_id(), leader = (unsigned)__ffsll((long long)mask) - 1u;
        const uint32_t rnk = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        uint32_t first = 0;
        if (lane == leader) first = atomicAdd(cursor, (uint32_t)__popcll(mask));
        first = n_out + (uint32_t)__shfl(first, (int)leader);
        const uint32_t count = first < capacity ? min((uint32_t)__popcll(mask), capacity - first) : 0u;
        if (ended && rnk < count) {
            stage_track_row(st + 4 * rnk, pv, id, flags);
            nrows[id] = step + 2u;                        // (rows 0 .. step + 1)
        }
        wave_store_rows(slab, first, st, count);
    }
}

__device__ inline void store_track_row(const PhotonView &dst, size_t o, const float4 &r0, const float4 &r1, const float4 &r2, const float4 &r3)
{
    store3(dst.pos, o, mk3(r0.x, r0.y, r0.z));
    store3(dst.dir, o, mk3(r1.x, r1.y, r1.z));
    store3(dst.pol, o, mk3(r2.x, r2.y, r2.z));
    dst.wavelengths[o] = r0.w;
    dst.t[o] = r1.w;
    dst.weights[o] = r2.w;
    dst.flags[o] = __float_as_uint(r3.x);
    dst.evidx[o] = __float_as_uint(r3.y);
    dst.last_hit_triangles[o] = __float_as_int(r3.z);
}

// row 0 of photon i to offsets[i] of the caller's arrays -- and to the row behind it for a photon that was terminal before
// the first step (it has two rows then, and is in no slab); the offsets themselves to the caller's 64-bit array
__global__ __launch_bounds__(TRACK_BLOCK) void
k_track_scatter_row0(const float4 *rows0, uint64_t n, const uint32_t *offsets, PhotonView dst, uint64_t *offsets_out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TRACK_BLOCK) {
        const float4 *r = rows0 + 4 * i;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        const uint32_t o = offsets[i], end = offsets[i + 1];
        offsets_out[i] = o;
        if (i + 1 == n) offsets_out[n] = end;
        if (o >= end) continue;                            // (every photon has its row 0)
        store_track_row(dst, o, r0, r1, r2, r3);
        if ((__float_as_uint(r3.x) & CHROMA_TERMINAL_MASK) && end - o == 2u) store_track_row(dst, (size_t)o + 1, r0, r1, r2, r3);
    }
}

// the `count` rows of step `step` to their photons' tracks: row step + 1 of photon id (a row that has no place in its
// photon's track, which cannot be, is dropped)
__global__ __launch_bounds__(TRACK_BLOCK) void
k_track_scatter(const float4 *slab, uint32_t count, uint32_t step, uint64_t n, const uint32_t *offsets, PhotonView dst)
{
    for (uint64_t j = (uint64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x; j < count; j += (uint64_t)gridDim.x * TRACK_BLOCK) {
        const float4 *r = slab + 4 * j;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        const uint32_t id = __float_as_uint(r3.w);
        if (id >= n) continue;
        const uint64_t o = (uint64_t)offsets[id] + step + 1u;
        if (o < offsets[id + 1]) store_track_row(dst, o, r0, r1, r2, r3);
    }
}
