// kernel_step_control.h -- one step as separate launches: hit codes, the device-side step block (k_step_begin), the ray record
// (RayRecord, make_ray_record, k_ray_setup), what settles and retires a slot (settle_ray, retire_ray), how a wave takes rays (WorkClaim, RayFeed).
// One of the kernel families of libchroma_hip.so; included by chroma_hip.hip (one translation unit: the families share
// device helpers and launch-time constants, and are included in dependency order).
#pragma once

// ---- one step as separate launches -----------------------------------------------------------------
// The ray cast needs few registers and benefits from many resident waves; the physics needs many
// registers and little time.  A ray-cast kernel writes (triangle record, distance) per queue slot,
// k_physics consumes them.  Together they perform exactly one iteration of the loop of k_propagate
// for every queued photon, with identical arithmetic (both re-normalise dir/pol on load like
// propagate.cu:248,250 when the step opens a launch in the reference's sense, see k_step_begin).
#define HIT_SKIP (-3)      // photon already terminal: untouched (propagate.cu:258)
#define HIT_NAN  (-2)      // NaN guard fired (propagate.cu:270-273)
#define HIT_RETRY (-4)     // the ray takes the literal reference walk (k_raycast_retry)

// ---- device-side step control ---------------------------------------------------------------------
// chroma_propagate enqueues its steps without waiting for any of them: how many photons a step has
// (the tail of its input queue), whether its launch re-normalises (the reference's launch policy,
// chroma/gpu/photon.py:225-252) and the ray-cast work counters live in StepState (top of this file),
// written by k_step_begin at the head of every step and read by the step's kernels.
// `first_n` (first step of a call only, else 0): the size of the caller's arrays.  The reference decides its
// FIRST launch on pos.size, photons that are already terminal included (gpu/photon.py:207,227), and every
// later one on the survivor count; a batch that is mostly terminal already therefore still gets a
// one-step launch first and is re-normalised again by the launch after it.
__global__ void k_step_begin(const uint32_t *in_queue, uint32_t *out_queue, StepState *st, uint32_t few, uint32_t first_n)
{
    const uint32_t n = in_queue[0] - 1u;
    st->n = n;
    uint32_t renorm = 1u;
    if (st->in_tail) renorm = 0u;
    else if ((first_n ? first_n : n) < few) st->in_tail = 1u;
    st->renorm = renorm;
    if (renorm && n) st->launches++;
    st->work = 0u;
    st->retry = 0u;
    out_queue[0] = 1u;
}

// ---- ray records --------------------------------------------------------------------------------------
// What a ray cast needs of a photon, prepared once per step by a streaming kernel instead of inside the
// persistent ray-cast kernels: there the set-up of a new ray (two dependent gathers, a normalisation,
// six IEEE divisions for the slab constants, the NaN and "moderate" checks) was ~300 instructions
// executed by the whole wave for the few rays being refilled -- a quarter of the kernel's VALU work.
// Status 0 = cast; the other slots (NaN, 1/d not moderate) get their hit entry -- and their place in the retry list -- from
// whoever meets them first (settle_ray).  The photon comes from the dense working set (see k_load_working).
#define WIDE_NONE 0xFFFFFFFFu      // no wide node / an empty entry of one / the leaf word of "no last hit"

// ---- the ray record -----------------------------------------------------------------------------------------------
// 64 bytes at the queue slot, four float4 rows ("ray records"):
//   {origin, last hit} {direction, status} {a, growth} {b, 0}
// LAST HIT is the index of a triangle RECORD (-1: none), STATUS 0 or the hit code the slot is settled with.  Rows 2-3 are
//   - the fused slab constants a = scale/d and b = (world_origin - o)/d with the growth G of the boxes (ray_growth), for every
//     walk but the exact one: RayFast's blo = b - G a and bhi = b + G a are rebuilt by the reader (fast());
//   - the reference's own two per-ray constants 1/d and -o/d (mesh.h:52-53) for the exact walk (inv_dir(), noid()).
// Written by make_ray_record (k_load_working, k_physics, k_ray_setup) and k_rays_from_arrays; read by every ray-cast kernel in
// two halves -- rows 0-1, the status test, then rows 2-3 -- and by k_raycast_retry, k_physics and the distance kernels (rows 0-1).
struct RayRecord {
    float4 row[4];

    RayRecord() = default;
    __device__ inline RayRecord(v3 origin, int last_hit, v3 direction, int status, v3 a, float growth, v3 b)
    {
        row[0] = make_float4(origin.x, origin.y, origin.z, __int_as_float(last_hit));
        row[1] = make_float4(direction.x, direction.y, direction.z, __int_as_float(status));
        row[2] = make_float4(a.x, a.y, a.z, growth);
        row[3] = make_float4(b.x, b.y, b.z, 0.0f);
    }
    __device__ inline void store(float4 *r) const { r[0] = row[0]; r[1] = row[1]; r[2] = row[2]; r[3] = row[3]; }
    __device__ inline void load_head(const float4 *r) { row[0] = r[0]; row[1] = r[1]; }
    __device__ inline void load_slabs(const float4 *r) { row[2] = r[2]; row[3] = r[3]; }      // (only of a record whose status is 0)

    __device__ inline v3 origin() const { return mk3(row[0].x, row[0].y, row[0].z); }
    __device__ inline v3 direction() const { return mk3(row[1].x, row[1].y, row[1].z); }
    __device__ inline int last_hit() const { return __float_as_int(row[0].w); }
    __device__ inline int status() const { return __float_as_int(row[1].w); }
    // the last hit as the wide tree's leaf entries hold it (never entered: WIDE_NONE)
    __device__ inline uint32_t leaf_word() const { const int lh = last_hit(); return lh >= 0 ? (0x80000000u | (uint32_t)lh) : WIDE_NONE; }
    __device__ inline v3 slab_a() const { return mk3(row[2].x, row[2].y, row[2].z); }
    __device__ inline float growth() const { return row[2].w; }
    __device__ inline v3 slab_b() const { return mk3(row[3].x, row[3].y, row[3].z); }
    __device__ inline RayFast fast() const
    {
        RayFast rf;
        rf.a = slab_a();
        rf.blo = slab_b() - growth() * rf.a;
        rf.bhi = slab_b() + growth() * rf.a;
        return rf;
    }
    __device__ inline v3 inv_dir() const { return slab_a(); }
    __device__ inline v3 noid() const { return slab_b(); }
};

// a finished ray's hit entry: the record index of its triangle, -1, or a HIT_* code -- HIT_RETRY also lists the slot for
// k_raycast_retry (the short form: k_raycast_packet, which hands nothing over)
__device__ inline void retire_ray(int slot, int triangle_index, float distance, int32_t *hit_triangle, float *hit_distance)
{
    hit_triangle[slot] = triangle_index;
    hit_distance[slot] = distance;
}
__device__ inline void retire_ray(int slot, int triangle_index, float distance, int32_t *hit_triangle, float *hit_distance,
                                  uint32_t *retry_list, uint32_t *retry_counter)
{
    retire_ray(slot, triangle_index, distance, hit_triangle, hit_distance);
    if (triangle_index == HIT_RETRY) retry_list[atomicAdd(retry_counter, 1u)] = (uint32_t)slot;
}
// a slot that is not to be cast (status HIT_NAN, or HIT_RETRY: 1/d not moderate) gets its hit entry and its place in the retry list
__device__ inline void settle_ray(int status, int slot, int32_t *hit_triangle, float *hit_distance, uint32_t *retry_list, uint32_t *retry_counter)
{
    retire_ray(slot, status, 0.0f, hit_triangle, hit_distance, retry_list, retry_counter);
}

// the record of one ray at `r`; returns its status (0 = cast, HIT_NAN, HIT_RETRY)
// `literal`: the record of the exact walk (k_raycast_literal), rows 2-3 in their second meaning
__device__ inline int make_ray_record(const GeoView &g, float4 *r, v3 origin, v3 direction, int renorm, int last_hit, bool literal = false)
{
    int status;
    v3 a = mk3(0.f, 0.f, 0.f), b = mk3(0.f, 0.f, 0.f);
    if (renorm) direction = direction / norm(direction);
    if (cm_isnan(direction.x * direction.y * direction.z * origin.x * origin.y * origin.z)) {
        status = HIT_NAN;
    } else {
        v3 noid = (-origin) / direction;
        v3 inv_dir = 1.0f / direction;
        bool moderate = cm_fabsf(inv_dir.x) < 1e30f && cm_fabsf(inv_dir.y) < 1e30f && cm_fabsf(inv_dir.z) < 1e30f &&
                        cm_fabsf(noid.x) < 1e30f && cm_fabsf(noid.y) < 1e30f && cm_fabsf(noid.z) < 1e30f;
        if (!moderate) {
            status = HIT_RETRY;
        } else if (literal) {
            a = inv_dir;
            b = noid;
            status = 0;
        } else {
            a = ray_fast(g, noid, inv_dir, 1.0f).a;
            // b exactly as ray_fast forms it (blo = b - G a, bhi = b + G a are rebuilt by the kernels; G travels in r[2].w)
            b = mk3(cm_fmaf(g.world_origin[0], inv_dir.x, noid.x), cm_fmaf(g.world_origin[1], inv_dir.y, noid.y),
                    cm_fmaf(g.world_origin[2], inv_dir.z, noid.z));
            status = 0;
        }
    }
    // (RayRecord's rows written out, growth computed between them: through the struct k_load_working and k_physics compile to another
    //  schedule, profiles/r11/not_converted.txt)
    r[0] = make_float4(origin.x, origin.y, origin.z, __int_as_float(last_hit));
    r[1] = make_float4(direction.x, direction.y, direction.z, __int_as_float(status));
    r[2] = make_float4(a.x, a.y, a.z, ray_growth(g, origin));
    r[3] = make_float4(b.x, b.y, b.z, 0.0f);
    return status;
}

// With the default walk this kernel does not run at all (round 2): k_load_working writes the records of the first
// step, k_physics those of every later one -- the photon is in their registers anyway, the launch policy of the next
// step is known (re-normalise unless the reference's last launch has begun: StepState::in_tail) -- and k_raycast_quad
// settles the few slots whose status is not 0 when it meets them (`settle`).  The cross-check walks keep it.
__global__ __launch_bounds__(256) void
k_ray_setup(GeoView g, const float4 *work, const StepState *st, float4 *rays,
            int32_t *hit_triangle, float *hit_distance, uint32_t *retry_list, uint32_t *retry_counter, int literal = 0)
{
    const int nthreads = (int)st->n, renorm = (int)st->renorm;
    for (int slot = blockIdx.x * blockDim.x + threadIdx.x; slot < nthreads; slot += gridDim.x * blockDim.x) {
        const PhotonRecord rec = PhotonRecord::load(work + 4 * (size_t)slot);
        const int status = make_ray_record(g, rays + 4 * (size_t)slot, rec.position(), rec.direction(), renorm, rec.last_hit(), literal != 0);
        if (status != 0) settle_ray(status, slot, hit_triangle, hit_distance, retry_list, retry_counter);
    }
}

// ---- how a persistent ray-cast wave takes its rays: WorkClaim claims chunks, RayFeed deals a chunk's rays to idle groups ------
// Most of a launch's rays are dealt out WITHOUT the work counter: the atomics of all waves on one word run at ~1e8 per second
// (every XCD's L2 hands them on to the memory side), and at 16-64 short rays per claim that rate IS the launch -- C5's 6-node
// tree: 0.19 ns per ray at any size; a small launch: two atomics per wave, 0.1 ms (profiles/r04/ab_static_claims.txt).
// Wave b of the W that take part owns the chunks b, b + W, b + 2W, ... of the first `eighths` / 8 of its share -- at least
// one -- and only the rest, what evens the waves out, goes through the counter; a launch of at most W chunks touches no counter
// at all.  `eighths` holds two shares: bits 0-3 for launches of big chunks (5: with 7 C3's big launches wait for their slowest
// waves, +5 %), bits 4-7 for the small ones (8).  0: every chunk through the counter (rounds 1-3, and the cross-check walks).
struct WorkClaim {
    uint32_t n, chunk, left, stride, next_static, dyn_base;
    bool no_dynamic;
    __device__ WorkClaim(int nthreads, int chunk_, int eighths)
    {
        n = (uint32_t)nthreads; chunk = (uint32_t)chunk_;
        const uint32_t e = (uint32_t)((chunk_ == 16) ? (eighths >> 4) : (eighths & 15));
        const uint32_t nwaves = min((uint32_t)gridDim.x, (n + 15u) / 16u), nchunks = (n + chunk - 1u) / chunk;
        // (a share of 8/8 is the whole launch: every chunk owned, the last round of chunks by the first waves only -- a wave
        //  that must ask the counter just to learn that nothing is left costs the launch 6144 atomics, 70 us)
        left = e == 8u ? (nchunks + nwaves - 1u) / nwaves : e ? max(nchunks / nwaves * e / 8u, 1u) : 0u;
        stride = chunk * nwaves;
        dyn_base = left * stride;
        no_dynamic = e && dyn_base >= n;
        next_static = (uint32_t)blockIdx.x * chunk;
    }
    // first ray of the wave's next chunk (the caller clamps [base, base + chunk) to n); `exhausted`: there is none after it
    __device__ uint32_t next(uint32_t *counter, unsigned lane, bool &exhausted)
    {
        uint32_t base = 0;
        if (left) {
            base = next_static; next_static += stride; left--;
            if (!left && no_dynamic) exhausted = true;
        } else {
            if (lane == 0) base = atomicAdd(counter, chunk);
            base = dyn_base + (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (base + chunk >= n) exhausted = true;
        }
        return base;
    }
};

// A wave's share of the launch: the rays [loc_next, loc_end) of the chunk it holds, and the claim that gets it the next one.
// Every pass of a persistent kernel ballots its idle groups (one lane each), takes a ray for each while there are `more()`, and
// ends its node phase early enough to refill (`stop_at`).  Used by k_raycast_pair and k_raycast_wide; k_raycast_quad,
// k_raycast_literal and k_raycast_coop hold the same frame written out (profiles/r11/not_converted.txt: through the struct they
// compile to other registers or to scratch), and k_raycast_persistent claims exactly n_idle rays per atomic and so holds no chunk.
struct RayFeed {
    WorkClaim claim;
    uint32_t loc_next = 0, loc_end = 0;
    bool exhausted = false;        // wave-uniform: no chunk after the one held
    __device__ RayFeed(int nthreads, int chunk, int eighths) : claim(nthreads, chunk, eighths) {}
    __device__ bool more() const { return !exhausted || loc_next < loc_end; }
    // the ray of this lane's group, the k-th idle one taking the k-th ray (a ray only if < loc_end); `group_shift`: the group's first lane
    __device__ uint32_t take(unsigned long long idle_mask, unsigned group_shift, int n_idle, uint32_t *counter, unsigned lane)
    {
        if (loc_next >= loc_end) {
            const uint32_t base = claim.next(counter, lane, exhausted);        // (wave-uniform: scalar registers)
            loc_next = min(base, claim.n);
            loc_end = min(base + claim.chunk, claim.n);
        }
        const uint32_t idx = loc_next + (uint32_t)__popcll(idle_mask & ((1ull << group_shift) - 1ull));
        loc_next = min(loc_end, loc_next + (uint32_t)n_idle);
        return idx;
    }
    // the node phase runs until only this many groups are active: `refill_min` fewer than now while rays are left to take
    __device__ int stop_at(int n_active, int refill_min) const { return more() ? max(0, n_active - refill_min) : 0; }
};
// rays per claim: `big_chunk` when every wave gets several rounds of them anyway (a hot word serves only ~88 atomics/us), else one wave-load
__device__ inline int ray_chunk(int nthreads, int big_chunk, int rays_per_wave)
{
    return ((long long)nthreads > 4ll * big_chunk * (long long)gridDim.x) ? big_chunk : rays_per_wave;
}
