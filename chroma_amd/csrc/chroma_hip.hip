// chroma_hip.hip -- the propagate path of libchroma_hip.so (gfx950 / MI355X only): what a walk costs and falls back to (one row
// of WALKS each), what a chroma_propagate* call runs (CallPlan, resolved from those rows), the call itself (PropagateCall: its
// state in one object, its launches, step loop and tail as members), the settings and statistics that go with it, and the two calls that run this path's device
// code on rays of their own: chroma_intersect_mesh (the same ray-cast kernels) and the hybrid render (k_propagate's step functions:
// the compiler specialises those for their callers, so the family compiles as it did only beside k_propagate).  The other entry points of include/chroma_hip.h: context.hip, geometry.hip, kernel_calls.hip, daq_calls.hip, steps_calls.hip, comm.hip,
// bvh_device.hip, wide_device.hip.
//
// The kernels of this path live in one header per family, included below in dependency order (each family is compiled in
// this translation unit alone):
//   kernel_propagate_fused.h      k_propagate -- lane-per-photon fused multi-step kernel
//   kernel_step_control.h         hit codes, k_step_begin, RayRecord and k_ray_setup, settle_ray / retire_ray, WorkClaim and RayFeed
//   kernels_raycast_crosscheck.h  k_raycast_persistent / _wide / _coop -- cross-check walks (+ the eight-lane helpers)
//   kernel_raycast_quad.h         k_raycast_quad -- the DEFAULT ray cast
//   kernel_raycast_pair.h         k_raycast_pair -- cross-check walk
//   kernel_raycast_literal.h      k_raycast_literal -- the EXACT walk (mesh.h:42-118 for every ray), and its cast for the tail kernel
//   kernel_tail_coop.h            k_tail_coop -- the last photons' remaining steps in one launch (default and exact walk)
//   kernel_raycast_retry.h        k_raycast_retry -- the strict loop for rays the fast walks hand over
//   kernel_physics.h              k_physics
//   kernels_working_set.h         k_load_working, k_store_working
//   kernels_propagate_ends.h      the initial queue, the abort-flag reduction, k_finalize_hits
//   kernels_tracks.h              k_track_row0, k_track_step, k_track_scatter*: the rows of chroma_propagate_tracks, between the steps
//   kernels_distance.h            k_distance_to_mesh, and the fast path of chroma_intersect_mesh around k_raycast_quad
//   kernels_locate.h              chroma_locate_materials: rays of one probe direction, the material from a ray's hit
//   kernels_hybrid_render.h       the hybrid render: k_propagate's step functions, one lane per sample
//   experimental/*.h              measured-and-not-faster kernels: ONLY in build_variants/libchroma_hip_experimental.so
// See DESIGN.md for the data layout and what bounds each kernel.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#ifndef CHROMA_EXPERIMENTAL
#define CHROMA_EXPERIMENTAL 0      // 1: build_variants/libchroma_hip_experimental.so (csrc/experimental/: packet ray cast, dealt physics, autosort)
#endif
#ifndef CHROMA_HYBRID_RENDER
#define CHROMA_HYBRID_RENDER 1     // 0 only for tests/test_hybrid_isa.py: the other kernels compiled without the hybrid render's
#endif
#include "chroma_internal.h"
#include "propagate_device.h"

// ---------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------
#include "kernel_propagate_fused.h"

#include "kernel_step_control.h"

#include "kernels_raycast_crosscheck.h"

#include "kernel_raycast_quad.h"

#include "kernel_raycast_pair.h"

#if CHROMA_EXPERIMENTAL
#include "experimental/raycast_packet.h"
#endif

#include "kernel_raycast_literal.h"

#include "kernel_tail_coop.h"

#include "kernel_raycast_retry.h"

#include "kernel_physics.h"

#if CHROMA_EXPERIMENTAL
#include "experimental/physics_deal.h"
#else
#define PHYS_DEAL 0
#define PHYS_DEAL_BLOCK 512
#endif

#include "kernels_working_set.h"

#include "kernels_propagate_ends.h"

#include "kernels_tracks.h"

#include "kernels_distance.h"

#include "kernels_locate.h"

#if CHROMA_HYBRID_RENDER
#include "kernels_hybrid_render.h"
#endif

// ---------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------
// the reference's tree with STACK_LDS entries in LDS and the rest in scratch: k_propagate, the persistent cast and the strict
// retry loop walk it, so every call may
static int check_stack(const chroma_geometry *geom)
{
    if (geom->stack_need <= STACK_LDS + STACK_SCRATCH) return CHROMA_OK;
    return set_error(CHROMA_ERR_STACK, "BVH needs %u traversal stack entries, more than the %d supported", geom->stack_need,
                     STACK_LDS + STACK_SCRATCH);
}

// The ray cast of a device step.  The exact walks run the reference's own loop for every ray (mesh.h:42-118 as it stands:
// its tree, its order, its box arithmetic, every triangle tested the moment its leaf box is entered) and k_physics takes
// their results as they are: LITERAL with four lanes per ray (k_raycast_literal) and the strict lane-per-ray loop for the few
// rays whose 1/d is not moderate, LITERAL_LANE with the strict loop for every ray (the cross-check).  The others walk the
// wide tree (WIDE 1, COOP 8, QUAD 4, PAIR 2 lanes per ray) or the reference's tree (PERSISTENT) and hand the rays they cannot
// settle to k_raycast_retry.  A Cast has the number of its CHROMA_WALK_*.
enum class Cast { PERSISTENT, WIDE, COOP, QUAD, PAIR, LITERAL, LITERAL_LANE };
enum SpillKind : unsigned { SPILL_NONE = 0, SPILL_COOP = 1, SPILL_WIDE = 2 };

// Everything the host knows about a walk, one row per CHROMA_WALK_* in the order of their numbers.
struct Walk {
    const char *name, *alias;      // what CHROMA_WALK accepts
    Cast cast;                     // the kernel of a device step
    int rays_per_wave;             // one wave per so many rays ...
    int waves_per_cu;              // ... up to the kernel's resident waves: a CU holds this many
    const char *waves_env;         // ... unless this variable says otherwise (at least 1)
    uint32_t stack;                // the deepest wide tree its stack holds, LDS part + global spill; 0: it walks the reference's tree (check_stack)
    SpillKind spill;               // the context's buffer behind the global part of its stack
    int fallback;                  // the walk that takes its place when the wide tree is deeper than `stack`
    bool chain;                    // the ray records go from kernel to kernel (k_load_working -> ray cast -> k_physics -> ...): no k_ray_setup
    bool tail;                     // under CHROMA_TAIL_COOP it hands the last photons to k_tail_coop (the cross-check walks keep per-step launches to the end)
};
static const Walk WALKS[] = {
    // (waves per CU: LDS-limited residency with 8 KB per wave | 11 KB per wave | 71 VGPRs, amdgpu_waves_per_eu 7 | the kernels' own attribute)
    {"reference", nullptr, Cast::PERSISTENT, PROP_BLOCK, 20, "CHROMA_RAY_WAVES_PER_CU", 0, SPILL_NONE, -1, false, false},
    {"wide", nullptr, Cast::WIDE, PROP_BLOCK, 14, "CHROMA_WIDE_WAVES_PER_CU", WIDE_STACK + WIDE_SPILL, SPILL_WIDE, CHROMA_WALK_REFERENCE, false, false},
    {"coop", nullptr, Cast::COOP, 8, 28, "CHROMA_COOP_WAVES_PER_CU", COOP_STACK + COOP_SPILL, SPILL_COOP, CHROMA_WALK_WIDE, false, true},
    {"quad", nullptr, Cast::QUAD, 16, 4 * QUAD_WAVES_PER_EU, "CHROMA_QUAD_WAVES_PER_CU", QUAD_STACK + COOP_SPILL, SPILL_COOP, CHROMA_WALK_COOP, true, true},
    {"pair", nullptr, Cast::PAIR, 32, 4 * PAIR_WAVES_PER_EU, "CHROMA_PAIR_WAVES_PER_CU", PAIR_STACK + COOP_SPILL, SPILL_COOP, CHROMA_WALK_QUAD, false, true},
    // (the exact walks never fall back; k_raycast_literal has the quad kernel's grid and its slice of the coop spill buffer)
    {"literal", "exact", Cast::LITERAL, 16, 4 * QUAD_WAVES_PER_EU, "CHROMA_QUAD_WAVES_PER_CU", 0, SPILL_COOP, -1, true, true},
    {"literal_lane", nullptr, Cast::LITERAL_LANE, PROP_BLOCK, 20, "CHROMA_RAY_WAVES_PER_CU", 0, SPILL_NONE, -1, false, false},
};
static const int NWALKS = sizeof WALKS / sizeof WALKS[0];
static_assert(NWALKS == CHROMA_WALK_LITERAL_LANE + 1, "one row per CHROMA_WALK_*");

// whether the walk's stack holds the geometry's tree
static bool walk_fits(const Walk &w, const chroma_geometry *geom)
{
    return w.stack == 0 || (geom->view.wnodes != nullptr && geom->wide_stack_need <= w.stack);
}

// What one call runs, fixed when it starts: the context's settings (chroma_set_walk / _tail / _packet / _autosort / _counting,
// the CHROMA_* environment) overridden by the call's own chroma_propagate_options, resolved against the geometry through the
// rows of WALKS.  Every function below a public entry point reads THIS (a propagate call: inside its PropagateCall), never
// the context's mutable settings, so a call cannot change under it.
struct CallPlan {
    int tail_mode;       // CHROMA_TAIL_*
    bool counting;
    Cast cast;           // what every device step runs: the chosen walk's, or that of the walk it fell back to
    bool chain;          // Walk::chain of the chosen walk, when it did not fall back
    bool tail_watch;     // near the end the host reads the survivor count every step, to start the tail when the reference does
    bool tail;           // ... and k_tail_coop can walk this geometry: it takes the last photons
    bool isect_quad;     // chroma_intersect_mesh casts with k_raycast_quad
    unsigned spill;      // SpillKind buffers the steps and the tail use
    int packet;          // experimental: k_raycast_packet offered for the first step (chroma_set_packet's mode), or 0
    int autosort;        // experimental: chroma_set_autosort's mode, or 0
};

// `walk`, `tail`, `counting`: the call's choice, or -1 for the context's
static int make_plan(const CallState &cs, const chroma_geometry *geom, int walk, int tail, int counting, CallPlan *plan)
{
    if (walk >= NWALKS) return set_error(CHROMA_ERR_INVALID, "unknown walk mode %d", walk);
    if (tail > CHROMA_TAIL_FUSED) return set_error(CHROMA_ERR_INVALID, "unknown tail mode %d", tail);
    const int w = walk >= 0 ? walk : cs.walk;
    CallPlan p = {};
    p.tail_mode = tail >= 0 ? tail : cs.tail_mode;
    p.counting = counting >= 0 ? counting != 0 : cs.counting != 0;
    // a fast walk whose stack is too shallow for the tree falls back to the next one (PAIR never to COOP)
    int r = w;
    while (!walk_fits(WALKS[r], geom)) {
        r = WALKS[r].fallback;
        if (w == CHROMA_WALK_PAIR && r == CHROMA_WALK_COOP) r = WALKS[r].fallback;
    }
    p.cast = WALKS[r].cast;
    // (a PAIR walk that fell back to the quad kernel keeps the k_ray_setup pass)
    p.chain = r == w && WALKS[w].chain;
    // (k_tail_coop and the quad cast of chroma_intersect_mesh have the coop walk's stack)
    const bool fits_coop = walk_fits(WALKS[CHROMA_WALK_COOP], geom);
    p.tail_watch = p.tail_mode == CHROMA_TAIL_COOP && WALKS[w].tail;
    p.tail = p.tail_watch && fits_coop;
    p.isect_quad = fits_coop && WALKS[w].stack != 0;
    if (p.tail_mode != CHROMA_TAIL_FUSED) p.spill = WALKS[r].spill | (p.tail ? SPILL_COOP : SPILL_NONE);
    if (p.chain && p.cast == Cast::QUAD) {
        p.autosort = cs.autosort_mode;
#if CHROMA_EXPERIMENTAL
        if (geom->wide_stack_need <= PACKET_STACK) p.packet = cs.packet_mode;
#endif
    }
    *plan = p;
    return CHROMA_OK;
}

// the global-memory parts of the fast walks' stacks, allocated at first use.  Every cooperative walk indexes the coop one
// with (wave * rays-per-wave + ray) * COOP_SPILL, so it is sized for the largest grid of any of them.
static int ensure_spill(const CallScope &scope, unsigned kinds)
{
    chroma_ctx *ctx = scope.ctx; CallState &cs = scope.state();
    const struct { SpillKind kind; uint2 **buf; size_t depth; } bufs[] = {{SPILL_COOP, &cs.coop_spill, COOP_SPILL},
                                                                          {SPILL_WIDE, &cs.wide_spill, WIDE_SPILL}};
    for (const auto &b : bufs) {
        if (!(kinds & b.kind) || *b.buf) continue;
        size_t rays = 0;
        for (const Walk &w : WALKS)
            if (w.spill == b.kind) rays = std::max(rays, (size_t)ctx->waves[(int)w.cast] * w.rays_per_wave);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(ctx_malloc(ctx, (void **)b.buf, rays * b.depth * sizeof(uint2)));
    }
    return CHROMA_OK;
}

// the ray cast's grid: one wave per Walk::rays_per_wave rays, up to the kernel's resident waves
static unsigned cast_waves(const chroma_ctx *ctx, Cast cast, long long n)
{
    const long long per = WALKS[(int)cast].rays_per_wave;
    return (unsigned)std::min<long long>((n + per - 1) / per, ctx->waves[(int)cast]);
}

// the lane-per-photon kernel with the reference's launch shape (CHROMA_TAIL=fused, chroma_propagate_step)
struct FusedLaunch { int first, nthreads; const uint32_t *in_q; uint32_t *out_q; int max_steps, use_weights, scatter_first; };
static int launch_propagate(const CallScope &scope, bool counting, chroma_geometry *geom, const PhotonView &pv, chroma_rng rng, const FusedLaunch &a)
{
    chroma_ctx *ctx = scope.ctx;
    const dim3 grid((unsigned)((a.nthreads + PROP_BLOCK - 1) / PROP_BLOCK)), block(PROP_BLOCK);
    with_bool(counting, [&](auto C) {
        hipLaunchKernelGGL((k_propagate<STACK_LDS, C>), grid, block, 0, ctx->stream, geom->view, pv, a.first, a.nthreads, a.in_q, a.out_q,
                           rng.seed, rng.photon_id_base, a.max_steps, a.use_weights, a.scatter_first, scope.state().d_counters);
    });
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// the kernels' counters since the last read, added to *stats; the counters start again at zero
static int stats_read(const CallScope &scope, chroma_propagate_stats *stats)
{
    chroma_ctx *ctx = scope.ctx; CallState &cs = scope.state();
    DeviceCounters c;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(&c, cs.d_counters, sizeof c, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(cs.d_counters, 0, sizeof c));
    stats->photon_steps += c.photon_steps;
    stats->nodes_visited += c.nodes_visited;
    stats->triangles_tested += c.triangles_tested;
    stats->stack_overflows += c.stack_overflows;
    stats->stack_spills += c.stack_spills;
    stats->packet_rays += c.packet_rays;
    stats->packet_nodes_visited += c.packet_nodes;
    stats->packet_triangles_tested += c.packet_tris;
    return CHROMA_OK;
}

// the timing events of one step, in the order they are recorded (EV_PER_STEP per step when a call times its kernels)
enum { EV_STEP_BEGIN, EV_PACKET_BEGIN, EV_CAST_BEGIN, EV_CAST_END, EV_PHYSICS_END, EV_STEP_END, EV_PER_STEP };

// The rows of one chroma_propagate_tracks call (kernels_tracks.h), all from the context's pool: row 0 of every photon, one slab
// per step run, and the rows per photon that the call's last launch turns into offsets.
struct chroma_tracks {
    struct Slab { float4 *rows; uint32_t count; };
    uint64_t nphotons = 0, nrows = 0;
    float4 *rows0 = nullptr;               // [nphotons][4]
    uint32_t *offsets = nullptr;           // [nphotons + 1] rows per photon while the call runs, their exclusive sum after it; [nphotons + 1] is k_track_step's cursor
    std::vector<Slab> slabs;               // slab k: the rows of step k
};

static void tracks_release(chroma_ctx *ctx, chroma_tracks *tr)
{
    if (!tr) return;
    for (const chroma_tracks::Slab &s : tr->slabs) chroma_free(ctx, s.rows);       // (parked until the stream has passed this point)
    chroma_free(ctx, tr->rows0);
    chroma_free(ctx, tr->offsets);
    delete tr;
}

namespace { struct PropagateCall; }
// *d_order: nullptr (the call takes its photons as they come) or a chroma_malloc'ed permutation to free after k_load_working
static int propagate_order(PropagateCall &call, uint32_t **d_order);

// One chroma_propagate* call: its entry point's scope and the CallState behind it, what it was asked, what it runs (CallPlan),
// the context's buffers in the roles they have at the moment, and what it has found out so far.  Built once by propagate_impl after its checks; the functions of the path are its
// members and take only what varies from one invocation to the next.  The context's own pointers and settings are not changed
// by a call: the pairs below swap HERE.  (Unnamed namespace: its members are not the library's symbols.)
namespace {
struct PropagateCall {
    const CallScope &scope; CallState &cs;
    chroma_ctx *ctx; chroma_geometry *geom;
    CallPlan plan;
    PhotonView pv; chroma_rng rng; chroma_propagate_options opt;
    uint64_t nphotons; uint32_t ncopies;
    uint32_t *in_q, *out_q;            // whole queues (slot 0 = tail): this step's input and output
    float4 *work_in, *work_out;        // ... and the dense working sets that go with them
    float4 *rays, *rays_next;          // ray records: this step's, and where a chaining k_physics writes the next step's
    float4 *final_rec;                 // the context's final records when this call uses them, else NULL (k_physics stores to the arrays)
    uint32_t final_epoch;              // ... and what marks a record as this call's
    HitsOut ho;                        // where the call's last pass (k_finalize_hits) puts the hits ...
    bool finalize;                     // ... if it runs at all: a hits request, or final records
    chroma_propagate_stats acc;        // launches and kernel times so far
    long long n_upper;                 // bounds the live photons: sizes the grids
    bool finalized;                    // k_finalize_hits has run already, beside the tail kernel (launch_tail)
    chroma_tracks *tracks;             // chroma_propagate_tracks: where the call records its rows, else NULL

    hipEvent_t *events(int step) const { return opt.time_kernels ? cs.step_events.data() + EV_PER_STEP * step : nullptr; }

    // the live photons into the dense working set (k_load_working), with the first step's ray records when the rays chain
    int load_working()
    {
        const unsigned blocks = (unsigned)std::min<uint64_t>((nphotons + PHYS_BLOCK - 1) / PHYS_BLOCK, (uint64_t)ctx->physics_blocks);
        int rc = scope.clear_words(W_PACKET_USE, W_PACKET_END - W_PACKET_USE); if (rc) return rc;
        uint32_t *d_order = nullptr;
        rc = propagate_order(*this, &d_order); if (rc) return rc;
        hipLaunchKernelGGL(k_load_working, dim3(blocks), dim3(PHYS_BLOCK), 0, ctx->stream, geom->view, pv, in_q, work_in,
                           (uint64_t)nphotons, ncopies, (uint32_t)(nphotons / ncopies), plan.chain ? rays : nullptr,
                           plan.packet == 2 ? cs.d_words + W_PACKET_COHERENT : nullptr, (const uint32_t *)d_order, plan.cast == Cast::LITERAL ? 1 : 0);
        if (d_order) { chroma_free(ctx, d_order); acc.reordered += nphotons; }      // (parked until the stream has passed this point)
#if CHROMA_EXPERIMENTAL
        if (plan.packet)
            hipLaunchKernelGGL(k_packet_decide, dim3(1), dim3(1), 0, ctx->stream, cs.d_words + W_PACKET_COHERENT, cs.d_words + W_PACKET_USE,
                               (uint64_t)nphotons, plan.packet);
#endif
        HIP_TRY(hipGetLastError());
        return CHROMA_OK;
    }

    // (with weights the reference runs ALL steps in one launch: every count is "few"; when it tracks, one step per launch
    //  to the end, also with weights -- chroma/gpu/photon.py:218-238 --: no count is)
    void launch_step_begin(uint32_t first_n)
    {
        hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(1), 0, ctx->stream, in_q, out_q, cs.d_step,
                           tracks ? 0u : opt.use_weights ? 0xFFFFFFFFu : (uint32_t)(PROP_BLOCK * 16 * 8), first_n);
    }

    // k_physics for one pass of a step.  `fixup`: 0 the main pass over every slot, 1 the slots k_raycast_retry has walked again
    // (a short list: a small grid), 2 every slot with the ray cast's results taken as they are (the exact walks).
    void launch_physics(int scatter_first, int fixup)
    {
        StepState *st = cs.d_step;
        float4 *chained = plan.chain ? rays_next : nullptr;
        const bool plain = geom->view.plain_optics != 0;      // (no re-emitting component, default surface model only)
        bool deal = false;
#if PHYS_DEAL
        deal = plain && !final_rec;                           // (photons of a block dealt by what happens to them: experimental/physics_deal.h)
#endif
        const int pb = deal ? PHYS_DEAL_BLOCK : PHYS_BLOCK_OF(!plain);
        unsigned blocks = (unsigned)std::min<long long>((n_upper + pb - 1) / pb, std::max<long long>(1, (long long)ctx->physics_blocks * PHYS_BLOCK / pb));
        // (the retry list is ~1e-3 of the slots with plain optics: an eighth of the grid strides over it in a round or two, and a
        //  launch of 2048 blocks that find nothing to do costs 0.07 ms, 29 times per batch; a plain geometry with faces on the
        //  world box lists a good part of its hits for the exact check, so not less than that)
        if (fixup == 1 && plain) blocks = std::max(std::min(blocks, 64u), blocks / 8);
        DeviceCounters *pc = plan.counting ? cs.d_counters : nullptr;
#if PHYS_DEAL
        if (deal) {
            hipLaunchKernelGGL(k_physics_deal, dim3(blocks), dim3(PHYS_DEAL_BLOCK), 0, ctx->stream, geom->view, pv, st, work_in, out_q, work_out,
                               cs.hit_triangle, cs.hit_distance, rng.seed, rng.photon_id_base, opt.use_weights, scatter_first,
                               cs.retry_list, fixup, pc, chained);
            return;
        }
#endif
        const int literal_rays = fixup == 2 ? 1 : 0;          // (the exact walks' ray records)
        with_bool(!plain, [&](auto FULL) {
            hipLaunchKernelGGL((k_physics<FULL>), dim3(blocks), dim3(PHYS_BLOCK_OF(FULL)), 0, ctx->stream, geom->view, pv, st, work_in, out_q,
                               work_out, cs.hit_triangle, cs.hit_distance, rng.seed, rng.photon_id_base, opt.use_weights, scatter_first,
                               cs.retry_list, fixup, pc, chained, final_rec, final_epoch, literal_rays);
        });
    }

    // One step as ray set-up + ray cast + physics (+ the strict walk and the physics of the few rays that need it), all reading the
    // photon count and the launch policy from the step block (k_step_begin).  `ev`: the step's EV_PER_STEP events, or NULL.  When the
    // rays chain, this step's records are in `rays` already (written by k_load_working or by the k_physics of the step before),
    // k_physics writes the next step's to `rays_next`, and the two swap.
    // `packet` (experimental): the first step of a call whose k_load_working looked at the photons' coherence -- k_raycast_packet
    // is launched before k_raycast_quad, and the word k_packet_decide wrote tells the two which of them has the step.
    int launch_split_step(int scatter_first, hipEvent_t *ev, uint32_t first_n, bool packet)
    {
        if (n_upper <= 0) return CHROMA_OK;
        StepState *st = cs.d_step;
        const Cast cast = plan.cast;
        const bool exact = cast == Cast::LITERAL || cast == Cast::LITERAL_LANE;
        const dim3 block(PROP_BLOCK);
        auto record = [&](int slot) { return ev ? hipEventRecord(ev[slot], ctx->stream) : hipSuccess; };
        // (both passes of the strict walk stride over the list and leave at once when it is short -- the usual case -- but a plain
        //  geometry with faces on the world box lists a good part of its hits for the exact check: grids for that)
        const unsigned rblocks = (unsigned)std::min<long long>((n_upper + PROP_BLOCK - 1) / PROP_BLOCK, 8 * 256);
        auto retry = [&](auto C) {
            hipLaunchKernelGGL((k_raycast_retry<C>), dim3(rblocks), block, 0, ctx->stream, geom->view, rays, st, cs.hit_triangle,
                               cs.hit_distance, cs.retry_list, cs.d_counters);
        };
        launch_step_begin(first_n);
        HIP_TRY(record(EV_STEP_BEGIN));
        if (!plan.chain) {
            unsigned sblocks = (unsigned)std::min<long long>((n_upper + 255) / 256, (long long)ctx->physics_blocks * 4);
            hipLaunchKernelGGL(k_ray_setup, dim3(sblocks), dim3(256), 0, ctx->stream, geom->view, work_in, st, rays,
                               cs.hit_triangle, cs.hit_distance, cs.retry_list, &st->retry, cast == Cast::LITERAL ? 1 : 0);
        }
        HIP_TRY(record(EV_PACKET_BEGIN));                             // the ray-cast kernels proper are timed from here
        const uint32_t *skip_quad = nullptr;
#if CHROMA_EXPERIMENTAL
        if (packet) {
            skip_quad = cs.d_words + W_PACKET_USE;
            const unsigned pwaves = (unsigned)std::min<long long>((n_upper + WAVE - 1) / WAVE, (long long)ctx->waves[(int)Cast::QUAD]);
            with_bool(plan.counting, [&](auto C) {
                hipLaunchKernelGGL((k_raycast_packet<C>), dim3(pwaves), block, 0, ctx->stream, geom->view, rays, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.d_counters, cs.d_words + W_PACKET_USE);
            });
        }
#else
        (void)packet;
#endif
        HIP_TRY(record(EV_CAST_BEGIN));
        const dim3 grid(cast_waves(ctx, cast, n_upper));
        const int chained = plan.chain ? 1 : 0;
        with_bool(plan.counting, [&](auto C) {
            switch (cast) {
            case Cast::PAIR:
                hipLaunchKernelGGL((k_raycast_pair<C>), grid, block, 0, ctx->stream, geom->view, rays, 0, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.coop_spill, cs.d_counters, ctx->coop_chunk);
                break;
            case Cast::QUAD:
                hipLaunchKernelGGL((k_raycast_quad<C>), grid, block, 0, ctx->stream, geom->view, rays, 0, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.coop_spill, cs.d_counters, ctx->coop_chunk, chained, skip_quad,
                                   ctx->claim_static);
                break;
            case Cast::COOP:
                hipLaunchKernelGGL((k_raycast_coop<C>), grid, block, 0, ctx->stream, geom->view, rays, 0, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.coop_spill, cs.d_counters, ctx->coop_chunk);
                break;
            case Cast::WIDE:
                hipLaunchKernelGGL((k_raycast_wide<C>), grid, block, 0, ctx->stream, geom->view, rays, 0, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.wide_spill, cs.d_counters, ctx->ray_chunk);
                break;
            case Cast::PERSISTENT:
                hipLaunchKernelGGL((k_raycast_persistent<C>), grid, block, 0, ctx->stream, geom->view, rays, 0, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.d_counters);
                break;
            case Cast::LITERAL:
                hipLaunchKernelGGL((k_raycast_literal<C>), grid, block, 0, ctx->stream, geom->view, rays, st, cs.hit_triangle,
                                   cs.hit_distance, cs.coop_spill, cs.d_counters, ctx->coop_chunk, chained, cs.retry_list,
                                   ctx->claim_static);
                retry(C);
                break;
            case Cast::LITERAL_LANE:
                hipLaunchKernelGGL((k_raycast_retry<C, true>), grid, block, 0, ctx->stream, geom->view, rays, st, cs.hit_triangle,
                                   cs.hit_distance, cs.retry_list, cs.d_counters);
                break;
            }
        });
        HIP_TRY(record(EV_CAST_END));
        // physics for every slot whose hit is regular; then the strict walk and the physics of the rest
        launch_physics(scatter_first, exact ? 2 : 0);
        HIP_TRY(record(EV_PHYSICS_END));
        if (!exact) {
            with_bool(plan.counting, retry);
            launch_physics(scatter_first, 1);
        }
        HIP_TRY(record(EV_STEP_END));
        HIP_TRY(hipGetLastError());
        if (plan.chain) std::swap(rays, rays_next);              // (what k_physics wrote is the next step's input)
        return CHROMA_OK;
    }

    // All remaining `nsteps` steps of the last photons in one launch (k_tail_coop), for a plan with `tail`.  Sets *done when it launched.
    int launch_tail(int nsteps, int scatter_first, hipEvent_t *ev, uint32_t first_n, bool *done)
    {
        // (a call that ends in k_finalize_hits: that pass runs on the context's auxiliary stream WHILE the tail kernel
        //  finishes the last photons, which are stamped first so that it leaves them to the tail kernel; the two meet again
        //  before the call reads its result words.  The tail kernel is launched FIRST: its ~1000 waves are resident before the
        //  24 000 blocks of the streaming pass fill every wave slot.  Launched second, its workgroups waited for slots behind them
        //  and the tail ended 1.7 ms after the pass instead of with it: DESIGN.md section 3.2)
        *done = false;
        const unsigned waves = cast_waves(ctx, Cast::COOP, n_upper);            // (8 lanes per photon)
        if ((long long)waves * 8 < n_upper) return CHROMA_OK;          // (cannot happen below 8192 photons)
        launch_step_begin(first_n);
        HitsOut beside; memset(&beside, 0, sizeof beside);
        uint32_t *words = nullptr;
        if (finalize) {
            beside = ho;
            words = cs.d_words;
            int rc = scope.clear_results(); if (rc) return rc;
            if (final_rec)
                hipLaunchKernelGGL(k_mark_tail, dim3(32), dim3(256), 0, ctx->stream, in_q, final_rec, photon_tail_stamp(final_epoch));
            HIP_TRY(hipEventRecord(cs.ev_fork, ctx->stream));          // (the words are cleared and the tail's photons stamped: the pass may start)
        }
        if (ev) HIP_TRY(hipEventRecord(ev[EV_STEP_BEGIN], ctx->stream));
        with_bool(plan.cast == Cast::LITERAL, [&](auto L) {
            with_bool(plan.counting, [&](auto C) {
                hipLaunchKernelGGL((k_tail_coop<C, L>), dim3(waves), dim3(PROP_BLOCK), 0, ctx->stream, geom->view, pv, cs.d_step, work_in,
                                   rng.seed, rng.photon_id_base, nsteps, opt.use_weights, scatter_first, cs.coop_spill, cs.d_counters, beside, words);
            });
        });
        if (ev) HIP_TRY(hipEventRecord(ev[EV_STEP_END], ctx->stream));
        if (finalize) {
            HIP_TRY(hipStreamWaitEvent(cs.aux_stream, cs.ev_fork, 0));
            launch_finalize(cs.aux_stream, photon_tail_stamp(final_epoch));
            HIP_TRY(hipEventRecord(cs.ev_join, cs.aux_stream));
            HIP_TRY(hipStreamWaitEvent(ctx->stream, cs.ev_join, 0));
            finalized = true;              // (the tail kernel writes every photon it held back)
        }
        HIP_TRY(hipGetLastError());
        *done = true;
        return CHROMA_OK;
    }

    // k_finalize_hits: the records to the caller's arrays, the abort word, the hit count, the compacted hits, the per-channel arrays
    void launch_finalize(hipStream_t stream, uint32_t tail_mark)
    {
        const unsigned blocks = (unsigned)((nphotons + COPY_ITEMS * 256 - 1) / (COPY_ITEMS * 256));
        hipLaunchKernelGGL(k_finalize_hits, dim3(blocks), dim3(256), 0, stream, geom->view, pv, (const float4 *)final_rec, final_epoch,
                           (uint64_t)nphotons, ho, cs.d_words, tail_mark);
    }

    // kernel, ray-cast, packet and physics times of a call's first `steps` steps from their events (time_kernels)
    int read_step_times(int steps, int tail_step)
    {
        for (int k = 0; k < steps; k++) {
            const hipEvent_t *ev = events(k);
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[EV_STEP_BEGIN], ev[EV_STEP_END]));
            acc.kernel_ms += ms;
            if (k == tail_step) continue;             // the fused tail is not a ray-cast launch
            HIP_TRY(hipEventElapsedTime(&ms, ev[EV_CAST_BEGIN], ev[EV_CAST_END]));
            acc.raycast_ms += ms;
            acc.raycast_launches++;
            if (k == 0 && plan.packet) {              // the first step's k_raycast_packet launch (an empty one when the photons are not coherent)
                HIP_TRY(hipEventElapsedTime(&ms, ev[EV_PACKET_BEGIN], ev[EV_CAST_BEGIN]));
                acc.packet_ms += ms;
                acc.packet_launches++;
            }
            HIP_TRY(hipEventElapsedTime(&ms, ev[EV_CAST_END], ev[EV_PHYSICS_END]));
            acc.physics_ms += ms;                    // the main pass of k_physics (not the fix-up pass)
            acc.physics_launches++;
        }
        return CHROMA_OK;
    }

    // Launch policy of the reference (chroma/gpu/photon.py:225-252): one step per launch while many
    // photons are alive, and ONE launch for all remaining steps once fewer than 64*16*8 are left (or
    // with weights).  A launch re-normalises dir/pol when it loads a photon (propagate.cu:248,250), so
    // the policy is part of the arithmetic.  Here every step is a ray cast + physics pair that gets the
    // whole chip; a step that the reference would run inside its last launch skips the re-normalisation
    // instead (same numbers; with weights that is every step but the first).  The policy is evaluated ON
    // THE DEVICE (k_step_begin), so the steps are enqueued back to back; the host looks at the survivor
    // count only now and then, to stop early, to shrink the grids and to hand the last photons to the
    // fused tail kernel.  The live photons travel in the dense working set (k_load_working).
    int run_device_steps()
    {
        const int max_steps = opt.max_steps;
        HIP_TRY(hipMemsetAsync(cs.d_step, 0, sizeof(StepState), ctx->stream));
        hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, in_q, 1u);
        hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, out_q, 1u);
        int rc = load_working(); if (rc) return rc;
        const int nev = opt.time_kernels ? EV_PER_STEP * max_steps : 0;
        while ((int)cs.step_events.size() < nev) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); cs.step_events.push_back(e); }
        const long long few = (long long)PROP_BLOCK * 16 * 8;
        int step = 0, next_check = 1, tail_step = -1;          // (tail_step: the step at which the fused tail was launched)
        bool done = false;
        while (step < max_steps && !done) {
            const int scatter_first = step == 0 ? opt.scatter_first : 0;
            const uint32_t first_n = step == 0 ? (uint32_t)nphotons : 0u;
            if (plan.tail && n_upper < few) {
                // the reference's last launch: all remaining steps at once, 8 lanes per photon
                rc = launch_tail(max_steps - step, scatter_first, events(step), first_n, &done); if (rc) return rc;
                if (done) { tail_step = step++; break; }
            }
            rc = launch_split_step(scatter_first, events(step), first_n, step == 0 && plan.packet != 0); if (rc) return rc;
            step++;
            std::swap(in_q, out_q);
            std::swap(work_in, work_out);
            if (step == next_check && step < max_steps) {
                // survivors = tail - 1 of what is now the input queue
                rc = scope.read_survivors(in_q, &n_upper); if (rc) return rc;
                if (n_upper <= 0) done = true;
                // look every step once the tail is near, so that it starts when the reference's does
                next_check = (plan.tail_watch && n_upper < 16 * few) ? step + 1 : (step < 8) ? step * 2 : step + 8;
            }
        }
        if (!done) {
            // max_steps reached with photons still alive: they go back to the caller's arrays
            unsigned blocks = (unsigned)std::min<long long>((n_upper + 255) / 256, 4096);
            hipLaunchKernelGGL(k_store_working, dim3(std::max(blocks, 1u)), dim3(256), 0, ctx->stream, geom->view, pv, in_q, work_in);
        }
        HIP_TRY(hipMemcpyAsync(cs.h_step, cs.d_step, sizeof(StepState), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        acc.launches += ((const StepState *)cs.h_step)->launches;
        return opt.time_kernels ? read_step_times(step, tail_step) : CHROMA_OK;
    }

    // The step loop of a call that records tracks: the reference's tracking loop (chroma/gpu/photon.py:218-238) -- one step per
    // launch, every one re-normalising, the survivor count read after each -- with the rows taken on the device between the
    // steps.  Row 0 before anything moves; then per step a slab the size of its input queue from the pool, the step, and
    // k_track_step behind its last launch; at the end the rows per photon summed into offsets.
    // the photons still alive (the input working set as it stands) back to the caller's arrays
    void store_working()
    {
        const unsigned blocks = (unsigned)std::min<long long>((n_upper + 255) / 256, 4096);
        hipLaunchKernelGGL(k_store_working, dim3(std::max(blocks, 1u)), dim3(256), 0, ctx->stream, geom->view, pv, in_q, work_in);
    }

    int run_tracked_steps(uint64_t max_rows)
    {
        chroma_tracks &tr = *tracks;
        const int max_steps = std::max(opt.max_steps, 0);
        const unsigned tblocks = (unsigned)std::min<uint64_t>((nphotons + TRACK_BLOCK - 1) / TRACK_BLOCK, 4096);
        hipLaunchKernelGGL(k_track_row0, dim3(tblocks), dim3(TRACK_BLOCK), 0, ctx->stream, pv, (uint64_t)nphotons, tr.rows0, tr.offsets,
                           (uint32_t)max_steps + 1u, max_steps >= 1 ? 2u : 1u);
        HIP_TRY(hipGetLastError());
        tr.nrows = nphotons;
        int step = 0;
        if (max_steps >= 1) {
            HIP_TRY(hipMemsetAsync(cs.d_step, 0, sizeof(StepState), ctx->stream));
            hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, in_q, 1u);
            hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, out_q, 1u);
            int rc = load_working(); if (rc) return rc;
            const int nev = opt.time_kernels ? EV_PER_STEP * max_steps : 0;
            while ((int)cs.step_events.size() < nev) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); cs.step_events.push_back(e); }
            rc = scope.read_survivors(in_q, &n_upper); if (rc) return rc;
            tr.nrows += nphotons - (uint64_t)n_upper;             // (the second row of the photons that were terminal already)
            uint32_t *cursor = tr.offsets + nphotons + 1;
            while (step < max_steps && n_upper > 0) {
                const uint32_t n_in = (uint32_t)n_upper;
                chroma_tracks::Slab slab = {nullptr, n_in};
                // (the one thing that can stop a call between two steps: no room for the next step's rows, on the device or
                //  under the caller's limit.  The live photons go back to the arrays first, so that the photons are what the
                //  steps taken so far left them, draw counters included, and the caller can go on from there)
                if (step == 0) {
                    slab.rows = tr.slabs[0].rows;                 // (reserved before the first launch, for up to every photon)
                    tr.slabs.clear();
                    rc = CHROMA_OK;
                } else if (tr.nrows + n_in > max_rows)
                    rc = set_error(CHROMA_ERR_INVALID, "tracks: step %d would bring the call to %llu rows, more than the %llu of CHROMA_TRACKS_MAX_ROWS; %d steps were taken",
                                   step, (unsigned long long)(tr.nrows + n_in), (unsigned long long)max_rows, step);
                else
                    rc = chroma_malloc(ctx, (size_t)n_in * 4 * sizeof(float4), (void **)&slab.rows);
                if (rc) {
                    store_working();
                    hipStreamSynchronize(ctx->stream);
                    return rc;
                }
                tr.slabs.push_back(slab);
                HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(uint32_t), ctx->stream));
                rc = launch_split_step(step == 0 ? opt.scatter_first : 0, events(step), step == 0 ? (uint32_t)nphotons : 0u, false);
                if (rc) return rc;
                const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)n_in + TRACK_BLOCK - 1) / TRACK_BLOCK, 4096);
                hipLaunchKernelGGL(k_track_step, dim3(blocks), dim3(TRACK_BLOCK), 0, ctx->stream, geom->view, pv, (const uint32_t *)in_q,
                                   (const uint32_t *)out_q, (const float4 *)work_out, slab.rows, n_in, cursor, tr.offsets, (uint32_t)step);
                HIP_TRY(hipGetLastError());
                tr.nrows += n_in;
                step++;
                std::swap(in_q, out_q);
                std::swap(work_in, work_out);
                rc = scope.read_survivors(in_q, &n_upper); if (rc) return rc;
            }
            if (n_upper > 0) store_working();
            HIP_TRY(hipMemcpyAsync(cs.h_step, cs.d_step, sizeof(StepState), hipMemcpyDeviceToHost, ctx->stream));
        }
        int rc = chroma_internal_exclusive_sum(ctx, tr.offsets, (uint32_t)nphotons + 1u); if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        // (the caller sizes the arrays of chroma_tracks_gather by the host's count: the device's has to be the same)
        uint32_t total = 0;
        HIP_TRY(hipMemcpy(&total, tr.offsets + nphotons, sizeof total, hipMemcpyDeviceToHost));
        if (total != tr.nrows)
            return set_error(CHROMA_ERR_INTERNAL, "tracks: %u rows recorded where the step counts give %llu", total, (unsigned long long)tr.nrows);
        if (max_steps >= 1) acc.launches += ((const StepState *)cs.h_step)->launches;
        return opt.time_kernels ? read_step_times(step, -1) : CHROMA_OK;
    }

    // CHROMA_TAIL=fused: the lane-per-photon kernel with the reference's own launch shapes
    int run_fused()
    {
        hipLaunchKernelGGL(k_init_queue, dim3((unsigned)((nphotons + 255) / 256)), dim3(256), 0, ctx->stream, in_q,
                           (uint64_t)nphotons, ncopies, (uint32_t)(nphotons / ncopies));
        hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, out_q, 1u);
        HIP_TRY(hipGetLastError());
        const int max_steps = opt.max_steps;
        int scatter_first = opt.scatter_first;
        long long n = (long long)nphotons;
        int step = 0;
        while (step < max_steps) {
            const bool few = n < (long long)PROP_BLOCK * 16 * 8;
            int nsteps = (few || opt.use_weights) ? (max_steps - step) : 1;
            if (opt.time_kernels) HIP_TRY(hipEventRecord(cs.ev_start, ctx->stream));
            int rc = launch_propagate(scope, plan.counting, geom, pv, rng, {0, (int)n, in_q + 1, out_q, nsteps, opt.use_weights, scatter_first});
            if (rc) return rc;
            acc.launches++;
            if (opt.time_kernels) {
                HIP_TRY(hipEventRecord(cs.ev_stop, ctx->stream));
                HIP_TRY(hipEventSynchronize(cs.ev_stop));
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, cs.ev_start, cs.ev_stop));
                acc.kernel_ms += ms;
            }
            step += nsteps;
            scatter_first = 0;
            if (step < max_steps) {
                std::swap(in_q, out_q);
                // survivors = tail - 1 (one 4-byte read per step, as photon.py:250)
                hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, ctx->stream, out_q, 1u);
                rc = scope.read_survivors(in_q, &n); if (rc) return rc;
                if (n == 0) break;
            }
        }
        return CHROMA_OK;
    }

    // The call's last pass and its report.  A finalizing call: one pass takes the records to the caller's arrays and writes the
    // abort word, the hit count, the compacted hits and the per-channel arrays (k_finalize_hits), unless it has run beside the
    // tail kernel already (`finalized`, launch_tail).  Otherwise the abort word alone (photon.py:254-255).
    int finish(chroma_hits_request *hr, chroma_propagate_stats *stats, int32_t *aborted)
    {
        int rc = CHROMA_OK;
        if (!finalize) {
            rc = scope.clear_words(W_ABORT); if (rc) return rc;
            const unsigned blocks = (unsigned)std::min<uint64_t>((nphotons + 255) / 256, 4096);
            hipLaunchKernelGGL(k_flags_or, dim3(blocks), dim3(256), 0, ctx->stream, pv.flags, (uint64_t)nphotons, CHROMA_NAN_ABORT,
                               cs.d_words + W_ABORT);
        } else if (!finalized) {
            rc = scope.clear_results(); if (rc) return rc;
            launch_finalize(ctx->stream, 0u);
        }
        HIP_TRY(hipGetLastError());
        rc = scope.read_results(); if (rc) return rc;
        if (hr) hr->nhits = scope.word(W_HIT_COUNT);          // (a call with a hits request finalizes)
        if (aborted) *aborted = (scope.word(W_ABORT) & CHROMA_NAN_ABORT) ? 1 : 0;
        chroma_propagate_stats tmp; memset(&tmp, 0, sizeof tmp);
        chroma_propagate_stats *s = stats ? stats : &tmp;
        rc = stats_read(scope, s); if (rc) return rc;
        if (stats) {
            stats->launches += acc.launches;
            stats->kernel_ms += acc.kernel_ms;
            stats->raycast_ms += acc.raycast_ms;
            stats->raycast_launches += acc.raycast_launches;
            stats->physics_ms += acc.physics_ms;
            stats->physics_launches += acc.physics_launches;
            stats->packet_ms += acc.packet_ms;
            stats->packet_launches += acc.packet_launches;
            stats->reordered += acc.reordered;
        }
        if (s->stack_overflows) return set_error(CHROMA_ERR_STACK, "traversal stack overflowed for %llu rays", (unsigned long long)s->stack_overflows);
        return CHROMA_OK;
    }
};
}

// chroma_init's share of this file: the grids of the ray-cast kernels from their residency, the walk and the launch policy
// from the CHROMA_* environment
int propagate_settings(const CallScope &scope)
{
    chroma_ctx *ctx = scope.ctx; CallState &cs = scope.state();
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    ctx->physics_blocks = prop.multiProcessorCount * 8;          // (for blocks of PHYS_BLOCK threads)
    const char *walk = getenv("CHROMA_WALK");
    if (walk) cs.walk = CHROMA_WALK_QUAD;                      // (what is no walk's name means the default)
    for (int w = 0; w < NWALKS; w++) {
        const Walk &row = WALKS[w];
        int per_cu = row.waves_per_cu;
        if (const char *e = getenv(row.waves_env)) per_cu = std::max(1, atoi(e));
        ctx->waves[(int)row.cast] = prop.multiProcessorCount * per_cu;
        if (walk && (!strcmp(walk, row.name) || (row.alias && !strcmp(walk, row.alias)))) cs.walk = w;
    }
#if CHROMA_EXPERIMENTAL
    if (const char *e = getenv("CHROMA_PACKET")) cs.packet_mode = !strcmp(e, "on") ? 1 : !strcmp(e, "auto") ? 2 : 0;
    if (const char *e = getenv("CHROMA_AUTOSORT")) cs.autosort_mode = !strcmp(e, "on") || !strcmp(e, "1") ? 1 : !strcmp(e, "off") || !strcmp(e, "0") ? 0 : 2;
#endif
    if (const char *e = getenv("CHROMA_RAY_CHUNK")) ctx->ray_chunk = std::max(64, atoi(e));
    if (const char *e = getenv("CHROMA_COOP_CHUNK")) ctx->coop_chunk = std::max(8, atoi(e));
    if (const char *e = getenv("CHROMA_CLAIM_STATIC")) { int big = 0, small = 0; if (sscanf(e, "%d:%d", &big, &small) < 2) small = big; ctx->claim_static = std::min(8, std::max(0, big)) | std::min(8, std::max(0, small)) << 4; }
    if (const char *e = getenv("CHROMA_TAIL"))        // coop (default) | split | fused (the lane-per-photon k_propagate)
        cs.tail_mode = !strcmp(e, "fused") ? CHROMA_TAIL_FUSED : !strcmp(e, "split") ? CHROMA_TAIL_SPLIT : CHROMA_TAIL_COOP;
    return CHROMA_OK;
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
extern "C" {

// ---- kernel-level entry points ------------------------------------------------------------------------
int chroma_propagate_step(chroma_ctx *ctx, chroma_geometry *geom, int32_t first_photon, int32_t nthreads,
                          const uint32_t *d_input_queue, uint32_t *d_output_queue, chroma_rng rng,
                          const chroma_photon_arrays *photons, int32_t max_steps, int32_t use_weights,
                          int32_t scatter_first)
{
    if (!ctx || !geom) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(photons, true);
    if (rc) return rc;
    if (first_photon < 0 || nthreads < 0) return set_error(CHROMA_ERR_INVALID, "negative photon range");
    if (nthreads == 0) return CHROMA_OK;
    if ((rc = check_stack(geom))) return rc;
    const CallScope scope(ctx);
    return launch_propagate(scope, scope.state().counting != 0, geom, to_view(photons), rng,
                            {first_photon, nthreads, d_input_queue, d_output_queue, max_steps, use_weights, scatter_first});
}

static int ensure_queues(const CallScope &scope, size_t n)
{
    chroma_ctx *ctx = scope.ctx; CallState &cs = scope.state();
    if (cs.queue_capacity >= n + 1) return CHROMA_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const auto buffers = queue_buffers(cs);
    for (const QueueBuffer &b : buffers) { if (*b.ptr) hipFree(*b.ptr); *b.ptr = nullptr; }
    cs.queue_capacity = 0;
    for (const QueueBuffer &b : buffers) HIP_TRY(ctx_malloc(ctx, b.ptr, (n + 1) * b.bytes));
    cs.queue_capacity = n + 1;
    return CHROMA_OK;
}

int chroma_distance_to_mesh(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const float *d_origin,
                            const float *d_direction, float *d_distance, int32_t *d_triangle)
{
    return chroma_intersect_mesh(ctx, geom, nthreads, d_origin, d_direction, nullptr, d_distance, d_triangle);
}

int chroma_intersect_mesh(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const float *d_origin,
                          const float *d_direction, const int32_t *d_last_hit, float *d_distance, int32_t *d_triangle)
{
    if (!ctx || !geom || !d_origin || !d_direction || !d_distance) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nthreads <= 0) return CHROMA_OK;
    const CallScope scope(ctx);          // (the fast path uses the context's queues and ray records, as a propagate call does)
    return intersect_mesh_in_scope(scope, geom, nthreads, d_origin, d_direction, d_last_hit, d_distance, d_triangle);
}

}  // extern "C"

// chroma_intersect_mesh behind its checks and its lock (chroma_internal.h: the particle loop of steps_calls.hip calls it too)
int intersect_mesh_in_scope(const CallScope &scope, chroma_geometry *geom, int32_t nthreads, const float *d_origin, const float *d_direction,
                            const int32_t *d_last_hit, float *d_distance, int32_t *d_triangle)
{
    chroma_ctx *ctx = scope.ctx;
    CallState &cs = scope.state();
    CallPlan plan;
    int rc = check_stack(geom); if (rc) return rc;
    rc = make_plan(cs, geom, -1, -1, -1, &plan); if (rc) return rc;
    if (!plan.isect_quad) {
        const dim3 grid((unsigned)((nthreads + PROP_BLOCK - 1) / PROP_BLOCK)), block(PROP_BLOCK);
        with_bool(plan.counting, [&](auto C) {
            hipLaunchKernelGGL((k_distance_to_mesh<STACK_LDS, C>), grid, block, 0, ctx->stream, geom->view, nthreads, d_origin, d_direction,
                               d_last_hit, d_distance, d_triangle, cs.d_counters);
        });
        HIP_TRY(hipGetLastError());
        return CHROMA_OK;
    }
    // the quad walk of the default propagate step over the caller's rays: k_raycast_quad, then the strict loop for the rays it hands over
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_queues(scope, (size_t)nthreads); if (rc) return rc;
    rc = ensure_spill(scope, SPILL_COOP); if (rc) return rc;
    StepState *st = cs.d_step;
    const unsigned blocks = (unsigned)((nthreads + 255) / 256);
    hipLaunchKernelGGL(k_step_set, dim3(1), dim3(1), 0, ctx->stream, st, (uint32_t)nthreads);
    hipLaunchKernelGGL(k_rays_from_arrays, dim3(blocks), dim3(256), 0, ctx->stream, geom->view, (int)nthreads, d_origin, d_direction,
                       d_last_hit, cs.rays, cs.hit_triangle, cs.hit_distance, cs.retry_list, st);
    const unsigned waves = cast_waves(ctx, Cast::QUAD, nthreads);
    with_bool(plan.counting, [&](auto C) {
        hipLaunchKernelGGL((k_raycast_quad<C>), dim3(waves), dim3(PROP_BLOCK), 0, ctx->stream, geom->view, cs.rays, 0, st,
                           cs.hit_triangle, cs.hit_distance, cs.retry_list, cs.coop_spill, cs.d_counters, ctx->coop_chunk, 0, nullptr, ctx->claim_static);
    });
    hipLaunchKernelGGL(k_distance_finish, dim3(blocks), dim3(256), 0, ctx->stream, geom->view, (int)nthreads, cs.rays, cs.hit_triangle,
                       cs.hit_distance, d_distance, d_triangle, cs.retry_list, st);
    with_bool(plan.counting, [&](auto C) {
        hipLaunchKernelGGL((k_distance_retry<C>), dim3(256), dim3(PROP_BLOCK), 0, ctx->stream, geom->view, cs.rays, st,
                           cs.retry_list, d_distance, d_triangle, cs.d_counters);
    });
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

extern "C" {

// The ray cast of chroma_intersect_mesh over rays that share one direction, then the material from each ray's triangle.  The
// cast's own per-slot results are its scratch: the distances go back where they came from, and the triangle ids take the
// place of the hit records when the caller does not ask for them.
int chroma_locate_materials(chroma_ctx *ctx, chroma_geometry *geom, int32_t n, const float *d_points, const float direction[3],
                            int32_t outside, int32_t *d_material, int32_t *d_triangle)
{
    if (!ctx || !geom || !d_points || !d_material) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (n < 0) return set_error(CHROMA_ERR_INVALID, "negative number of points");
    const float dx = direction ? direction[0] : 0.0f, dy = direction ? direction[1] : 0.0f, dz = direction ? direction[2] : 1.0f;
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    if (!(len > 0.0f) || !isfinite(len)) return set_error(CHROMA_ERR_INVALID, "probe direction of no length");
    if (n == 0) return CHROMA_OK;
    int rc = check_stack(geom); if (rc) return rc;
    const CallScope scope(ctx);
    CallState &cs = scope.state();
    CallPlan plan;
    rc = make_plan(cs, geom, -1, -1, -1, &plan); if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_queues(scope, (size_t)n); if (rc) return rc;
    int32_t *triangle = d_triangle ? d_triangle : cs.hit_triangle;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (!plan.isect_quad) {
        with_bool(plan.counting, [&](auto C) {
            hipLaunchKernelGGL((k_locate_walk<STACK_LDS, C>), dim3((unsigned)((n + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, ctx->stream,
                               geom->view, (int)n, d_points, dx, dy, dz, triangle, cs.d_counters);
        });
    } else {
        rc = ensure_spill(scope, SPILL_COOP); if (rc) return rc;
        StepState *st = cs.d_step;
        hipLaunchKernelGGL(k_step_set, dim3(1), dim3(1), 0, ctx->stream, st, (uint32_t)n);
        hipLaunchKernelGGL(k_locate_rays, dim3(blocks), dim3(256), 0, ctx->stream, geom->view, (int)n, d_points, dx, dy, dz, cs.rays,
                           cs.hit_triangle, cs.hit_distance, cs.retry_list, st);
        const unsigned waves = cast_waves(ctx, Cast::QUAD, n);
        with_bool(plan.counting, [&](auto C) {
            hipLaunchKernelGGL((k_raycast_quad<C>), dim3(waves), dim3(PROP_BLOCK), 0, ctx->stream, geom->view, cs.rays, 0, st,
                               cs.hit_triangle, cs.hit_distance, cs.retry_list, cs.coop_spill, cs.d_counters, ctx->coop_chunk, 0, nullptr, ctx->claim_static);
        });
        hipLaunchKernelGGL(k_distance_finish, dim3(blocks), dim3(256), 0, ctx->stream, geom->view, (int)n, cs.rays, cs.hit_triangle,
                           cs.hit_distance, cs.hit_distance, triangle, cs.retry_list, st);
        with_bool(plan.counting, [&](auto C) {
            hipLaunchKernelGGL((k_distance_retry<C>), dim3(256), dim3(PROP_BLOCK), 0, ctx->stream, geom->view, cs.rays, st,
                               cs.retry_list, cs.hit_distance, triangle, cs.d_counters);
        });
    }
    hipLaunchKernelGGL(k_locate_material, dim3(blocks), dim3(256), 0, ctx->stream, geom->view, (int)n, triangle, dx, dy, dz, outside, d_material);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

// ---- fused host loops -----------------------------------------------------------------------------------
int chroma_propagate_stats_read(chroma_ctx *ctx, chroma_propagate_stats *stats)
{
    if (!ctx || !stats) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    return stats_read(scope, stats);
}

int chroma_set_counting(chroma_ctx *ctx, int32_t enabled)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    CallScope(ctx).state().counting = enabled ? 1 : 0;
    return CHROMA_OK;
}

int chroma_set_walk(chroma_ctx *ctx, int32_t mode)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (mode < 0 || mode >= NWALKS) return set_error(CHROMA_ERR_INVALID, "unknown walk mode %d", mode);
    CallScope(ctx).state().walk = mode;
    return CHROMA_OK;
}

int chroma_set_packet(chroma_ctx *ctx, int32_t mode)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (mode < 0 || mode > 2) return set_error(CHROMA_ERR_INVALID, "unknown packet mode %d", mode);
#if !CHROMA_EXPERIMENTAL
    if (mode != 0) return set_error(CHROMA_ERR_INVALID, "the packet ray cast is an experiment that is not part of this build (csrc/experimental/: build_variants/libchroma_hip_experimental.so)");
#endif
    CallScope(ctx).state().packet_mode = mode;
    return CHROMA_OK;
}

int chroma_set_autosort(chroma_ctx *ctx, int32_t mode)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (mode < 0 || mode > 2) return set_error(CHROMA_ERR_INVALID, "unknown autosort mode %d", mode);
#if !CHROMA_EXPERIMENTAL
    if (mode != 0) return set_error(CHROMA_ERR_INVALID, "the engine-side direction sort is an experiment that is not part of this build (csrc/experimental/: build_variants/libchroma_hip_experimental.so)");
#endif
    CallScope(ctx).state().autosort_mode = mode;
    return CHROMA_OK;
}

int chroma_set_tail(chroma_ctx *ctx, int32_t mode)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (mode != CHROMA_TAIL_COOP && mode != CHROMA_TAIL_SPLIT && mode != CHROMA_TAIL_FUSED)
        return set_error(CHROMA_ERR_INVALID, "unknown tail mode %d", mode);
    CallScope(ctx).state().tail_mode = mode;
    return CHROMA_OK;
}

#if CHROMA_EXPERIMENTAL
#include "experimental/autosort.h"
#else
// (product build: a call takes its photons as they come -- the engine-side direction sort lives in experimental/autosort.h)
static int propagate_order(PropagateCall &, uint32_t **d_order) { *d_order = nullptr; return CHROMA_OK; }
#endif

// the photons' final records (chroma_propagate_hits): 64 bytes per photon of the largest batch seen, zeroed once -- a record
// belongs to a call when it carries that call's epoch, and epochs start at 1
static int ensure_final_records(const CallScope &scope, size_t n)
{
    chroma_ctx *ctx = scope.ctx; CallState &cs = scope.state();
    if (cs.final_capacity >= n) return CHROMA_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (cs.final_rec) hipFree(cs.final_rec);
    cs.final_rec = nullptr; cs.final_capacity = 0;
    HIP_TRY(ctx_malloc(ctx, (void **)&cs.final_rec, n * 4 * sizeof(float4)));
    HIP_TRY(hipMemsetAsync(cs.final_rec, 0, n * 4 * sizeof(float4), ctx->stream));
    cs.final_capacity = n;
    cs.final_epoch = 0;
    return CHROMA_OK;
}

static int propagate_impl(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons, uint64_t nphotons,
                          uint32_t ncopies, chroma_rng rng, const chroma_propagate_options &opt,
                          chroma_propagate_stats *stats, int32_t *aborted, chroma_hits_request *hr)
{
    if (!ctx || !geom) return set_error(CHROMA_ERR_INVALID, "bad argument");
    int rc = check_photons(photons, true); if (rc) return rc;
    // one call at a time per context: the queues, working sets, step block and final records are the context's own
    const CallScope scope(ctx);
    CallState &cs = scope.state();
    // what this call does: the context's settings as they are NOW, overridden by the call's own options
    CallPlan plan;
    rc = make_plan(cs, geom, opt.walk, opt.tail, opt.counting, &plan); if (rc) return rc;
    if (hr) {
        hr->nhits = 0;
        if (!geom->view.nsolids) return set_error(CHROMA_ERR_INVALID, "geometry has no detector channel map");
        if (hr->dst) { rc = check_photons(hr->dst, false); if (rc) return rc; }
        if ((hr->dst != nullptr) != (hr->d_channels != nullptr)) return set_error(CHROMA_ERR_INVALID, "flat hits need both dst and d_channels");
    }
    if (nphotons >= 0x7fffffffull) return set_error(CHROMA_ERR_INVALID, "at most 2^31-2 photons per call");
    if (ncopies == 0 || nphotons % ncopies) return set_error(CHROMA_ERR_INVALID, "nphotons must be a multiple of ncopies");
    if (aborted) *aborted = 0;
    // (no step to take: a hits request is honoured all the same -- the photons detected before the call are its hits, read from
    //  the arrays as they are, so that the call means propagate + get_flat_hits for every max_steps)
    const bool stepping = opt.max_steps > 0;
    if (nphotons == 0 || (!stepping && !hr)) return CHROMA_OK;
    if (stepping && (rc = check_stack(geom))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (stepping) {
        rc = ensure_queues(scope, nphotons); if (rc) return rc;
        rc = ensure_spill(scope, plan.spill); if (rc) return rc;
    }
    // (final records: with a hit request, or for every call under CHROMA_FINAL_RECORDS=1 -- an A/B switch)
    static const bool records_always = getenv("CHROMA_FINAL_RECORDS") && atoi(getenv("CHROMA_FINAL_RECORDS")) != 0;
    const bool use_records = stepping && (hr != nullptr || records_always) && plan.tail_mode != CHROMA_TAIL_FUSED;
    if (use_records) {
        rc = ensure_final_records(scope, nphotons); if (rc) return rc;
        cs.final_epoch++;
        if (cs.final_epoch == 0u || cs.final_epoch >= 0x7FFFFFFFu) {            // (wrapped -- the top bit marks the tail kernel's photons --: no stale record may look current)
            HIP_TRY(hipMemsetAsync(cs.final_rec, 0, cs.final_capacity * 4 * sizeof(float4), ctx->stream));
            cs.final_epoch = 1u;
        }
    }
    PropagateCall call = {scope, cs, ctx, geom, plan, to_view(photons), rng, opt, nphotons, ncopies, cs.queue_a, cs.queue_b, cs.work_a, cs.work_b,
                          cs.rays, cs.rays_b, use_records ? cs.final_rec : nullptr, cs.final_epoch};
    if (hr) {
        call.ho.want = 1;
        call.ho.detection_state = hr->detection_state;
        if (hr->dst) { call.ho.dst = to_view(hr->dst); call.ho.channels = hr->d_channels; call.ho.capacity = hr->capacity; }
        call.ho.hit_count = hr->d_hit_count; call.ho.earliest = hr->d_hit_count ? hr->d_earliest_time_bits : nullptr;
    }
    call.finalize = use_records || hr;
    call.n_upper = (long long)nphotons;
    if (stepping) {
        rc = plan.tail_mode == CHROMA_TAIL_FUSED ? call.run_fused() : call.run_device_steps();
        if (rc) return rc;
    }
    return call.finish(hr, stats, aborted);
}

static chroma_propagate_options default_options(int32_t max_steps, int32_t use_weights, int32_t scatter_first, int32_t time_kernels)
{
    chroma_propagate_options o; memset(&o, 0, sizeof o);
    o.max_steps = max_steps; o.use_weights = use_weights; o.scatter_first = scatter_first; o.time_kernels = time_kernels;
    o.walk = o.tail = o.counting = -1;
    return o;
}

int chroma_propagate(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons, uint64_t nphotons,
                     uint32_t ncopies, chroma_rng rng, int32_t max_steps, int32_t use_weights, int32_t scatter_first,
                     int32_t time_kernels, chroma_propagate_stats *stats, int32_t *aborted)
{
    return propagate_impl(ctx, geom, photons, nphotons, ncopies, rng, default_options(max_steps, use_weights, scatter_first, time_kernels), stats, aborted, nullptr);
}

int chroma_propagate_hits(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons, uint64_t nphotons,
                          uint32_t ncopies, chroma_rng rng, int32_t max_steps, int32_t use_weights, int32_t scatter_first,
                          int32_t time_kernels, chroma_propagate_stats *stats, int32_t *aborted, chroma_hits_request *hits)
{
    if (!hits) return set_error(CHROMA_ERR_INVALID, "bad argument");
    return propagate_impl(ctx, geom, photons, nphotons, ncopies, rng, default_options(max_steps, use_weights, scatter_first, time_kernels), stats, aborted, hits);
}

int chroma_propagate_opt(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons, uint64_t nphotons,
                         uint32_t ncopies, chroma_rng rng, const chroma_propagate_options *options,
                         chroma_propagate_stats *stats, int32_t *aborted, chroma_hits_request *hits)
{
    if (!options) return set_error(CHROMA_ERR_INVALID, "bad argument");
    return propagate_impl(ctx, geom, photons, nphotons, ncopies, rng, *options, stats, aborted, hits);
}

// ---- photon tracks ------------------------------------------------------------------------------------------------------
// A propagate call that also records every photon's track (kernels_tracks.h, PropagateCall::run_tracked_steps): the split step
// loop with one re-normalising launch per step, no hits request and no final records.  Everything that can be refused is
// refused before the first launch; what the call allocates as it goes (a slab per step) comes from the context's pool.
int chroma_propagate_tracks(chroma_ctx *ctx, chroma_geometry *geom, const chroma_photon_arrays *photons, uint64_t nphotons,
                            uint32_t ncopies, chroma_rng rng, const chroma_propagate_options *options,
                            chroma_propagate_stats *stats, int32_t *aborted, chroma_tracks **tracks, uint64_t *nrows)
{
    if (!ctx || !geom || !options || !tracks || !nrows) return set_error(CHROMA_ERR_INVALID, "bad argument");
    *tracks = nullptr; *nrows = 0;
    int rc = check_photons(photons, true); if (rc) return rc;
    const CallScope scope(ctx);
    CallState &cs = scope.state();
    const chroma_propagate_options &opt = *options;
    if ((opt.tail >= 0 ? opt.tail : cs.tail_mode) == CHROMA_TAIL_FUSED)
        return set_error(CHROMA_ERR_INVALID, "tracks are recorded between the steps of the split step loop: not with the fused tail");
    CallPlan plan;
    rc = make_plan(cs, geom, opt.walk, CHROMA_TAIL_SPLIT, opt.counting, &plan); if (rc) return rc;
    plan.packet = plan.autosort = 0;
    if (nphotons >= 0x7fffffffull) return set_error(CHROMA_ERR_INVALID, "at most 2^31-2 photons per call");
    if (ncopies == 0 || nphotons % ncopies) return set_error(CHROMA_ERR_INVALID, "nphotons must be a multiple of ncopies");
    const uint64_t max_steps = opt.max_steps > 0 ? (uint64_t)opt.max_steps : 0u;
    if (nphotons * (max_steps + 1) > 0xFFFFFFFFull)
        return set_error(CHROMA_ERR_INVALID, "%llu photons of up to %llu rows each: more than the 2^32-1 rows a call holds, pass fewer photons or steps",
                         (unsigned long long)nphotons, (unsigned long long)(max_steps + 1));
    // (CHROMA_TRACKS_MAX_ROWS: the rows a call may record -- 64 bytes of device memory each while it runs -- read at every call)
    uint64_t max_rows = 0xFFFFFFFFull;
    if (const char *e = getenv("CHROMA_TRACKS_MAX_ROWS")) max_rows = std::min<uint64_t>(max_rows, strtoull(e, nullptr, 10));
    const uint64_t least_rows = nphotons * (max_steps > 0 ? 2u : 1u);          // (row 0, and one more for a photon alive or not)
    if (least_rows > max_rows)
        return set_error(CHROMA_ERR_INVALID, "%llu photons have at least %llu rows, more than the %llu of CHROMA_TRACKS_MAX_ROWS",
                         (unsigned long long)nphotons, (unsigned long long)least_rows, (unsigned long long)max_rows);
    if (aborted) *aborted = 0;
    if (max_steps > 0 && nphotons > 0 && (rc = check_stack(geom))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    chroma_tracks *tr = new chroma_tracks;
    tr->nphotons = nphotons;
    if (nphotons == 0) { *tracks = tr; return CHROMA_OK; }
    rc = chroma_malloc(ctx, (size_t)nphotons * 4 * sizeof(float4), (void **)&tr->rows0);
    if (rc == CHROMA_OK) rc = chroma_malloc(ctx, ((size_t)nphotons + 2) * sizeof(uint32_t), (void **)&tr->offsets);
    if (rc == CHROMA_OK && max_steps > 0) {
        // (the first step's slab too, for as many rows as there are photons: what fails for lack of memory before a step has
        //  been taken fails here, before the first launch)
        chroma_tracks::Slab first = {nullptr, 0u};
        rc = chroma_malloc(ctx, (size_t)nphotons * 4 * sizeof(float4), (void **)&first.rows);
        if (rc == CHROMA_OK) tr->slabs.push_back(first);
    }
    if (rc == CHROMA_OK && max_steps > 0) {
        rc = ensure_queues(scope, nphotons);
        if (rc == CHROMA_OK) rc = ensure_spill(scope, plan.spill);
    }
    if (rc == CHROMA_OK) {
        PropagateCall call = {scope, cs, ctx, geom, plan, to_view(photons), rng, opt, nphotons, ncopies, cs.queue_a, cs.queue_b, cs.work_a, cs.work_b,
                              cs.rays, cs.rays_b, nullptr, 0u};
        call.n_upper = (long long)nphotons;
        call.tracks = tr;
        rc = call.run_tracked_steps(max_rows);
        if (rc == CHROMA_OK) rc = call.finish(nullptr, stats, aborted);
    }
    if (rc != CHROMA_OK) { tracks_release(ctx, tr); return rc; }
    *tracks = tr; *nrows = tr->nrows;
    return CHROMA_OK;
}

int chroma_tracks_gather(chroma_ctx *ctx, chroma_tracks *tracks, const chroma_photon_arrays *dst, uint64_t *d_offsets)
{
    if (!ctx || !tracks || !d_offsets) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (tracks->nphotons == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), ctx->stream));
        return CHROMA_OK;
    }
    int rc = check_photons(dst, false); if (rc) return rc;
    const PhotonView out = to_view(dst);
    const uint64_t n = tracks->nphotons;
    hipLaunchKernelGGL(k_track_scatter_row0, dim3((unsigned)std::min<uint64_t>((n + TRACK_BLOCK - 1) / TRACK_BLOCK, 4096)), dim3(TRACK_BLOCK), 0,
                       ctx->stream, (const float4 *)tracks->rows0, n, (const uint32_t *)tracks->offsets, out, d_offsets);
    for (size_t k = 0; k < tracks->slabs.size(); k++) {
        const chroma_tracks::Slab &s = tracks->slabs[k];
        if (!s.count) continue;
        hipLaunchKernelGGL(k_track_scatter, dim3((unsigned)std::min<uint64_t>(((uint64_t)s.count + TRACK_BLOCK - 1) / TRACK_BLOCK, 4096)),
                           dim3(TRACK_BLOCK), 0, ctx->stream, (const float4 *)s.rows, s.count, (uint32_t)k, n, (const uint32_t *)tracks->offsets, out);
    }
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_tracks_destroy(chroma_ctx *ctx, chroma_tracks *tracks)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    const CallScope scope(ctx);            // (not while another thread's chroma_tracks_gather reads the handle)
    tracks_release(ctx, tracks);
    return CHROMA_OK;
}

#if CHROMA_HYBRID_RENDER
// ---- the hybrid render (chroma/cuda/hybrid_render.cu as chroma/camera.py:188-249 drives it; kernels_hybrid_render.h) ----
// Everything is checked before the first launch.  The two sample passes hold a CallScope: they run the step
// functions and count stack overflows into the context's counters, as the propagate calls do.
static int hybrid_check(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, const uint32_t *d_rng_counters, uint32_t ncounters,
                        uint32_t nlookup, int32_t max_steps, const void *s_tri, const void *s_side, const void *s_history)
{
    if (!ctx || !geom || !d_rng_counters) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nthreads < 0) return set_error(CHROMA_ERR_INVALID, "negative thread count");
    if ((uint32_t)nthreads > ncounters) return set_error(CHROMA_ERR_INVALID, "%d threads but %u rng counters", nthreads, ncounters);
    if ((size_t)nlookup != geom->ntriangles)
        return set_error(CHROMA_ERR_INVALID, "lookup tables of %u entries for %zu triangles", nlookup, geom->ntriangles);
    if (geom->ntriangles >= 0x7fffffffu) return set_error(CHROMA_ERR_INVALID, "at most 2^31-2 triangles");
    if (max_steps < 0) return set_error(CHROMA_ERR_INVALID, "max_steps %d is negative", max_steps);
    if ((s_tri != nullptr) != (s_side != nullptr) || (s_tri != nullptr) != (s_history != nullptr))
        return set_error(CHROMA_ERR_INVALID, "sample outputs: give all or none");
    return check_stack(geom);
}

int chroma_hybrid_lookup(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, int32_t total_threads, int32_t offset,
                         const float position[3], chroma_rng rng, uint32_t *d_rng_counters, uint32_t ncounters, float wavelength,
                         const float xyz[3], float *d_lookup1, float *d_lookup2, uint32_t nlookup, int32_t max_steps,
                         int32_t *d_sample_triangle, uint32_t *d_sample_side, uint32_t *d_sample_history, float *d_sample_cos)
{
    int rc = hybrid_check(ctx, geom, nthreads, d_rng_counters, ncounters, nlookup, max_steps, d_sample_triangle, d_sample_side,
                          d_sample_history);
    if (rc) return rc;
    if (!position || !xyz || !d_lookup1 || !d_lookup2) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if ((d_sample_triangle != nullptr) != (d_sample_cos != nullptr)) return set_error(CHROMA_ERR_INVALID, "sample outputs: give all or none");
    if (total_threads < 0 || offset < 0) return set_error(CHROMA_ERR_INVALID, "negative triangle range");
    const int64_t end = std::min<int64_t>(std::min<int64_t>((int64_t)offset + nthreads, total_threads), (int64_t)geom->ntriangles);
    const int64_t n = end - offset;                    // threads whose triangle exists; the rest return at once (draw nothing)
    if (n <= 0) return CHROMA_OK;
    const uint32_t key_none = 2u * (uint32_t)geom->ntriangles;            // past every (2 * triangle + side)
    const int end_bit = 32 - __builtin_clz(key_none);
    const CallScope scope(ctx);
    void *buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};          // keys, ids, sorted keys, order, values
    const size_t bytes[5] = {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 12};
    for (int i = 0; i < 5 && rc == CHROMA_OK; i++) rc = chroma_malloc(ctx, bytes[i], &buf[i]);
    uint32_t *keys = (uint32_t *)buf[0], *ids = (uint32_t *)buf[1], *sorted = (uint32_t *)buf[2], *order = (uint32_t *)buf[3];
    float *values = (float *)buf[4];
    if (rc == CHROMA_OK) {
        hipLaunchKernelGGL((k_hybrid_lookup<STACK_LDS>), dim3((unsigned)((n + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0,
                           ctx->stream, geom->view, (int)n, (int)offset, position[0], position[1], position[2], rng.seed,
                           rng.photon_id_base, d_rng_counters, wavelength, xyz[0], xyz[1], xyz[2], max_steps, key_none, keys, ids,
                           values, d_sample_triangle, d_sample_side, d_sample_history, d_sample_cos, scope.state().d_counters);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = set_error((int)e, "k_hybrid_lookup: %s", hipGetErrorString(e));
    }
    if (rc == CHROMA_OK) rc = chroma_internal_sort_pairs(ctx, keys, sorted, ids, order, (uint32_t)n, end_bit);
    if (rc == CHROMA_OK) {
        hipLaunchKernelGGL(k_hybrid_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, sorted, order,
                           values, key_none, d_lookup1, d_lookup2);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = set_error((int)e, "k_hybrid_reduce: %s", hipGetErrorString(e));
    }
    for (void *p : buf) if (p) chroma_free(ctx, p);       // (parked behind the stream's work)
    return rc;
}

int chroma_hybrid_image(chroma_ctx *ctx, chroma_geometry *geom, int32_t nthreads, chroma_rng rng, uint32_t *d_rng_counters,
                        uint32_t ncounters, const float *d_positions, const float *d_directions, float wavelength, const float xyz[3],
                        const float *d_lookup1, const float *d_lookup2, uint32_t nlookup, float *d_image, uint32_t nimage,
                        int32_t nlookup_calls, int32_t max_steps, int32_t *d_sample_triangle, uint32_t *d_sample_side,
                        uint32_t *d_sample_history)
{
    int rc = hybrid_check(ctx, geom, nthreads, d_rng_counters, ncounters, nlookup, max_steps, d_sample_triangle, d_sample_side,
                          d_sample_history);
    if (rc) return rc;
    if (!d_positions || !d_directions || !xyz || !d_lookup1 || !d_lookup2 || !d_image) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if ((uint32_t)nthreads > nimage) return set_error(CHROMA_ERR_INVALID, "%d rays but an image of %u pixels", nthreads, nimage);
    if (nlookup_calls < 1) return set_error(CHROMA_ERR_INVALID, "nlookup_calls must be at least 1");
    if (nthreads == 0) return CHROMA_OK;
    const CallScope scope(ctx);
    hipLaunchKernelGGL((k_hybrid_image<STACK_LDS>), dim3((unsigned)((nthreads + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0,
                       ctx->stream, geom->view, (int)nthreads, rng.seed, rng.photon_id_base, d_rng_counters, d_positions, d_directions,
                       wavelength, xyz[0], xyz[1], xyz[2], d_lookup1, d_lookup2, d_image, (int)nlookup_calls, max_steps,
                       d_sample_triangle, d_sample_side, d_sample_history, scope.state().d_counters);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

int chroma_hybrid_pixels(chroma_ctx *ctx, int32_t nthreads, const float *d_image, uint32_t *d_pixels, int32_t nimages)
{
    if (!ctx || !d_image || !d_pixels) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (nthreads < 0) return set_error(CHROMA_ERR_INVALID, "negative pixel count");
    if (nimages < 1) return set_error(CHROMA_ERR_INVALID, "nimages must be at least 1");
    if (nthreads == 0) return CHROMA_OK;
    hipLaunchKernelGGL(k_hybrid_pixels, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, ctx->stream, (int)nthreads, d_image,
                       d_pixels, (int)nimages);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}
#endif  // CHROMA_HYBRID_RENDER

}  // extern "C"
