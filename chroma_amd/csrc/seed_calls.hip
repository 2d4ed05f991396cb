// seed_calls.hip -- the vertex seed's entry point (kernels_seed.h): chroma_vertex_seed is a pipeline on the context's pooled scratch
// block -- the two host arrays copied up, the validation pass over the two device arrays of coordinates and its verdict read
// back, the level-0 scores of every (fit, candidate), then the refinement of every fit through all its levels in one launch (batches
// beyond a launch's 2^23 - 1 blocks take several of either).
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "chroma_internal.h"

#include "kernels_seed.h"

static_assert(sizeof(chroma_vertex_seeder) == 88, "chroma_vertex_seeder is 88 bytes (include/chroma_hip.h)");
static_assert(sizeof(SeedLds) + SEED_WAVES * 8 + 8 <= SEED_LDS_BYTES && SEED_LDS_BYTES <= 65536, "the seed kernels' LDS: two blocks to a CU at the least");
static_assert(SEED_CHUNK == SEED_BLOCK, "a thread stages one hit of a chunk");

// The call's share of the context's scratch block, in this order: the validation's verdict, the offsets, tau0, the level-0 maxima
struct SeedScratch {
    uint32_t *bad, *offsets; int32_t *tau0; unsigned long long *best0;

    void lay(Carver &c, size_t nfits)
    {
        bad = c.take<uint32_t>(1);
        offsets = c.take<uint32_t>(nfits + 1);
        tau0 = c.take<int32_t>(nfits);
        best0 = c.take<unsigned long long>(nfits);
    }
};

// The blocks of one launch: fewer than 2^32 threads (HIP does not support gridDim.x * blockDim.x >= 2^32), so 2^23 - 1 blocks of
// 512.  CHROMA_SEED_LAUNCH_BLOCKS in the environment lowers it (1 .. that): how tests/test_gpu_seed.py makes a small batch take
// several launches of both kernels; the results do not depend on it.
static uint32_t seed_launch_limit()
{
    const uint32_t most = seed::launch_blocks(SEED_BLOCK);
    if (const char *e = getenv("CHROMA_SEED_LAUNCH_BLOCKS")) {
        const long long v = atoll(e);
        if (v >= 1 && v < (long long)most) return (uint32_t)v;
    }
    return most;
}
static_assert((uint64_t)seed::launch_blocks(SEED_BLOCK) * SEED_BLOCK < (1ull << 32) && seed::launch_blocks(SEED_BLOCK) >= (seed::MAX_CAND + SEED_WAVES - 1) / SEED_WAVES,
              "a launch stays under 2^32 threads and holds one fit's candidates");

extern "C" {

int chroma_vertex_seed(chroma_ctx *ctx, const chroma_vertex_seeder *seeder, uint32_t nchannels, const int32_t *d_channel_pos, uint32_t ncand,
                       const int32_t *d_cand, uint32_t nfits, const uint32_t *offsets, const int32_t *tau0, const int32_t *d_hit_channel,
                       const int32_t *d_hit_time, const uint32_t *d_hit_weight, int32_t *d_best_pos, uint32_t *d_best_score, uint32_t *d_best_bin,
                       uint32_t *d_best_cand, uint32_t *d_outside, uint32_t *d_level_score, uint32_t *d_scores)
{
    if (!ctx || !seeder ||
        (nfits && (!d_cand || !offsets || !tau0 || !d_best_pos || !d_best_score || !d_best_bin || !d_best_cand || !d_outside || !d_level_score)) ||
        (nfits && nchannels && !d_channel_pos))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = seed::check(seeder, nchannels, ncand, nfits, offsets, d_scores != nullptr)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (nfits == 0) return CHROMA_OK;
    if (offsets[nfits] && (!d_hit_channel || !d_hit_time || !d_hit_weight)) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    hipStream_t stream = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    SeedScratch sc;
    int rc = carve_call_scratch(scope, [&](Carver &c) { sc.lay(c, nfits); }); if (rc) return rc;
    // The two host arrays up, and the validation pass of the two device arrays with its verdict before the first fit is launched.
    // Whatever fails in between, the stream is drained before the call returns: the caller's host arrays are his again.
    uint32_t bad = 0u;
    const auto validate = [&]() -> int {
        HIP_TRY(hipMemsetAsync(sc.bad, 0, sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(sc.best0, 0, (size_t)nfits * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemcpyAsync(sc.offsets, offsets, ((size_t)nfits + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(sc.tau0, tau0, (size_t)nfits * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        if (nchannels) {          // (3 * nchannels < 2^32: seed::check)
            hipLaunchKernelGGL(k_seed_check, dim3((3u * nchannels + 255u) / 256u), dim3(256), 0, stream, d_channel_pos, 3u * nchannels, sc.bad);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_seed_check, dim3((3u * ncand + 255u) / 256u), dim3(256), 0, stream, d_cand, 3u * ncand, sc.bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, sc.bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
        return CHROMA_OK;
    };
    rc = validate();
    const hipError_t drained = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIP_TRY(drained);
    if (bad) return set_error(CHROMA_ERR_INVALID, "vertex seed: a coordinate of a channel or of a candidate is beyond 2^23");
    // level 0: eight candidates a block, whole fits a launch, as many as a launch's blocks hold
    const SeedHits hits{d_hit_channel, d_hit_time, d_hit_weight};
    const uint32_t limit = seed_launch_limit();
    const uint32_t groups = (ncand + SEED_WAVES - 1u) / SEED_WAVES;
    const uint32_t fits_a_launch = seed::fits_a_launch(groups, limit);
    for (uint32_t fit = 0u; fit < nfits;) {
        const uint32_t count = std::min(fits_a_launch, nfits - fit);
        hipLaunchKernelGGL(k_seed_scores, dim3(count * groups), dim3(SEED_BLOCK), 0, stream, *seeder, nchannels, d_channel_pos, ncand, d_cand, groups, fit,
                           sc.offsets, sc.tau0, hits, sc.best0, d_scores);
        HIP_TRY(hipGetLastError());
        fit += count;
    }
    // levels 1 .. L and the results: a block per fit, all levels of a fit in its one launch
    const SeedResults out{d_best_pos, d_best_score, d_best_bin, d_best_cand, d_outside, d_level_score};
    for (uint32_t fit = 0u; fit < nfits;) {
        const uint32_t count = std::min(limit, nfits - fit);
        hipLaunchKernelGGL(k_seed_refine, dim3(count), dim3(SEED_BLOCK), 0, stream, *seeder, nchannels, d_channel_pos, ncand, d_cand, fit, sc.offsets, sc.tau0,
                           hits, sc.best0, out);
        HIP_TRY(hipGetLastError());
        fit += count;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

}  // extern "C"
