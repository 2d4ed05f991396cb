// dirseed_calls.hip -- the direction seed's entry point (kernels_dirseed.h): chroma_direction_seed is a pipeline on the context's
// pooled scratch block -- the two host arrays copied up, the validation pass over the three device arrays of coordinates and its
// verdict read back, a record per hit (k_dir_prepare), the level-0 scores of every (fit, candidate), then the refinement of every
// fit through all its levels in one launch (batches beyond a launch's blocks take several of each).
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "chroma_internal.h"

#include "kernels_dirseed.h"

static_assert(sizeof(chroma_direction_seeder) == 276, "chroma_direction_seeder is 276 bytes (include/chroma_hip.h)");
static_assert(sizeof(DirLds) + 4 * 256 + DIRSEED_WAVES * 8 + 8 <= DIRSEED_LDS_BYTES, "the direction seed kernels' LDS (DESIGN 3.10)");
static_assert(DIRSEED_CHUNK == DIRSEED_BLOCK, "a thread stages one record of a chunk");
static_assert(dirseed::ONE + 2 * (int32_t)dirseed::MAX_STEP <= dirseed::MAX_COMPONENT, "a lattice point is a point");

// The call's share of the context's scratch block, in this order: the validation's verdict, the offsets, tau0, the level-0 maxima,
// the hits' records
struct DirScratch {
    uint32_t *bad, *offsets; int32_t *tau0; unsigned long long *best0; uint2 *records;

    void lay(Carver &c, size_t nfits, size_t nhits)
    {
        bad = c.take<uint32_t>(1);
        offsets = c.take<uint32_t>(nfits + 1);
        tau0 = c.take<int32_t>(nfits);
        best0 = c.take<unsigned long long>(nfits);
        records = c.take<uint2>(nhits);
    }
};

// The blocks of one launch: fewer than 2^32 threads, CHROMA_SEED_LAUNCH_BLOCKS in the environment lowers it (as seed_calls.hip's:
// how tests/test_gpu_dirseed.py makes a small batch take several launches of each kernel; the results do not depend on it)
static uint32_t dir_launch_limit(uint32_t block)
{
    const uint32_t most = seed::launch_blocks(block);
    if (const char *e = getenv("CHROMA_SEED_LAUNCH_BLOCKS")) {
        const long long v = atoll(e);
        if (v >= 1 && v < (long long)most) return (uint32_t)v;
    }
    return most;
}
static_assert((uint64_t)seed::launch_blocks(DIRSEED_BLOCK) * DIRSEED_BLOCK < (1ull << 32) &&
              (uint64_t)seed::launch_blocks(DIRSEED_PREPARE_BLOCK) * DIRSEED_PREPARE_BLOCK < (1ull << 32) &&
              seed::launch_blocks(DIRSEED_BLOCK) >= (seed::MAX_CAND + DIRSEED_WAVES - 1) / DIRSEED_WAVES,
              "a launch stays under 2^32 threads and holds one fit's candidates");

extern "C" {

int chroma_direction_seed(chroma_ctx *ctx, const chroma_direction_seeder *seeder, const chroma_vertex_seeder *timing, uint32_t nchannels,
                          const int32_t *d_channel_pos, uint32_t ncand, const int32_t *d_cand, uint32_t nfits, const uint32_t *offsets, const int32_t *tau0,
                          const int32_t *d_vertex, const uint32_t *d_bin, const int32_t *d_hit_channel, const int32_t *d_hit_time, const uint32_t *d_hit_weight,
                          int32_t *d_best_dir, uint32_t *d_best_score, uint32_t *d_best_cand, uint32_t *d_inside, uint32_t *d_outside, uint32_t *d_level_score,
                          uint32_t *d_cos_hist)
{
    const bool timed = d_hit_time != nullptr;
    if (!ctx || !seeder ||
        (nfits && (!d_cand || !offsets || !d_vertex || !d_best_dir || !d_best_score || !d_best_cand || !d_inside || !d_outside || !d_level_score)) ||
        (nfits && nchannels && !d_channel_pos) || (nfits && timed && (!timing || !tau0 || !d_bin)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = dirseed::check(seeder, timed ? timing : nullptr, nchannels, ncand, nfits, offsets)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (nfits == 0) return CHROMA_OK;
    const uint32_t nhits = offsets[nfits];
    if (nhits && (!d_hit_channel || !d_hit_weight)) return set_error(CHROMA_ERR_INVALID, "bad argument");
    const CallScope scope(ctx);
    hipStream_t stream = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    DirScratch sc;
    int rc = carve_call_scratch(scope, [&](Carver &c) { sc.lay(c, nfits, nhits); }); if (rc) return rc;
    // The two host arrays up, and the validation pass of the three device arrays with its verdict before anything is written.
    // Whatever fails in between, the stream is drained before the call returns: the caller's host arrays are his again.
    uint32_t bad = 0u;
    const auto validate = [&]() -> int {
        HIP_TRY(hipMemsetAsync(sc.bad, 0, sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(sc.best0, 0, (size_t)nfits * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemcpyAsync(sc.offsets, offsets, ((size_t)nfits + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        if (timed) HIP_TRY(hipMemcpyAsync(sc.tau0, tau0, (size_t)nfits * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        if (nchannels) {          // (3 * nchannels < 2^32: dirseed::check)
            hipLaunchKernelGGL(k_dir_check, dim3((3u * nchannels + 255u) / 256u), dim3(256), 0, stream, d_channel_pos, 3u * nchannels, seed::MAX_COORD, sc.bad);
            HIP_TRY(hipGetLastError());
        }
        for (uint64_t at = 0u; at < 3ull * nfits;) {          // (3 * nfits < 2^33: two launches at the most)
            const uint32_t count = (uint32_t)std::min<uint64_t>(3ull * nfits - at, 1ull << 31);
            hipLaunchKernelGGL(k_dir_check, dim3((count + 255u) / 256u), dim3(256), 0, stream, d_vertex + at, count, seed::MAX_COORD, sc.bad);
            HIP_TRY(hipGetLastError());
            at += count;
        }
        hipLaunchKernelGGL(k_dir_check, dim3((3u * ncand + 255u) / 256u), dim3(256), 0, stream, d_cand, 3u * ncand, dirseed::MAX_COMPONENT, sc.bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, sc.bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
        return CHROMA_OK;
    };
    rc = validate();
    const hipError_t drained = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIP_TRY(drained);
    if (bad) return set_error(CHROMA_ERR_INVALID, "direction seed: a coordinate of a channel or of a vertex is beyond 2^23, or a candidate's component beyond 2^15");
    // the records: a thread per hit, and the fits' inside and outside sums
    HIP_TRY(hipMemsetAsync(d_inside, 0, (size_t)nfits * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(d_outside, 0, (size_t)nfits * sizeof(uint32_t), stream));
    const DirHits hits{d_hit_channel, d_hit_time, d_hit_weight};
    const chroma_vertex_seeder none = {};
    const uint32_t prepare_limit = dir_launch_limit(DIRSEED_PREPARE_BLOCK);
    for (uint32_t hit = 0u; hit < nhits;) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(prepare_limit, ((uint64_t)(nhits - hit) + DIRSEED_PREPARE_BLOCK - 1u) / DIRSEED_PREPARE_BLOCK);
        const uint32_t upto = (uint32_t)std::min<uint64_t>(nhits, (uint64_t)hit + (uint64_t)blocks * DIRSEED_PREPARE_BLOCK);
        hipLaunchKernelGGL(k_dir_prepare, dim3(blocks), dim3(DIRSEED_PREPARE_BLOCK), 0, stream, *seeder, timed ? *timing : none, nchannels, d_channel_pos, nfits,
                           sc.offsets, sc.tau0, d_vertex, d_bin, hits, hit, upto, sc.records, d_inside, d_outside);
        HIP_TRY(hipGetLastError());
        hit = upto;
    }
    // level 0: eight candidates a block, whole fits a launch, as many as a launch's blocks hold
    const uint32_t limit = dir_launch_limit(DIRSEED_BLOCK);
    const uint32_t groups = (ncand + DIRSEED_WAVES - 1u) / DIRSEED_WAVES;
    const uint32_t fits_a_launch = seed::fits_a_launch(groups, limit);
    for (uint32_t fit = 0u; fit < nfits;) {
        const uint32_t count = std::min(fits_a_launch, nfits - fit);
        hipLaunchKernelGGL(k_dir_scores, dim3(count * groups), dim3(DIRSEED_BLOCK), 0, stream, *seeder, ncand, d_cand, groups, fit, sc.offsets, sc.records, sc.best0);
        HIP_TRY(hipGetLastError());
        fit += count;
    }
    // levels 1 .. L, cos_hist and the results: a block per fit, all levels of a fit in its one launch
    const DirResults out{d_best_dir, d_best_score, d_best_cand, d_level_score, d_cos_hist};
    for (uint32_t fit = 0u; fit < nfits;) {
        const uint32_t count = std::min(limit, nfits - fit);
        hipLaunchKernelGGL(k_dir_refine, dim3(count), dim3(DIRSEED_BLOCK), 0, stream, *seeder, ncand, d_cand, fit, sc.offsets, sc.records, sc.best0, out);
        HIP_TRY(hipGetLastError());
        fit += count;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return CHROMA_OK;
}

}  // extern "C"
