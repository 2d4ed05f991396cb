// seed_host.cpp -- chroma_vertex_seed_host: the vertex seed as plain loops over fit, position and hit on the host (one thread),
// over the same functions as the device kernels (seed_common.h).  What the CPU tests run, what VertexSeeder.fit_many computes
// without a GPU, and the yardstick of tools/seed_probe.py.
#include <stdint.h>
#include <vector>

#include "seed_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

namespace {

struct Fit {
    const chroma_vertex_seeder &p;
    uint32_t nchannels;
    const int32_t *channel_pos;
    int32_t tau0;
    uint32_t n;
    const int32_t *channel, *time;
    const uint32_t *weight;
    std::vector<uint32_t> &H;          // nbins + K words

    // the key (score, bin) of the position (x, y, z) and its OUTSIDE hits
    uint64_t at(int32_t x, int32_t y, int32_t z, uint32_t *outside) const
    {
        const uint32_t span = p.nbins * p.bin_ticks;
        H.assign(p.nbins + p.nshape, 0u);
        uint32_t out = 0u;
        for (uint32_t i = 0; i < n; i++) {
            const int32_t c = channel[i];
            if (c < 0 || (uint32_t)c >= nchannels) { out++; continue; }
            const uint64_t d = seed::distance(channel_pos[3 * (size_t)c], channel_pos[3 * (size_t)c + 1], channel_pos[3 * (size_t)c + 2], x, y, z);
            const uint32_t b = seed::bin_of(time[i], seed::time_of_flight(d, p.slowness), tau0, p.bin_ticks, span);
            if (b == seed::OUTSIDE) { out++; continue; }
            H[b] += weight[i] < seed::MAX_WEIGHT ? weight[i] : seed::MAX_WEIGHT;
        }
        uint64_t best = 0u;
        for (uint32_t s = 0; s < p.nbins; s++) {
            uint32_t A = 0u;
            for (uint32_t j = 0; j < p.nshape; j++) A += p.shape[j] * H[s + j];
            const uint64_t key = seed::key_of(A, s);
            best = key > best ? key : best;
        }
        *outside = out;
        return best;
    }
};

}  // namespace

extern "C" {

int chroma_vertex_seed_host(const chroma_vertex_seeder *seeder, uint32_t nchannels, const int32_t *channel_pos, uint32_t ncand, const int32_t *cand,
                            uint32_t nfits, const uint32_t *offsets, const int32_t *tau0, const int32_t *hit_channel, const int32_t *hit_time,
                            const uint32_t *hit_weight, int32_t *best_pos, uint32_t *best_score, uint32_t *best_bin, uint32_t *best_cand,
                            uint32_t *outside, uint32_t *level_score, uint32_t *scores)
{
    if (!seeder || (nfits && (!cand || !offsets || !tau0 || !best_pos || !best_score || !best_bin || !best_cand || !outside || !level_score)) ||
        (nfits && nchannels && !channel_pos))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = seed::check(seeder, nchannels, ncand, nfits, offsets, scores != nullptr)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (nfits == 0) return CHROMA_OK;
    if (offsets[nfits] && (!hit_channel || !hit_time || !hit_weight)) return set_error(CHROMA_ERR_INVALID, "bad argument");
    for (uint64_t i = 0; i < 3ull * nchannels; i++)
        if (!seed::coordinate_ok(channel_pos[i])) return set_error(CHROMA_ERR_INVALID, "vertex seed: a channel's coordinate is beyond 2^23");
    for (uint64_t i = 0; i < 3ull * ncand; i++)
        if (!seed::coordinate_ok(cand[i])) return set_error(CHROMA_ERR_INVALID, "vertex seed: a candidate's coordinate is beyond 2^23");
    const chroma_vertex_seeder &p = *seeder;
    std::vector<uint32_t> H;
    for (uint32_t f = 0; f < nfits; f++) {
        const uint32_t first = offsets[f];
        const Fit fit{p, nchannels, channel_pos, tau0[f], offsets[f + 1] - first, hit_channel + first, hit_time + first, hit_weight + first, H};
        uint32_t out = 0u;
        uint64_t best0 = 0u;
        for (uint32_t c = 0; c < ncand; c++) {
            const uint64_t key = fit.at(cand[3 * (size_t)c], cand[3 * (size_t)c + 1], cand[3 * (size_t)c + 2], &out);
            if (scores) scores[(size_t)f * ncand + c] = seed::key_score(key);
            const uint64_t k0 = seed::key_of(seed::key_score(key), c);
            best0 = k0 > best0 ? k0 : best0;
        }
        const uint32_t c0 = seed::key_index(best0);
        int32_t x = cand[3 * (size_t)c0], y = cand[3 * (size_t)c0 + 1], z = cand[3 * (size_t)c0 + 2];
        uint32_t *ls = level_score + (size_t)f * (p.nlevels + 1u);
        ls[0] = seed::key_score(best0);
        for (uint32_t l = 1; l <= p.nlevels; l++) {
            const uint32_t s = seed::level_spacing(p, l);
            uint64_t best = 0u;
            for (uint32_t m = 0; m < seed::LATTICE; m++) {
                int32_t px, py, pz;
                seed::lattice(m, s, x, y, z, &px, &py, &pz);
                const uint64_t k = seed::key_of(seed::key_score(fit.at(px, py, pz, &out)), seed::lattice_rank(m));
                best = k > best ? k : best;
            }
            seed::lattice(seed::lattice_point(seed::key_index(best)), s, x, y, z, &x, &y, &z);
            ls[l] = seed::key_score(best);
        }
        const uint64_t last = fit.at(x, y, z, &out);
        best_pos[3 * (size_t)f] = x; best_pos[3 * (size_t)f + 1] = y; best_pos[3 * (size_t)f + 2] = z;
        best_score[f] = seed::key_score(last); best_bin[f] = seed::key_index(last); best_cand[f] = c0; outside[f] = out;
    }
    return CHROMA_OK;
}

}  // extern "C"
