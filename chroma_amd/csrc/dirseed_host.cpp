// dirseed_host.cpp -- chroma_direction_seed_host: the direction seed as plain loops over fit, point and hit on the host (one
// thread), over the same functions as the device kernels (dirseed_common.h).  What the CPU tests run, what
// DirectionSeeder.fit_many computes without a GPU, and the yardstick of tools/dirseed_probe.py.
#include <stdint.h>
#include <vector>

#include "dirseed_common.h"

// (context.hip: the calling thread's chroma_last_error() message; chroma_internal.h declares it for the device units)
__attribute__((visibility("hidden"))) int set_error(int code, const char *fmt, ...);

namespace {

struct Record { int32_t x, y, z; uint32_t w; };

// score(f, u) over the fit's INSIDE hits
uint32_t score_of(const chroma_direction_seeder &p, const std::vector<Record> &records, int32_t ux, int32_t uy, int32_t uz)
{
    if (!(ux | uy | uz)) return 0u;
    uint32_t score = 0u;
    for (const Record &r : records) score += r.w * p.profile[dirseed::cos_bin(dirseed::cosine(r.x, r.y, r.z, ux, uy, uz), p.log2_ncos)];
    return score;
}

}  // namespace

extern "C" {

int chroma_direction_seed_host(const chroma_direction_seeder *seeder, const chroma_vertex_seeder *timing, uint32_t nchannels, const int32_t *channel_pos,
                               uint32_t ncand, const int32_t *cand, uint32_t nfits, const uint32_t *offsets, const int32_t *tau0, const int32_t *vertex,
                               const uint32_t *bin, const int32_t *hit_channel, const int32_t *hit_time, const uint32_t *hit_weight, int32_t *best_dir,
                               uint32_t *best_score, uint32_t *best_cand, uint32_t *inside, uint32_t *outside, uint32_t *level_score, uint32_t *cos_hist)
{
    const bool timed = hit_time != nullptr;
    if (!seeder || (nfits && (!cand || !offsets || !vertex || !best_dir || !best_score || !best_cand || !inside || !outside || !level_score)) ||
        (nfits && nchannels && !channel_pos) || (nfits && timed && (!timing || !tau0 || !bin)))
        return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (const char *why = dirseed::check(seeder, timed ? timing : nullptr, nchannels, ncand, nfits, offsets)) return set_error(CHROMA_ERR_INVALID, "%s", why);
    if (nfits == 0) return CHROMA_OK;
    if (offsets[nfits] && (!hit_channel || !hit_weight)) return set_error(CHROMA_ERR_INVALID, "bad argument");
    for (uint64_t i = 0; i < 3ull * nchannels; i++)
        if (!seed::coordinate_ok(channel_pos[i])) return set_error(CHROMA_ERR_INVALID, "direction seed: a channel's coordinate is beyond 2^23");
    for (uint64_t i = 0; i < 3ull * nfits; i++)
        if (!seed::coordinate_ok(vertex[i])) return set_error(CHROMA_ERR_INVALID, "direction seed: a vertex's coordinate is beyond 2^23");
    for (uint64_t i = 0; i < 3ull * ncand; i++)
        if (!dirseed::component_ok(cand[i])) return set_error(CHROMA_ERR_INVALID, "direction seed: a candidate's component is beyond 2^15");
    const chroma_direction_seeder &p = *seeder;
    const uint32_t ncos = 1u << p.log2_ncos;
    std::vector<Record> records;
    for (uint32_t f = 0; f < nfits; f++) {
        // the per-hit work, once
        records.clear();
        uint32_t in = 0u, out = 0u;
        for (uint32_t i = offsets[f]; i < offsets[f + 1]; i++) {
            Record r;
            if (dirseed::hit_record(p, timing, nchannels, channel_pos, hit_channel[i], timed, timed ? hit_time[i] : 0, hit_weight[i], vertex[3 * (size_t)f],
                                    vertex[3 * (size_t)f + 1], vertex[3 * (size_t)f + 2], timed ? tau0[f] : 0, timed ? bin[f] : 0u, &r.w, &r.x, &r.y, &r.z)) {
                in += r.w;
                records.push_back(r);
            } else
                out++;
        }
        // level 0
        uint64_t best0 = 0u;
        for (uint32_t c = 0; c < ncand; c++) {
            int32_t ux, uy, uz;
            dirseed::unit_of_point(cand[3 * (size_t)c], cand[3 * (size_t)c + 1], cand[3 * (size_t)c + 2], &ux, &uy, &uz);
            const uint64_t k0 = seed::key_of(score_of(p, records, ux, uy, uz), c);
            best0 = k0 > best0 ? k0 : best0;
        }
        const uint32_t c0 = seed::key_index(best0);
        int32_t x, y, z;
        dirseed::unit_of_point(cand[3 * (size_t)c0], cand[3 * (size_t)c0 + 1], cand[3 * (size_t)c0 + 2], &x, &y, &z);
        uint32_t *ls = level_score + (size_t)f * (p.nlevels + 1u);
        ls[0] = seed::key_score(best0);
        for (uint32_t l = 1; l <= p.nlevels; l++) {
            const uint32_t s = seed::level_spacing(p, l);
            uint64_t best = 0u;
            int32_t bx = x, by = y, bz = z;
            for (uint32_t m = 0; m < seed::LATTICE; m++) {
                int32_t ux = x, uy = y, uz = z;          // (the centre as it is)
                if (m != seed::CENTRE) {
                    seed::lattice(m, s, x, y, z, &ux, &uy, &uz);
                    dirseed::unit_of_point(ux, uy, uz, &ux, &uy, &uz);
                }
                const uint64_t k = seed::key_of(score_of(p, records, ux, uy, uz), seed::lattice_rank(m));
                if (k > best) { best = k; bx = ux; by = uy; bz = uz; }
            }
            x = bx; y = by; z = bz;
            ls[l] = seed::key_score(best);
        }
        best_dir[3 * (size_t)f] = x; best_dir[3 * (size_t)f + 1] = y; best_dir[3 * (size_t)f + 2] = z;
        best_score[f] = ls[p.nlevels]; best_cand[f] = c0; inside[f] = in; outside[f] = out;
        if (cos_hist) {
            uint32_t *h = cos_hist + ((size_t)f << p.log2_ncos);
            for (uint32_t k = 0; k < ncos; k++) h[k] = 0u;
            for (const Record &r : records) h[dirseed::cos_bin(dirseed::cosine(r.x, r.y, r.z, x, y, z), p.log2_ncos)] += r.w;
        }
    }
    return CHROMA_OK;
}

}  // extern "C"
