// bvh_result.h -- what chroma_bvh_build (host, bvh_build.cpp) and chroma_bvh_build_device (bvh_device.hip) hand back
// behind the same opaque handle: chroma_bvh_fetch / _data / _free serve both.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>
#include "uninit_vector.h"

namespace chroma_host {
struct Node { uint32_t x, y, z, w; };
struct BvhResult {
    uninit_vector<Node> nodes;
    std::vector<uint64_t> layer_bounds;   // nlayers + 1 entries
};

// What both builders refuse before any work is done; nullptr when the call can go ahead.
//   * target_degree < 2: with distinct Morton codes a layer of n nodes gets n one-child parents and the tree never closes;
//   * a frame that cannot quantise: (v - origin) / scale is NaN or inf for every vertex, and what the conversion to
//     uint32 makes of that differs between the host and the device.
inline const char *bvh_refusal(const float world_origin[3], float world_scale, int32_t target_degree)
{
    if (target_degree < 2) return "target_degree must be at least 2";
    if (!world_origin) return "bad argument";
    if (!std::isfinite(world_scale) || !(world_scale > 0.0f)) return "world_scale must be finite and positive (a mesh without extent, or with non-finite vertices)";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(world_origin[k])) return "world_origin must be finite (a mesh with non-finite vertices)";
    return nullptr;
}
}  // namespace chroma_host
