// Closest-point queries (include/ptk.h ptk_closest_points): the parameter block and launcher of the kernel in ptk_closest.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// The prune's slack: a child is dropped only when its box lies farther than sqrt(best) * (1 + PTK_CLOSEST_REL)
// + PTK_CLOSEST_K * 2^-21 * (max |p| + scene_bound).
#define PTK_CLOSEST_K 2.0f
#define PTK_CLOSEST_REL 0x1p-19f

// By value, preloaded into SGPRs.  closest_kernel writes the outputs that are not null.
struct ClosestParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float* points;        // [num_points][3]
    const float* max_dist;      // [num_points] or null: +inf
    int32_t* tri;               // [num_points], -1 on a miss
    float* dist;                // [num_points], +inf on a miss
    float* point;               // [num_points][3], 0 on a miss
    float* bary;                // [num_points][2], 0 on a miss
    unsigned long long* stats;  // [2] node visits, triangle tests, added to (the STATS variant only: ptk_closest_stats)
    int num_points;             // > 0
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
};

// one one-wave workgroup per 64 consecutive points; the variant that counts when h.stats is not null
void launch_closest(const ClosestParams& h, hipStream_t stream);

}  // namespace ptk
