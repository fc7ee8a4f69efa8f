// K-nearest triangle queries (include/ptk.h ptk_nearest_triangles): the parameter block and launcher of the kernel in ptk_knearest.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value, preloaded into SGPRs.  One point per lane, bounded by max_dist[i]; the kernel writes the first k columns of every output
// that is not null.
struct NearestParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float* points;        // [num_points][3]
    const float* max_dist;      // [num_points] or null: +inf
    int32_t* count;             // [num_points] min(k, accepted)
    int32_t* tri;               // [num_points][k], -1 behind count
    float* dist;                // [num_points][k], +inf behind count
    float* point;               // [num_points][k][3], 0 behind count
    float* bary;                // [num_points][k][2], 0 behind count
    unsigned long long* stats;  // [2] node visits, triangle tests, added to (the STATS variants only: ptk_nearest_stats)
    int num_points;             // > 0
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
    int k;                      // 1 .. PTK_NEAREST_MAX_K
};

// one one-wave workgroup per 64 consecutive points; the instantiation is the smallest list of {1, 4, 16} that holds k, its counting
// variant when h.stats is not null
void launch_nearest(const NearestParams& h, hipStream_t stream);

}  // namespace ptk
