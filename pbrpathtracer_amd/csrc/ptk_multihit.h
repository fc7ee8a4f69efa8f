// Ordered multi-hit ray queries (include/ptk.h ptk_multihit_rays): the parameter block and launcher of the kernel in ptk_multihit.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value, preloaded into SGPRs.  One ray (origins[i], dirs[i]) per lane, bounded by tmax[i]; the kernel writes the first max_hits
// columns of every output that is not null.
struct MultihitParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float* origins;       // [num][3]
    const float* dirs;          // [num][3], used as given
    const float* tmax;          // [num] or null: +inf
    int32_t* count;             // [num] min(max_hits, crossings)
    int32_t* tri;               // [num][max_hits], -1 behind count
    float* t;                   // [num][max_hits], +inf behind count
    float* bary;                // [num][max_hits][2], 0 behind count
    int8_t* side;               // [num][max_hits] +1 front, -1 back, 0 behind count
    int num;                    // > 0
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
    int tri_thr;                // the walk's triangle-arm vote (RenderParams::tri_thr): speed only
    int max_hits;               // 1 .. PTK_MULTIHIT_MAX
};

// one one-wave workgroup per 64 consecutive rays; the instantiation is the smallest list of {1, 2, 4, 8, 16} that holds max_hits
void launch_multihit(const MultihitParams& h, hipStream_t stream);

}  // namespace ptk
