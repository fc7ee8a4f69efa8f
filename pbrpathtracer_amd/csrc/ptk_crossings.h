// Crossing counts, point containment and the sign of a distance (include/ptk.h ptk_crossings_rays, ptk_contains_points,
// ptk_signed_distance): the parameter block and launchers of the kernels in ptk_crossings.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value, preloaded into SGPRs.  crossings_kernel: one ray (origins[i], dirs[i]) per lane, bounded by tmax[i]; it writes front and
// back where they are not null.  contains_kernel: one point origins[i] per lane and the num_dirs directions of dirs (null: the
// built-in set) one after the other for the whole wave; it writes inside and winding where they are not null and sets the sign bit
// of dist[i] where the point is inside.
struct CrossingsParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float* origins;       // [num][3]: ray origins / points
    const float* dirs;          // crossings_kernel: [num][3], used as given; contains_kernel: [num_dirs][3] or null
    const float* tmax;          // [num] or null: +inf (crossings_kernel)
    int32_t* front;             // [num] crossings with a > 0 (crossings_kernel)
    int32_t* back;              // [num] crossings with a < 0
    uint8_t* inside;            // [num] (contains_kernel)
    int32_t* winding;           // [num][num_dirs] back - front
    float* dist;                // [num] in / out: ptk_signed_distance's, written by closest_kernel before
    int num;                    // > 0
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
    int tri_thr;                // the walk's triangle-arm vote (RenderParams::tri_thr): speed only
    int num_dirs;               // odd, 1 .. 31 (contains_kernel)
    int mode;                   // PTK_INSIDE_WINDING / PTK_INSIDE_PARITY
};

// one one-wave workgroup per 64 consecutive rays / points
void launch_crossings(const CrossingsParams& h, hipStream_t stream);
void launch_contains(const CrossingsParams& h, hipStream_t stream);

}  // namespace ptk
