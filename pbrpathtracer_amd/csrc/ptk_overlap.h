// Overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres): the parameter block and launcher of the kernel in
// ptk_overlap.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// The prune's slack is ptk_closest.h's, PTK_CLOSEST_K and PTK_CLOSEST_REL: a child is dropped by a box query only
// when its decoded box lies beyond the query box by more than K * 2^-21 * (max |lo, hi| + scene_bound) on some axis; by a sphere
// query only when its box distance exceeds r * (1 + REL) + the same slack around the centre (the sphere rule is the closest rule's d2k).

enum { OVERLAP_BOX = 0, OVERLAP_SPHERE = 1 };

// By value, preloaded into SGPRs.  overlap_kernel writes the outputs that are not null.
struct OverlapParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float* qa;            // boxes: lo [num][3]; spheres: centers [num][3]
    const float* qb;            // boxes: hi [num][3]; spheres: radius [num]
    const int32_t* tri_from;    // [num] or null: 0
    int32_t* count;             // [num] or null
    int32_t* list;              // [num][k], null with k == 0
    unsigned long long* stats;  // [4] node visits, triangle tests, accepted, records past the three box axes; added to (the STATS
                                // variant only: ptk_overlap_stats)
    int num;                    // > 0
    int k;                      // 0 .. PTK_OVERLAP_MAX_K columns of list
    int shape;                  // OVERLAP_BOX / OVERLAP_SPHERE
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
};

// one one-wave workgroup per 64 consecutive queries; the variant that counts when h.stats is not null
void launch_overlap(const OverlapParams& h, hipStream_t stream);

}  // namespace ptk
