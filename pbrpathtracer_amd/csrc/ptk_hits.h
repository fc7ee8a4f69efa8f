// Closest-hit and occlusion queries for caller-supplied rays (include/ptk.h ptk_intersect_rays, ptk_occluded_rays): the parameter
// block and launchers of the kernels in ptk_hits.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value: 27 dwords, preloaded into SGPRs.  hits_kernel writes the hit outputs that are not null (tri, t, bary, material);
// occluded_kernel reads tmax where it is not null and writes occluded.
struct HitsParams {
    const float4* nodes;        // the scene tables of RenderParams
    const float4* tris;
    const float4* shade;
    const int4* texinfo;
    const uint32_t* texels;
    const float* origins;       // [num_rays][3]
    const float* dirs;          // [num_rays][3], used as given
    const float* tmax;          // [num_rays] or null: +inf (occluded_kernel)
    int32_t* tri;               // [num_rays], -1 on a miss
    float* t;                   // [num_rays], +inf on a miss
    float* bary;                // [num_rays][2], 0 on a miss
    int32_t* material;          // [num_rays], -1 on a miss
    uint8_t* occluded;          // [num_rays] (occluded_kernel)
    int num_rays;               // > 0
    int num_nodes;              // > 0: a scene without triangles never gets here (the API fills the outputs)
    float scene_bound;
    int tri_thr;                // the walk's triangle-arm vote (RenderParams::tri_thr): speed only
    uint32_t seed_lo, seed_hi, sample, key_base;
};

// one one-wave workgroup per 64 consecutive rays
void launch_hits(const HitsParams& h, hipStream_t stream);
void launch_occluded(const HitsParams& h, hipStream_t stream);

}  // namespace ptk
