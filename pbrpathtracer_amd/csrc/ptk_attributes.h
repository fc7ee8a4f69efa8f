// Surface attribute queries (include/ptk.h ptk_surface_attributes): the parameter block and launcher of the kernel in
// ptk_attributes.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value.  One query per thread; the kernel computes and writes every output that is not null.
struct AttributeParams {
    const float4* shade;        // the shading records (ptk_device.h)
    const float4* mats;         // the material records
    const int4* texinfo;
    const uint32_t* texels;
    const float* verts;         // [num_tris][9] resident world-space vertices
    const int32_t* tri;         // [num]
    const float* bary;          // [num][2], 8-byte aligned
    const float* dirs;          // [num][3] or null: the shading normal is not flipped
    int32_t* material;          // [num]
    float* uv;                  // [num][2], 8-byte aligned
    float* position;            // [num][3]
    float* normal_geom;         // [num][3]
    float* normal;              // [num][3]
    float* albedo;              // [num][3]
    float* emission;            // [num][3]
    float* gloss;               // [num][2], 8-byte aligned
    float* opacity;             // [num]
    int num;                    // > 0
    int num_tris;               // >= 0: a triangle index outside [0, num_tris) is a miss
};
void launch_attributes(const AttributeParams& p, hipStream_t stream);

}  // namespace ptk
