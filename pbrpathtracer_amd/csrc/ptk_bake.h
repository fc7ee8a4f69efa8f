// Lightmap baking (include/ptk.h ptk_bake_lightmap): parameter block and launchers of the kernels in ptk_bake.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

#define PTK_BAKE_UNOWNED 0x7fffffff     // owner plane before / without a covering triangle (INT_MAX: atomicMin's neutral element)

struct BakeParams {
    const float* uvs;           // [num_tris][6] in this GPU's memory, or null: the uvs of the shading records
    const float4* shade;        // shading records: s0.xyz the face normal, s1 / s2.xy the scene's own uvs
    const float* verts;         // [num_tris][9] resident world-space vertices
    int num_tris;
    int width, height;
    float offset;               // ray origin = P + n * offset
    int back;                   // 1: n is the negated face normal (PTK_BAKE_BACK)
    uint32_t key_base;
    int* plane;                 // [H][W] smallest covering triangle index, PTK_BAKE_UNOWNED where none
    uint32_t* block_counts;     // covered texels per block of 256 texels; after the scan: covered texels in the blocks before it
    // what bake_rays_kernel writes; each may be null
    int32_t* owner;             // [H][W], -1 uncovered
    float* bary;                // [H][W][2] (b2, b3), 0 uncovered
    float* pos;                 // [H][W][3] surface point, 0 uncovered
    // compacted covered texels in ascending texel index (null: none is written - coverage only)
    float* origins; float* dirs; uint32_t* keys; uint32_t* texel;
    float* sums;                // [covered][3]: under PTK_BAKE_ACCUMULATE loaded with out[texel] here
    const float* out;           // the caller's image, read under PTK_BAKE_ACCUMULATE only (else null)
};

// plane <- the smallest covering triangle per texel (the plane must hold PTK_BAKE_UNOWNED before)
void launch_bake_cover(const BakeParams& p, hipStream_t stream);
// block_counts <- exclusive prefix of the covered texels per block; *total <- their number
void launch_bake_count(const BakeParams& p, uint32_t* total, hipStream_t stream);
// the scan alone: counts[0 .. n) <- their exclusive prefix sums, *total <- their sum (ptk_rays_adaptive.hip compacts with it)
void launch_bake_scan(uint32_t* counts, uint32_t n, uint32_t* total, hipStream_t stream);
void launch_bake_rays(const BakeParams& p, hipStream_t stream);
// out[texel[i]] = sums[i]
void launch_bake_scatter(const float* sums, const uint32_t* texel, uint32_t count, float* out, hipStream_t stream);
// one dilation pass from (src_image, src_owner) to (dst_image, dst_owner)
void launch_dilate(const float* src_image, const int32_t* src_owner, float* dst_image, int32_t* dst_owner, int width, int height, hipStream_t stream);

}  // namespace ptk
