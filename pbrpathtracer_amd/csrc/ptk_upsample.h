// Guided upsampling (include/ptk.h ptk_upsample_planes, ptk_upsample_frame): parameter blocks and launchers of the
// kernels in ptk_upsample.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// 64 x 4 pixels per workgroup, as the temporal kernel's: a wave writes contiguous rows of 64 pixels
constexpr int UP_BLOCK_X = 64, UP_BLOCK_Y = 4;

// The low image in the packed layout, each image [h][w] float4, rows bottom-up: a tap is three 16-byte loads, four with albedo.
struct UpsampleImages {
    float4* ci;                 // (color.rgb, the id's bits)
    float4* px;                 // (position.xyz, 0)
    float4* nz;                 // (normal.xyz, 0)
    float4* al;                 // (albedo.rgb, 0), or null: no albedo planes
};

// Where the low colour comes from: a plane [h][w][3] as it is, or the accumulator S1 divided by the pixel's count n_p - per-pixel
// counts after an adaptive render, else `samples` - exactly as the display transform's frame entry takes it
enum { UPSAMPLE_SRC_PLANE = 0, UPSAMPLE_SRC_ACCUM_COUNTS = 1, UPSAMPLE_SRC_ACCUM_SAMPLES = 2 };

// The SoA low planes into the packed layout.
struct UpsamplePackParams {
    const float* color;         // [h][w][3]: the plane, or S1
    const uint32_t* counts;     // [h][w] (ACCUM_COUNTS) or null
    int samples;                // (ACCUM_SAMPLES)
    int kind;                   // UPSAMPLE_SRC_*
    const int32_t* id;          // [h][w]
    const float* position;      // [h][w][3]
    const float* normal;        // [h][w][3]
    const float* albedo;        // [h][w][3] or null
    int width, height;
};

// By value, preloaded into SGPRs.  The once-per-call values of the rule (sx, sy, zz) are computed by the host, in float32.
struct UpsampleParams {
    UpsampleImages lo;
    int w, h;
    const int32_t* hi_id;       // [H][W]
    const float* hi_position;   // [H][W][3]
    const float* hi_normal;     // [H][W][3]
    const float* hi_albedo;     // [H][W][3], present exactly when lo.al is
    float* out_color;           // [H][W][3]
    int32_t* out_class;         // [H][W]
    int W, H;
    float sx, sy, zz, min_normal_dot;
    int wide;
};

void launch_upsample_pack(const UpsamplePackParams& p, const UpsampleImages& im, hipStream_t stream);
void launch_upsample(const UpsampleParams& p, hipStream_t stream);

}  // namespace ptk
