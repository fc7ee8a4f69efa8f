// Variance of the accumulated demodulated luminance from its temporal moments (include/ptk.h ptk_variance_planes,
// ptk_temporal_variance, ptk_denoise_temporal): parameter blocks and launchers of the kernels in ptk_variance.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// 64 x 4 pixels per workgroup, as the denoiser's and the reprojection's: a wave's tap is one contiguous row of 64 float4 (1 KiB)
constexpr int VR_BLOCK_X = 64, VR_BLOCK_Y = 4;

// What a pixel and a tap are read from, each image [H][W] float4, rows as stored: the layout of a moments history set
// (ptk_temporal.h), so that ptk_temporal_variance reads what temporal_kernel has just written and packs nothing.
struct VarianceImages {
    float4* mm;                 // (m1, m2, count - 0 where id < 0 or !(count > 0): no variance -, the frame's own count)
    float4* pi;                 // (position.xyz, the id's bits)
    float4* nz;                 // (normal.xyz, 0)
};

// The caller's SoA planes into that layout (the planes entries).
struct VariancePackParams {
    const float* moments;       // [H][W][2]
    const float* count;         // [H][W]
    const float* frame_count;   // [H][W]
    const int32_t* id;          // [H][W]
    const float* position;      // [H][W][3]
    const float* normal;        // [H][W][3]
    int width, height;
};

// By value, preloaded into SGPRs.
struct VarianceParams {
    const float4* mm;
    const float4* pi;
    const float4* nz;
    float* raw;                 // [H][W]: the variance before the prefilter
    int width, height;
    int radius;                 // 1..3
    int mark;                   // a prefilter follows: a pixel that may not be its tap (id < 0 or !(count > 0)) gets -1, not 0
    float min_frames, zz, min_normal_dot;
};

struct VariancePrefilterParams {
    const float* raw;           // [H][W], marked
    float* out;                 // [H][W]
    int width, height;
};

void launch_variance_pack(const VariancePackParams& p, const VarianceImages& im, hipStream_t stream);
void launch_variance(const VarianceParams& p, hipStream_t stream);
void launch_variance_prefilter(const VariancePrefilterParams& p, hipStream_t stream);
// ptk_denoise_temporal's mask: 0 where count > 0, triangle >= 0 and the three channels of emission equal 0, else -1
void launch_temporal_mask(const float* count, const int32_t* triangle, const float* emission, int32_t* mask, int width, int height,
                          hipStream_t stream);

}  // namespace ptk
