// The a-trous denoiser (include/ptk.h ptk_denoise_planes, ptk_denoise_frame): parameter blocks and launchers of
// the kernels in ptk_denoise.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// 64 x 4 pixels per workgroup: the tap of a wave is one contiguous row of 64 float4 (1 KiB)
constexpr int DN_BLOCK_X = 64, DN_BLOCK_Y = 4;

// The packed images of a call, each [H][W] float4: g0 = (normal.xyz, valid ? 1 : 0), g1 = (position.xyz, 0), and the two ping-pong
// images c[2] = (c.rgb, variance).  Iteration k reads c[k & 1] and writes c[(k + 1) & 1].
struct DenoiseImages {
    float4* g0;
    float4* g1;
    float4* c[2];
};

// By value, preloaded into SGPRs.  Planes as the header lists them; albedo and variance may be null.
struct DenoisePackParams {
    const float* color;         // [H][W][3]
    const int32_t* mask;        // [H][W], valid iff >= 0
    const float* normal;        // [H][W][3]
    const float* position;      // [H][W][3]
    const float* albedo;        // [H][W][3] or null
    const float* variance;      // [H][W] or null
    int width, height;
};

// The frame entry's pack: colour, validity and variance from the accumulator and the feature planes (all rows bottom-up).
struct DenoiseFramePackParams {
    const float* accum;         // [H][W][3] S1
    const float* moments;       // [H][W][3] S2, or null: no variance
    const uint32_t* counts;     // [H][W] per-pixel counts of an adaptive render, or null: `samples` on the owned pixels
    const int32_t* triangle;    // the feature planes
    const float* emission;
    const float* normal;
    const float* position;
    const float* albedo;
    int width, height;
    int samples;
    int rank, world;
};

struct DenoiseFilterParams {
    const float4* g0;
    const float4* g1;
    const float4* in;
    float4* out;
    int width, height;
    int s;                      // tap spacing 1 << k
    int iterations;             // of the call (1..8); the kernel uses s alone
    int normal_squarings;       // 0..7
    int have_variance;
    float sigma_z, sigma_l;
};

struct DenoiseUnpackParams {
    const float4* g0;
    const float4* c;            // the last iteration's output
    const float* albedo;        // [H][W][3] or null
    float* out_color;           // [H][W][3]
    float* out_variance;        // [H][W] or null
    int width, height;
};

void launch_denoise_pack(const DenoisePackParams& p, const DenoiseImages& im, hipStream_t stream);
void launch_denoise_pack_frame(const DenoiseFramePackParams& p, const DenoiseImages& im, hipStream_t stream);
void launch_denoise_filter(const DenoiseFilterParams& p, hipStream_t stream);
void launch_denoise_unpack(const DenoiseUnpackParams& p, hipStream_t stream);
// out[i] = resolve8(in[i]) for n floats (ptk_resolve_denoised_rgb8)
void launch_denoise_resolve8(const float* in, uint8_t* out, size_t n, hipStream_t stream);

}  // namespace ptk
