// Temporal reprojection (include/ptk.h ptk_reproject_planes, ptk_temporal_frame): parameter blocks and launchers of
// the kernels in ptk_temporal.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// 64 x 4 pixels per workgroup, as the denoiser's: a wave reads and writes contiguous rows of 64 float4 (1 KiB)
constexpr int TP_BLOCK_X = 64, TP_BLOCK_Y = 4;

// A history in the packed layout, each image [H][W] float4, rows bottom-up: a tap is three 16-byte loads.
struct TemporalImages {
    float4* cn;                 // (color.rgb, count)
    float4* pi;                 // (position.xyz, the id's bits)
    float4* nz;                 // (normal.xyz, 0)
};

// The caller's SoA history planes into the packed layout (the planes entries).
struct TemporalPackParams {
    const float* color;         // [H][W][3]
    const float* count;         // [H][W]
    const int32_t* id;          // [H][W]
    const float* position;      // [H][W][3]
    const float* normal;        // [H][W][3]
    int width, height;
};

// By value, preloaded into SGPRs.  The once-per-call values of the rule (nrm, e, num, zz) are computed by the host, in float32.
struct TemporalParams {
    // the current frame: either the caller's planes ...
    const float* color;         // [H][W][3]
    const float* count;         // [H][W]
    // ... or the accumulator (the frame entry): count = n_p, color = S1 / n_p
    const float* accum;         // [H][W][3] S1
    const uint32_t* counts;     // [H][W] per-pixel counts of an adaptive render, or null: `samples` on the owned pixels
    int samples, rank, world;
    const int32_t* id;          // [H][W]
    const float* position;      // [H][W][3]
    const float* normal;        // [H][W][3]
    TemporalImages hist;        // cn null: no history, the output is the current frame
    TemporalImages next;        // cn null: not written (the planes entries)
    float* out_color;           // [H][W][3]
    float* out_count;           // [H][W]
    int width, height;
    float pos[3], right[3], up[3], e[3], nrm[3];
    float num, delta_x, delta_y, zz, min_normal_dot, max_history;
    int match_id;
    // moving mode (ptk_reproject_planes_moving, ptk_temporal_frame_moving; ptk_motion.h): where the current frame's points and
    // normals were in the history's geometry.  Both null: the plain rule.  (Last, so that the fields above keep their offsets.)
    const float* prev_position; // [H][W][3]
    const float* prev_normal;   // [H][W][3]
    // moments mode (ptk_reproject_moments, ptk_temporal_frame_moments; ptk_variance.h): the first and second moment of demodulated
    // luminance ride through the same taps.  out_moments null: the plain rule.  (Last again, for the same reason.)
    const float* albedo;        // [H][W][3], or null: no demodulation
    const float4* hist_mm;      // the history's fourth packed image (m1, m2, count or 0, the frame's own count; ptk_variance.h); read with hist.cn
    float4* next_mm;            // ... and the next history's, written with next.cn
    float* out_moments;         // [H][W][2]
};

void launch_temporal_pack(const TemporalPackParams& p, const TemporalImages& im, hipStream_t stream);
// its sibling for the moments entries: mm = (m1, m2, 0, 0) from the caller's [H][W][2] plane
void launch_temporal_pack_moments(const float* moments, float4* mm, int width, int height, hipStream_t stream);
void launch_temporal(const TemporalParams& p, hipStream_t stream);

}  // namespace ptk
