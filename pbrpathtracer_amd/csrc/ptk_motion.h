// Previous-frame geometry of the first hits and screen-space motion vectors (include/ptk.h ptk_render_motion,
// ptk_temporal_frame_moving): parameter block and launcher of the kernel in ptk_motion.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// By value.  The once-per-call values of the projection (nrm, e, num) are computed by the host, in float32, as for TemporalParams.
struct MotionParams {
    const int32_t* tri;         // [H][W] PTK_FEAT_TRIANGLE
    const float* bary;          // [H][W][2]
    const float* position;      // [H][W][3]
    const float* normal;        // [H][W][3]
    const float* verts;         // [num_tris][9] the resident world-space vertices
    const float* prev;          // [num_tris][9] the snapshot, or null: every triangle is unmoved
    int num_tris;
    float* prev_position;       // [H][W][3]
    float* prev_normal;         // [H][W][3]
    float* motion;              // [H][W][2]
    int width, height;
    int have_view;              // 0: motion is NaN everywhere
    float pos[3], right[3], up[3], e[3], nrm[3];
    float num, delta_x, delta_y;
};

void launch_motion(const MotionParams& p, hipStream_t stream);

}  // namespace ptk
