// HIP kernel for gfx950 of the moving-geometry half of temporal reprojection (include/ptk.h ptk_render_motion,
// ptk_temporal_frame_moving).
//   * motion_kernel - one thread per pixel: where the surface point this pixel sees was when the geometry snapshot was taken (X'),
//     the pixel's normal in that triangle's previous frame (n'), and the screen-space motion vector of X' under a view.
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/motion_rule.py).  No atomics, no LDS, no loop; the two 36-byte vertex records of a
// pixel's triangle are plain global loads (neighbouring lanes mostly share a triangle, so they mostly share the cache lines).
#include "ptk_device_fn.h"
#include "ptk_motion.h"
#include "ptk_temporal.h"

namespace ptk {

__device__ __forceinline__ float mv_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
    return ((ax * bx) + (ay * by)) + (az * bz);
}

struct mv_vec { float x, y, z; };
__device__ __forceinline__ mv_vec mv_cross(const mv_vec a, const mv_vec b)
{
    return { (a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x) };
}
__device__ __forceinline__ mv_vec mv_sub(const mv_vec a, const mv_vec b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }

__global__ __launch_bounds__(TP_BLOCK_X * TP_BLOCK_Y) void motion_kernel(const MotionParams P)
{
    const int x = blockIdx.x * TP_BLOCK_X + threadIdx.x, y = blockIdx.y * TP_BLOCK_Y + threadIdx.y;
    if (x >= P.width || y >= P.height) return;
    const size_t ip = (size_t)y * P.width + x;
    const int k = P.tri[ip];
    const float X0 = P.position[3 * ip], X1 = P.position[3 * ip + 1], X2 = P.position[3 * ip + 2];
    const float n0 = P.normal[3 * ip], n1 = P.normal[3 * ip + 1], n2 = P.normal[3 * ip + 2];
    float Y0 = X0, Y1 = X1, Y2 = X2, m0 = n0, m1 = n1, m2 = n2;      // a miss and an unmoved triangle: the planes' bits
    // (a triangle index from before an upload of a smaller scene names no record: unmoved)
    if (k >= 0 && k < P.num_tris && P.prev)
    {
        const float* a = P.verts + (size_t)k * 9;
        const float* b = P.prev + (size_t)k * 9;
        float c[9], p[9];
        bool moved = false;
#pragma unroll
        for (int j = 0; j < 9; j++) { c[j] = a[j]; p[j] = b[j]; moved = moved || !(c[j] == p[j]); }
        if (moved)
        {
            const float u = P.bary[2 * ip], v = P.bary[2 * ip + 1];
            const float w = (1.0f - u) - v;
            Y0 = X0 + ((((p[0] - c[0]) * w) + ((p[3] - c[3]) * u)) + ((p[6] - c[6]) * v));
            Y1 = X1 + ((((p[1] - c[1]) * w) + ((p[4] - c[4]) * u)) + ((p[7] - c[7]) * v));
            Y2 = X2 + ((((p[2] - c[2]) * w) + ((p[5] - c[5]) * u)) + ((p[8] - c[8]) * v));
            const mv_vec v0 = { c[0], c[1], c[2] }, v1 = { c[3], c[4], c[5] }, v2 = { c[6], c[7], c[8] };
            const mv_vec q0 = { p[0], p[1], p[2] }, q1 = { p[3], p[4], p[5] }, q2 = { p[6], p[7], p[8] };
            const mv_vec e1 = mv_sub(v1, v0), e2 = mv_sub(v2, v0), N = mv_cross(e1, e2);
            const mv_vec f1 = mv_sub(q1, q0), f2 = mv_sub(q2, q0), M = mv_cross(f1, f2);
            const float ca = mv_dot(n0, n1, n2, e1.x, e1.y, e1.z), cb = mv_dot(n0, n1, n2, e2.x, e2.y, e2.z), cc = mv_dot(n0, n1, n2, N.x, N.y, N.z);
            const mv_vec A = mv_cross(f2, M), B = mv_cross(M, f1);
            const float nn = mv_dot(M.x, M.y, M.z, M.x, M.y, M.z);
            m0 = (((ca * A.x) + (cb * B.x)) + (cc * M.x)) / nn;
            m1 = (((ca * A.y) + (cb * B.y)) + (cc * M.y)) / nn;
            m2 = (((ca * A.z) + (cb * B.z)) + (cc * M.z)) / nn;
        }
    }
    float mx = __int_as_float(0x7fc00000), my = mx;
    if (k >= 0 && P.have_view)
    {
        const float d0 = Y0 - P.pos[0], d1 = Y1 - P.pos[1], d2 = Y2 - P.pos[2];
        const float den = mv_dot(d0, d1, d2, P.nrm[0], P.nrm[1], P.nrm[2]);
        const float s = P.num / den;
        const float Q0 = (d0 * s) - P.e[0], Q1 = (d1 * s) - P.e[1], Q2 = (d2 * s) - P.e[2];
        const float col = mv_dot(Q0, Q1, Q2, P.right[0], P.right[1], P.right[2]) / P.delta_x;
        const float row = (0.0f - mv_dot(Q0, Q1, Q2, P.up[0], P.up[1], P.up[2])) / P.delta_y;
        // plane row y is top-down row H-1-y
        if (s > 0.0f) { mx = col - (float)x; my = row - (float)(P.height - 1 - y); }
    }
    P.prev_position[3 * ip] = Y0; P.prev_position[3 * ip + 1] = Y1; P.prev_position[3 * ip + 2] = Y2;
    P.prev_normal[3 * ip] = m0; P.prev_normal[3 * ip + 1] = m1; P.prev_normal[3 * ip + 2] = m2;
    P.motion[2 * ip] = mx; P.motion[2 * ip + 1] = my;
}

void launch_motion(const MotionParams& p, hipStream_t stream)
{
    const dim3 grid((p.width + TP_BLOCK_X - 1) / TP_BLOCK_X, (p.height + TP_BLOCK_Y - 1) / TP_BLOCK_Y);
    hipLaunchKernelGGL(motion_kernel, grid, dim3(TP_BLOCK_X, TP_BLOCK_Y), 0, stream, p);
}

}  // namespace ptk
