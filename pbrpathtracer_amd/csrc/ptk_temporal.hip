// HIP kernels for gfx950 of temporal reprojection (include/ptk.h ptk_reproject_planes, ptk_temporal_frame).
//   * temporal_pack_kernel - the caller's SoA history planes into float4 images, so that a tap is three 16-byte loads:
//     cn = (colour, count), pi = (position, id bits), nz = (normal, 0);
//   * temporal_kernel - one thread per pixel: projection of its first-hit position into the history's view, the four bilinear taps
//     in the rule's order, the blend; writes the SoA outputs and - in the frame entry - the next history in the packed layout.
//     Its MOVING instantiations project the point's previous place instead (ptk.h ptk_temporal_frame_moving);
//     its MOMENTS instantiations carry the two moments of demodulated luminance in a fourth image mm = (m1, m2, count, the frame's
//     own count) beside the colour (ptk.h ptk_temporal_frame_moments).
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/temporal_rule.py).  No atomics, no LDS, no persistent waves; the only loop is the four taps.
#include "ptk_device_fn.h"
#include "ptk_temporal.h"

namespace ptk {

__device__ __forceinline__ float tp_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// pixel (x, y) of a launch of TP_BLOCK_X x TP_BLOCK_Y blocks; false off the image
__device__ __forceinline__ bool tp_pixel(const int width, const int height, int& x, int& y)
{
    x = blockIdx.x * TP_BLOCK_X + threadIdx.x;
    y = blockIdx.y * TP_BLOCK_Y + threadIdx.y;
    return x < width && y < height;
}

__global__ __launch_bounds__(TP_BLOCK_X * TP_BLOCK_Y) void temporal_pack_kernel(const TemporalPackParams P, const TemporalImages im)
{
    int x, y;
    if (!tp_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    im.cn[i] = make_float4(P.color[3 * i], P.color[3 * i + 1], P.color[3 * i + 2], P.count[i]);
    im.pi[i] = make_float4(P.position[3 * i], P.position[3 * i + 1], P.position[3 * i + 2], __int_as_float(P.id[i]));
    im.nz[i] = make_float4(P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2], 0.0f);
}

__global__ __launch_bounds__(TP_BLOCK_X * TP_BLOCK_Y) void temporal_pack_moments_kernel(const float* __restrict__ moments, float4* __restrict__ mm,
                                                                                       const int width, const int height)
{
    int x, y;
    if (!tp_pixel(width, height, x, y)) return;
    const size_t i = (size_t)y * width + x;
    mm[i] = make_float4(moments[2 * i], moments[2 * i + 1], 0.0f, 0.0f);
}

// FRAME: the current colour and count come from the accumulator (n_p and S1 / n_p exactly as denoise_pack_frame_kernel has them).
// The loads of the four taps are issued together from clamped (always on-image) addresses; a tap off the image is then dropped
// by its predicate with the others, so nothing it holds reaches a sum.
// MOVING: everything that is geometry of the history - the projected point and the two tap tests - takes X' and n' from the planes
// motion_kernel wrote (ptk_motion.hip); the next history still holds the unprimed X and n.
// MOMENTS: the two moments of demodulated luminance are one more pair of channels of every tap and of the blend (ptk.h
// ptk_reproject_moments); the colour and the count are computed by the very expressions of the plain instantiations.
template <bool FRAME, bool MOVING, bool MOMENTS>
__global__ __launch_bounds__(TP_BLOCK_X * TP_BLOCK_Y) void temporal_kernel(const TemporalParams P)
{
    int x, y;
    if (!tp_pixel(P.width, P.height, x, y)) return;
    const size_t ip = (size_t)y * P.width + x;
    float c0, c1, c2, nc;
    if (FRAME)
    {
        uint32_t n;
        if (P.counts) n = P.counts[ip];
        else
        {
            // rows are stored bottom-up; the tiles count from the image's top-left (tile_origin's map, inverted)
            const int ty = (P.height - 1 - y) / PTK_TILE, tx = x / PTK_TILE, tiles_x = (P.width + PTK_TILE - 1) / PTK_TILE;
            const int tile = ty * tiles_x + (tx + 3 * ty) % tiles_x;
            n = tile % P.world == P.rank ? (uint32_t)P.samples : 0u;
        }
        nc = (float)n;
        c0 = c1 = c2 = 0.0f;
        if (n > 0u) { c0 = P.accum[3 * ip] / nc; c1 = P.accum[3 * ip + 1] / nc; c2 = P.accum[3 * ip + 2] / nc; }
    }
    else { c0 = P.color[3 * ip]; c1 = P.color[3 * ip + 1]; c2 = P.color[3 * ip + 2]; nc = P.count[ip]; }
    const int id = P.id[ip];
    const float X0 = P.position[3 * ip], X1 = P.position[3 * ip + 1], X2 = P.position[3 * ip + 2];
    const float n0 = P.normal[3 * ip], n1 = P.normal[3 * ip + 1], n2 = P.normal[3 * ip + 2];
    float o0 = c0, o1 = c1, o2 = c2, on = nc;                  // an invalid pixel and a pixel without history: the input bits
    float cm1 = 0.0f, cm2 = 0.0f;                              // the current moments: 0 for an invalid pixel and for one without samples
    if (MOMENTS && id >= 0 && nc > 0.0f)
    {
        float l0 = c0, l1 = c1, l2 = c2;
        if (P.albedo)
        {
            l0 = c0 / (P.albedo[3 * ip] + 0.00390625f); l1 = c1 / (P.albedo[3 * ip + 1] + 0.00390625f); l2 = c2 / (P.albedo[3 * ip + 2] + 0.00390625f);
        }
        const float l = ((0.2126f * l0) + (0.7152f * l1)) + (0.0722f * l2);
        cm1 = l; cm2 = l * l;
    }
    float om1 = cm1, om2 = cm2;
    if (id >= 0 && P.hist.cn)
    {
        const float Y0 = MOVING ? P.prev_position[3 * ip] : X0, Y1 = MOVING ? P.prev_position[3 * ip + 1] : X1, Y2 = MOVING ? P.prev_position[3 * ip + 2] : X2;
        const float m0 = MOVING ? P.prev_normal[3 * ip] : n0, m1 = MOVING ? P.prev_normal[3 * ip + 1] : n1, m2 = MOVING ? P.prev_normal[3 * ip + 2] : n2;
        const float d0 = Y0 - P.pos[0], d1 = Y1 - P.pos[1], d2 = Y2 - P.pos[2];
        const float den = tp_dot(d0, d1, d2, P.nrm[0], P.nrm[1], P.nrm[2]);
        const float s = P.num / den;
        const float Q0 = (d0 * s) - P.e[0], Q1 = (d1 * s) - P.e[1], Q2 = (d2 * s) - P.e[2];
        const float col = tp_dot(Q0, Q1, Q2, P.right[0], P.right[1], P.right[2]) / P.delta_x;
        const float row = (0.0f - tp_dot(Q0, Q1, Q2, P.up[0], P.up[1], P.up[2])) / P.delta_y;
        // (every comparison is false for NaN; they also bound the conversions below)
        if (s > 0.0f && col > -1.0f && col < (float)P.width && row > -1.0f && row < (float)P.height)
        {
            const int x0 = (int)floorf(col), i0 = (int)floorf(row);
            const float fx = col - (float)x0, fy = row - (float)i0;
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            const float b[4] = { gx * gy, fx * gy, gx * fy, fx * fy };
            float4 hc[4], hp[4], hn[4], hm[4];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const int qx = x0 + (k & 1), qi = i0 + (k >> 1);
                in[k] = qx >= 0 && qx < P.width && qi >= 0 && qi < P.height;
                // top-down row qi is plane row H-1-qi
                const size_t iq = in[k] ? (size_t)(P.height - 1 - qi) * P.width + qx : ip;
                hc[k] = P.hist.cn[iq]; hp[k] = P.hist.pi[iq]; hn[k] = P.hist.nz[iq];
                if (MOMENTS) hm[k] = P.hist_mm[iq];
            }
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f, sw = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const int hid = __float_as_int(hp[k].w);
                const float z = tp_dot(m0, m1, m2, hp[k].x - Y0, hp[k].y - Y1, hp[k].z - Y2);
                const float cn = tp_dot(m0, m1, m2, hn[k].x, hn[k].y, hn[k].z);
                if (in[k] && hid >= 0 && (!P.match_id || hid == id) && hc[k].w > 0.0f && b[k] > 0.0f && z * z <= P.zz && cn >= P.min_normal_dot)
                {
                    s0 = s0 + (b[k] * hc[k].x); s1 = s1 + (b[k] * hc[k].y); s2 = s2 + (b[k] * hc[k].z);
                    sn = sn + (b[k] * hc[k].w);
                    sw = sw + b[k];
                    if (MOMENTS) { sm1 = sm1 + (b[k] * hm[k].x); sm2 = sm2 + (b[k] * hm[k].y); }
                }
            }
            if (sw > 0.0f)
            {
                const float h0 = s0 / sw, h1 = s1 / sw, h2 = s2 / sw;
                float hw = sn / sw;
                hw = hw > P.max_history ? P.max_history : hw;
                const float hm1 = MOMENTS ? sm1 / sw : 0.0f, hm2 = MOMENTS ? sm2 / sw : 0.0f;
                if (nc == 0.0f) { o0 = h0; o1 = h1; o2 = h2; on = hw; om1 = hm1; om2 = hm2; }
                else
                {
                    const float tot = hw + nc;
                    o0 = ((h0 * hw) + (c0 * nc)) / tot; o1 = ((h1 * hw) + (c1 * nc)) / tot; o2 = ((h2 * hw) + (c2 * nc)) / tot;
                    on = tot;
                    if (MOMENTS) { om1 = ((hm1 * hw) + (cm1 * nc)) / tot; om2 = ((hm2 * hw) + (cm2 * nc)) / tot; }
                }
            }
        }
    }
    P.out_color[3 * ip] = o0; P.out_color[3 * ip + 1] = o1; P.out_color[3 * ip + 2] = o2;
    P.out_count[ip] = on;
    if (P.next.cn)
    {
        P.next.cn[ip] = make_float4(o0, o1, o2, on);
        P.next.pi[ip] = make_float4(X0, X1, X2, __int_as_float(id));
        P.next.nz[ip] = make_float4(n0, n1, n2, 0.0f);
    }
    if (MOMENTS)
    {
        P.out_moments[2 * ip] = om1; P.out_moments[2 * ip + 1] = om2;
        // (the blended count - 0 where the pixel can have no variance - and the frame's own ride along: variance_kernel reads a
        // pixel's four numbers in one load)
        if (P.next_mm) P.next_mm[ip] = make_float4(om1, om2, id >= 0 && on > 0.0f ? on : 0.0f, nc);
    }
}

static dim3 tp_grid(int width, int height) { return dim3((width + TP_BLOCK_X - 1) / TP_BLOCK_X, (height + TP_BLOCK_Y - 1) / TP_BLOCK_Y); }
static const dim3 tp_block(TP_BLOCK_X, TP_BLOCK_Y);

void launch_temporal_pack(const TemporalPackParams& p, const TemporalImages& im, hipStream_t stream)
{
    hipLaunchKernelGGL(temporal_pack_kernel, tp_grid(p.width, p.height), tp_block, 0, stream, p, im);
}

void launch_temporal_pack_moments(const float* moments, float4* mm, int width, int height, hipStream_t stream)
{
    hipLaunchKernelGGL(temporal_pack_moments_kernel, tp_grid(width, height), tp_block, 0, stream, moments, mm, width, height);
}

template <bool MOMENTS>
static void launch_temporal_as(const TemporalParams& p, hipStream_t stream)
{
    const dim3 grid = tp_grid(p.width, p.height);
    if (p.prev_position)
    {
        if (p.accum) hipLaunchKernelGGL((temporal_kernel<true, true, MOMENTS>), grid, tp_block, 0, stream, p);
        else hipLaunchKernelGGL((temporal_kernel<false, true, MOMENTS>), grid, tp_block, 0, stream, p);
    }
    else if (p.accum) hipLaunchKernelGGL((temporal_kernel<true, false, MOMENTS>), grid, tp_block, 0, stream, p);
    else hipLaunchKernelGGL((temporal_kernel<false, false, MOMENTS>), grid, tp_block, 0, stream, p);
}

void launch_temporal(const TemporalParams& p, hipStream_t stream)
{
    if (p.out_moments) launch_temporal_as<true>(p, stream);
    else launch_temporal_as<false>(p, stream);
}

}  // namespace ptk
