// HIP kernels for gfx950 of guided upsampling (include/ptk.h ptk_upsample_planes, ptk_upsample_frame).
//   * upsample_pack_kernel - the SoA low planes into float4 images over the SMALL image, so that a tap is three 16-byte loads, four
//     with albedo: ci = (colour, id bits), px = (position, 0), nz = (normal, 0), al = (albedo, 0).  Its ACCUM instantiations take the
//     colour from the accumulator, S1 / n_p in registers, exactly as the display transform's frame entry takes it;
//   * upsample_kernel - one thread per HIGH pixel: its place in the low image, the four bilinear taps in the rule's order behind the
//     id, tangent-plane and normal tests, the twelve taps of ring 1 where ring 0 took nothing, the hole's nearest pixel otherwise,
//     the re-modulation with the high albedo.  The high guides are read in place.
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/upsample_rule.py).  No atomics, no LDS, no persistent waves; the loops are the four and
// the sixteen taps.
#include "ptk_device_fn.h"
#include "ptk_upsample.h"

namespace ptk {

__device__ __forceinline__ float up_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// pixel (x, y) of a launch of UP_BLOCK_X x UP_BLOCK_Y blocks; false off the image
__device__ __forceinline__ bool up_pixel(const int width, const int height, int& x, int& y)
{
    x = blockIdx.x * UP_BLOCK_X + threadIdx.x;
    y = blockIdx.y * UP_BLOCK_Y + threadIdx.y;
    return x < width && y < height;
}

template <int KIND, bool ALBEDO>
__global__ __launch_bounds__(UP_BLOCK_X * UP_BLOCK_Y) void upsample_pack_kernel(const UpsamplePackParams P, const UpsampleImages im)
{
    int x, y;
    if (!up_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    float c0 = P.color[3 * i], c1 = P.color[3 * i + 1], c2 = P.color[3 * i + 2];
    if (KIND != UPSAMPLE_SRC_PLANE)
    {
        // the accumulator: S1 / (float)n_p, 0 where n_p = 0
        const uint32_t n = KIND == UPSAMPLE_SRC_ACCUM_COUNTS ? P.counts[i] : (uint32_t)P.samples;
        const float nf = (float)n;
        const bool have = n > 0u;
        c0 = have ? c0 / nf : 0.0f; c1 = have ? c1 / nf : 0.0f; c2 = have ? c2 / nf : 0.0f;
    }
    im.ci[i] = make_float4(c0, c1, c2, __int_as_float(P.id[i]));
    im.px[i] = make_float4(P.position[3 * i], P.position[3 * i + 1], P.position[3 * i + 2], 0.0f);
    im.nz[i] = make_float4(P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2], 0.0f);
    if (ALBEDO) im.al[i] = make_float4(P.albedo[3 * i], P.albedo[3 * i + 1], P.albedo[3 * i + 2], 0.0f);
}

// One low tap's texels, read from a clamped (always on-image) address: `in` says whether the tap itself lies in the low image.
struct UpTap {
    float4 ci, px, nz, al;
    bool in;
};

template <bool ALBEDO>
__device__ __forceinline__ UpTap up_load(const UpsampleParams& P, const int tx, const int ti)
{
    UpTap t;
    t.in = tx >= 0 && tx < P.w && ti >= 0 && ti < P.h;
    const int cx = tx < 0 ? 0 : (tx > P.w - 1 ? P.w - 1 : tx), ci = ti < 0 ? 0 : (ti > P.h - 1 ? P.h - 1 : ti);
    // top-down row ci is plane row h-1-ci
    const size_t iq = (size_t)(P.h - 1 - ci) * P.w + cx;
    t.ci = P.lo.ci[iq]; t.px = P.lo.px[iq]; t.nz = P.lo.nz[iq];
    if (ALBEDO) t.al = P.lo.al[iq];
    return t;
}

// The rule's acceptance of tap t for the high pixel (id, X, n), and its sums
template <bool ALBEDO>
__device__ __forceinline__ void up_take(const UpsampleParams& P, const UpTap& t, const float b, const int id, const float X0, const float X1,
                                        const float X2, const float n0, const float n1, const float n2, float& s0, float& s1, float& s2, float& sw)
{
    const int idq = __float_as_int(t.ci.w);
    bool ok;
    if (id < 0) ok = idq < 0;
    else
    {
        const float z = up_dot(n0, n1, n2, t.px.x - X0, t.px.y - X1, t.px.z - X2);
        const float cn = up_dot(n0, n1, n2, t.nz.x, t.nz.y, t.nz.z);
        ok = idq == id && z * z <= P.zz && cn >= P.min_normal_dot;
    }
    if (!(t.in && ok && b > 0.0f)) return;
    float v0 = t.ci.x, v1 = t.ci.y, v2 = t.ci.z;
    if (ALBEDO && idq >= 0) { v0 = v0 / (t.al.x + 0.00390625f); v1 = v1 / (t.al.y + 0.00390625f); v2 = v2 / (t.al.z + 0.00390625f); }
    s0 = s0 + (b * v0); s1 = s1 + (b * v1); s2 = s2 + (b * v2);
    sw = sw + b;
}

template <bool ALBEDO>
__global__ __launch_bounds__(UP_BLOCK_X * UP_BLOCK_Y) void upsample_kernel(const UpsampleParams P)
{
    int x, y;
    if (!up_pixel(P.W, P.H, x, y)) return;
    const size_t ip = (size_t)y * P.W + x;
    const int i = P.H - 1 - y;                                 // the top-down row of plane row y
    const int id = P.hi_id[ip];
    const float X0 = P.hi_position[3 * ip], X1 = P.hi_position[3 * ip + 1], X2 = P.hi_position[3 * ip + 2];
    const float n0 = P.hi_normal[3 * ip], n1 = P.hi_normal[3 * ip + 1], n2 = P.hi_normal[3 * ip + 2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (ALBEDO) { a0 = P.hi_albedo[3 * ip]; a1 = P.hi_albedo[3 * ip + 1]; a2 = P.hi_albedo[3 * ip + 2]; }
    const float col = (((float)x + 0.5f) * P.sx) - 0.5f, row = (((float)i + 0.5f) * P.sy) - 0.5f;
    const int x0 = (int)floorf(col), i0 = (int)floorf(row);
    const float fx = col - (float)x0, fy = row - (float)i0;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float b[4] = { gx * gy, fx * gy, gx * fy, fx * fy };
    // the loads of the four taps are issued together, then tested and summed in the rule's order
    UpTap t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = up_load<ALBEDO>(P, x0 + (k & 1), i0 + (k >> 1));
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) up_take<ALBEDO>(P, t[k], b[k], id, X0, X1, X2, n0, n1, n2, s0, s1, s2, sw);
    int cls = 0;
    // the rare path (silhouettes and thin features): a wave no lane of which needs it skips the block
    if (!(sw > 0.0f) && P.wide)
    {
        cls = 1;
        s0 = s1 = s2 = sw = 0.0f;
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                if ((j == 1 || j == 2) && (k == 1 || k == 2)) continue;
                const int tx = x0 - 1 + k, ti = i0 - 1 + j;
                const float dx = (float)tx - col, dy = (float)ti - row;
                const float bw = 1.0f / (1.0f + ((dx * dx) + (dy * dy)));
                const UpTap q = up_load<ALBEDO>(P, tx, ti);
                up_take<ALBEDO>(P, q, bw, id, X0, X1, X2, n0, n1, n2, s0, s1, s2, sw);
            }
    }
    float o0, o1, o2;
    if (sw > 0.0f)
    {
        o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw;
        if (ALBEDO && id >= 0) { o0 = o0 * (a0 + 0.00390625f); o1 = o1 * (a1 + 0.00390625f); o2 = o2 * (a2 + 0.00390625f); }
    }
    else
    {
        // a hole: the nearest low pixel's colour, its bits (the clamps also bound the conversions: col and row are finite)
        cls = 2;
        int xn = (int)floorf(col + 0.5f), in = (int)floorf(row + 0.5f);
        xn = xn < 0 ? 0 : (xn > P.w - 1 ? P.w - 1 : xn);
        in = in < 0 ? 0 : (in > P.h - 1 ? P.h - 1 : in);
        const float4 c = P.lo.ci[(size_t)(P.h - 1 - in) * P.w + xn];
        o0 = c.x; o1 = c.y; o2 = c.z;
    }
    P.out_color[3 * ip] = o0; P.out_color[3 * ip + 1] = o1; P.out_color[3 * ip + 2] = o2;
    P.out_class[ip] = cls;
}

static dim3 up_grid(int width, int height) { return dim3((width + UP_BLOCK_X - 1) / UP_BLOCK_X, (height + UP_BLOCK_Y - 1) / UP_BLOCK_Y); }
static const dim3 up_block(UP_BLOCK_X, UP_BLOCK_Y);

template <bool ALBEDO>
static void launch_upsample_pack_as(const UpsamplePackParams& p, const UpsampleImages& im, hipStream_t stream)
{
    const dim3 grid = up_grid(p.width, p.height);
    if (p.kind == UPSAMPLE_SRC_ACCUM_COUNTS) hipLaunchKernelGGL((upsample_pack_kernel<UPSAMPLE_SRC_ACCUM_COUNTS, ALBEDO>), grid, up_block, 0, stream, p, im);
    else if (p.kind == UPSAMPLE_SRC_ACCUM_SAMPLES) hipLaunchKernelGGL((upsample_pack_kernel<UPSAMPLE_SRC_ACCUM_SAMPLES, ALBEDO>), grid, up_block, 0, stream, p, im);
    else hipLaunchKernelGGL((upsample_pack_kernel<UPSAMPLE_SRC_PLANE, ALBEDO>), grid, up_block, 0, stream, p, im);
}

void launch_upsample_pack(const UpsamplePackParams& p, const UpsampleImages& im, hipStream_t stream)
{
    if (p.albedo) launch_upsample_pack_as<true>(p, im, stream);
    else launch_upsample_pack_as<false>(p, im, stream);
}

void launch_upsample(const UpsampleParams& p, hipStream_t stream)
{
    const dim3 grid = up_grid(p.W, p.H);
    if (p.lo.al) hipLaunchKernelGGL((upsample_kernel<true>), grid, up_block, 0, stream, p);
    else hipLaunchKernelGGL((upsample_kernel<false>), grid, up_block, 0, stream, p);
}

}  // namespace ptk
