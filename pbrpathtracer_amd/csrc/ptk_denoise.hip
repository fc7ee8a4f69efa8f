// HIP kernels for gfx950 of the a-trous denoiser (include/ptk.h ptk_denoise_planes, ptk_denoise_frame).
//   * denoise_pack_kernel / denoise_pack_frame_kernel - the caller's SoA planes (or the accumulator and the feature planes) into
//     float4 images, so that a tap is three 16-byte loads: g0 = (normal, valid), g1 = (position, 0), c = (colour, variance);
//   * denoise_filter_kernel - one iteration: one thread per pixel, its 25 taps summed in the rule's order in that thread;
//   * denoise_unpack_kernel - remodulation and the [H][W][3] / [H][W] outputs;
//   * denoise_resolve8_kernel - the frame's 8-bit resolve of a float plane.
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/denoise_rule.py).  No atomics, no persistent waves, every loop bounded by 25 taps.
#include "ptk_device_fn.h"
#include "ptk_denoise.h"

namespace ptk {

#define DN_ALBEDO_EPS 0.00390625f
#define DN_DEN_EPS 1e-10f
#define DN_CENTRE 0.140625f

__device__ __forceinline__ float dn_lum(const float4 c) { return ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z); }
__device__ __forceinline__ float dn_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// pixel (x, y) of a launch of DN_BLOCK_X x DN_BLOCK_Y blocks; false off the image
__device__ __forceinline__ bool dn_pixel(const int width, const int height, int& x, int& y)
{
    x = blockIdx.x * DN_BLOCK_X + threadIdx.x;
    y = blockIdx.y * DN_BLOCK_Y + threadIdx.y;
    return x < width && y < height;
}

__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_pack_kernel(const DenoisePackParams P, const DenoiseImages im)
{
    int x, y;
    if (!dn_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    const bool valid = P.mask[i] >= 0;
    float c0 = P.color[3 * i], c1 = P.color[3 * i + 1], c2 = P.color[3 * i + 2];
    if (valid && P.albedo)
    {
        c0 = c0 / (P.albedo[3 * i] + DN_ALBEDO_EPS);
        c1 = c1 / (P.albedo[3 * i + 1] + DN_ALBEDO_EPS);
        c2 = c2 / (P.albedo[3 * i + 2] + DN_ALBEDO_EPS);
    }
    im.g0[i] = make_float4(P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2], valid ? 1.0f : 0.0f);
    im.g1[i] = make_float4(P.position[3 * i], P.position[3 * i + 1], P.position[3 * i + 2], 0.0f);
    im.c[0][i] = make_float4(c0, c1, c2, P.variance ? P.variance[i] : 0.0f);
}

// The frame entry: n_p, colour = S1 / n_p, validity and - with the moments - the variance of the demodulated mean, then as above.
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_pack_frame_kernel(const DenoiseFramePackParams P, const DenoiseImages im)
{
    int x, y;
    if (!dn_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    uint32_t n;
    if (P.counts) n = P.counts[i];
    else
    {
        // rows are stored bottom-up; the tiles count from the image's top-left (tile_origin's map, inverted)
        const int ty = (P.height - 1 - y) / PTK_TILE, tx = x / PTK_TILE, tiles_x = (P.width + PTK_TILE - 1) / PTK_TILE;
        const int tile = ty * tiles_x + (tx + 3 * ty) % tiles_x;
        n = tile % P.world == P.rank ? (uint32_t)P.samples : 0u;
    }
    const float nf = (float)n;
    const float e0 = P.emission[3 * i], e1 = P.emission[3 * i + 1], e2 = P.emission[3 * i + 2];
    bool valid = n > 0u && P.triangle[i] >= 0 && e0 == 0.0f && e1 == 0.0f && e2 == 0.0f;
    if (P.moments) valid = valid && n >= 2u;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, var = 0.0f;
    if (n > 0u) { m0 = P.accum[3 * i] / nf; m1 = P.accum[3 * i + 1] / nf; m2 = P.accum[3 * i + 2] / nf; }
    float c0 = m0, c1 = m1, c2 = m2;
    if (valid)
    {
        const float A0 = P.albedo[3 * i] + DN_ALBEDO_EPS, A1 = P.albedo[3 * i + 1] + DN_ALBEDO_EPS, A2 = P.albedo[3 * i + 2] + DN_ALBEDO_EPS;
        if (P.moments)
        {
            float v0 = P.moments[3 * i] / nf - m0 * m0, v1 = P.moments[3 * i + 1] / nf - m1 * m1, v2 = P.moments[3 * i + 2] / nf - m2 * m2;
            v0 = v0 < 0.0f ? 0.0f : v0; v1 = v1 < 0.0f ? 0.0f : v1; v2 = v2 < 0.0f ? 0.0f : v2;
            var = (((v0 / (A0 * A0)) + (v1 / (A1 * A1))) + (v2 / (A2 * A2))) / (3.0f * (nf - 1.0f));
        }
        c0 = m0 / A0; c1 = m1 / A1; c2 = m2 / A2;
    }
    im.g0[i] = make_float4(P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2], valid ? 1.0f : 0.0f);
    im.g1[i] = make_float4(P.position[3 * i], P.position[3 * i + 1], P.position[3 * i + 2], 0.0f);
    im.c[0][i] = make_float4(c0, c1, c2, var);
}

// One iteration.  The loads of a row of taps are issued together from clamped (always on-image) addresses; a tap off the image or
// on an invalid pixel is then dropped by its predicate, so nothing it holds - NaN, 1e30 - reaches a sum.  The sums advance tap by
// tap in the rule's order: rows outer, columns inner.
template <bool VAR>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_filter_kernel(const DenoiseFilterParams P)
{
    int x, y;
    if (!dn_pixel(P.width, P.height, x, y)) return;
    const size_t ip = (size_t)y * P.width + x;
    const float4 np = P.g0[ip], cp = P.in[ip];
    if (np.w == 0.0f) { P.out[ip] = cp; return; }          // invalid: copied through, colour and variance alike
    const float4 pp = P.g1[ip];
    const float inv_z = 1.0f / P.sigma_z;
    float den;
    if (VAR) den = ((P.sigma_l * P.sigma_l) * cp.w) + DN_DEN_EPS;
    else { const float sk = P.sigma_l * (1.0f / (float)P.s); den = sk * sk; }      // (s is a power of two: the scaling is exact)
    const float iden = 1.0f / den;
    const float lp = dn_lum(cp);
    const float h[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++)
    {
        const int qy = y + (j - 2) * P.s;
        const bool row_in = qy >= 0 && qy < P.height;
        const size_t row = (size_t)(row_in ? qy : y) * P.width;
        float4 nq[5], pq[5], cq[5];
        bool in[5];
#pragma unroll
        for (int i = 0; i < 5; i++)
        {
            const int qx = x + (i - 2) * P.s;
            in[i] = row_in && qx >= 0 && qx < P.width;
            const size_t iq = row + (size_t)(in[i] ? qx : x);
            nq[i] = P.g0[iq]; pq[i] = P.g1[iq]; cq[i] = P.in[iq];
        }
#pragma unroll
        for (int i = 0; i < 5; i++)
        {
            float w;
            if (j == 2 && i == 2) w = DN_CENTRE;
            else
            {
                float cn = dn_dot(np.x, np.y, np.z, nq[i].x, nq[i].y, nq[i].z);
                cn = cn > 0.0f ? cn : 0.0f;
                for (int q = 0; q < P.normal_squarings; q++) cn = cn * cn;
                const float z = dn_dot(np.x, np.y, np.z, pq[i].x - pp.x, pq[i].y - pp.y, pq[i].z - pp.z) * inv_z;
                const float a = 1.0f + (z * z);
                const float dl = lp - dn_lum(cq[i]);
                const float b = 1.0f + ((dl * dl) * iden);
                w = ((h[j] * h[i]) * cn) / (a * b);
            }
            if (in[i] && nq[i].w != 0.0f && w > 0.0f)
            {
                s0 = s0 + (w * cq[i].x); s1 = s1 + (w * cq[i].y); s2 = s2 + (w * cq[i].z);
                sw = sw + w;
                if (VAR) sv = sv + ((w * w) * cq[i].w);
            }
        }
    }
    P.out[ip] = make_float4(s0 / sw, s1 / sw, s2 / sw, VAR ? sv / (sw * sw) : 0.0f);
}

__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_unpack_kernel(const DenoiseUnpackParams P)
{
    int x, y;
    if (!dn_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    const float4 c = P.c[i];
    float o0 = c.x, o1 = c.y, o2 = c.z;
    if (P.albedo && P.g0[i].w != 0.0f)
    {
        o0 = o0 * (P.albedo[3 * i] + DN_ALBEDO_EPS);
        o1 = o1 * (P.albedo[3 * i + 1] + DN_ALBEDO_EPS);
        o2 = o2 * (P.albedo[3 * i + 2] + DN_ALBEDO_EPS);
    }
    P.out_color[3 * i] = o0; P.out_color[3 * i + 1] = o1; P.out_color[3 * i + 2] = o2;
    if (P.out_variance) P.out_variance[i] = c.w;
}

__global__ __launch_bounds__(256) void denoise_resolve8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, const size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = resolve8(in[i]);
}

static dim3 dn_grid(int width, int height) { return dim3((width + DN_BLOCK_X - 1) / DN_BLOCK_X, (height + DN_BLOCK_Y - 1) / DN_BLOCK_Y); }
static const dim3 dn_block(DN_BLOCK_X, DN_BLOCK_Y);

void launch_denoise_pack(const DenoisePackParams& p, const DenoiseImages& im, hipStream_t stream)
{
    hipLaunchKernelGGL(denoise_pack_kernel, dn_grid(p.width, p.height), dn_block, 0, stream, p, im);
}

void launch_denoise_pack_frame(const DenoiseFramePackParams& p, const DenoiseImages& im, hipStream_t stream)
{
    hipLaunchKernelGGL(denoise_pack_frame_kernel, dn_grid(p.width, p.height), dn_block, 0, stream, p, im);
}

void launch_denoise_filter(const DenoiseFilterParams& p, hipStream_t stream)
{
    if (p.have_variance) hipLaunchKernelGGL(denoise_filter_kernel<true>, dn_grid(p.width, p.height), dn_block, 0, stream, p);
    else hipLaunchKernelGGL(denoise_filter_kernel<false>, dn_grid(p.width, p.height), dn_block, 0, stream, p);
}

void launch_denoise_unpack(const DenoiseUnpackParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(denoise_unpack_kernel, dn_grid(p.width, p.height), dn_block, 0, stream, p);
}

void launch_denoise_resolve8(const float* in, uint8_t* out, size_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(denoise_resolve8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, n);
}

}  // namespace ptk
