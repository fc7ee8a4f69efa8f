// HIP kernels for gfx950 of the temporal variance (include/ptk.h ptk_variance_planes, ptk_temporal_variance, ptk_denoise_temporal;
// DESIGN.md §4.21).
//   * variance_pack_kernel - the caller's SoA planes into the float4 images of a moments history set (the planes entries only: the
//     frame entry reads the set temporal_kernel<.., MOMENTS> has just written);
//   * variance_kernel - one thread per pixel: the temporal estimate from the pixel's own four numbers, or - where the history is
//     short - the spatial estimate over the (2r+1)^2 window, its taps three 16-byte loads each, summed in the rule's order;
//   * variance_prefilter_kernel - the 3x3 binomial over the raw plane;
//   * temporal_mask_kernel - the validity mask ptk_denoise_temporal hands to the denoiser.
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/variance_rule.py).  No atomics, no LDS, no persistent waves; the loops are the window's
// 2r+1 rows of 2r+1 taps and the prefilter's nine.
#include "ptk_device_fn.h"
#include "ptk_variance.h"

namespace ptk {

__device__ __forceinline__ float vr_dot(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// pixel (x, y) of a launch of VR_BLOCK_X x VR_BLOCK_Y blocks; false off the image
__device__ __forceinline__ bool vr_pixel(const int width, const int height, int& x, int& y)
{
    x = blockIdx.x * VR_BLOCK_X + threadIdx.x;
    y = blockIdx.y * VR_BLOCK_Y + threadIdx.y;
    return x < width && y < height;
}

__global__ __launch_bounds__(VR_BLOCK_X * VR_BLOCK_Y) void variance_pack_kernel(const VariancePackParams P, const VarianceImages im)
{
    int x, y;
    if (!vr_pixel(P.width, P.height, x, y)) return;
    const size_t i = (size_t)y * P.width + x;
    const int id = P.id[i];
    const float n = P.count[i];
    im.mm[i] = make_float4(P.moments[2 * i], P.moments[2 * i + 1], id >= 0 && n > 0.0f ? n : 0.0f, P.frame_count[i]);
    im.pi[i] = make_float4(P.position[3 * i], P.position[3 * i + 1], P.position[3 * i + 2], __int_as_float(id));
    im.nz[i] = make_float4(P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2], 0.0f);
}

// The spatial estimate of pixel (x, y): the window's rows outer, its columns inner, both ascending.  The loads of up to VR_TAPS taps
// of a row are issued together from clamped (always on-image) addresses; a tap off the image is then dropped by its predicate with
// the others.  (Three taps at a time, not the whole row: the window is the rare path, and its registers would otherwise halve the
// waves in flight on the common one, which is bound by the latency of its single load.)
constexpr int VR_TAPS = 3;

template <int R>
__device__ __forceinline__ float vr_spatial(const VarianceParams& P, const int x, const int y, const float fr)
{
    const size_t ip = (size_t)y * P.width + x;
    const float4 pp = P.pi[ip], np = P.nz[ip];
    const int id = __float_as_int(pp.w);
    float s1 = 0.0f, s2 = 0.0f, k = 0.0f;
#pragma unroll 1
    for (int dy = -R; dy <= R; dy++)
    {
        const int qy = y + dy;
        const bool row_in = qy >= 0 && qy < P.height;
        const size_t row = (size_t)(row_in ? qy : y) * P.width;
#pragma unroll
        for (int i0 = 0; i0 <= 2 * R; i0 += VR_TAPS)
        {
            float4 mq[VR_TAPS], pq[VR_TAPS], nq[VR_TAPS];
            bool in[VR_TAPS];
#pragma unroll
            for (int t = 0; t < VR_TAPS; t++)
                if (i0 + t <= 2 * R)
                {
                    const int qx = x + (i0 + t - R);
                    in[t] = row_in && qx >= 0 && qx < P.width;
                    const size_t iq = in[t] ? row + (size_t)qx : ip;
                    mq[t] = P.mm[iq]; pq[t] = P.pi[iq]; nq[t] = P.nz[iq];
                }
#pragma unroll
            for (int t = 0; t < VR_TAPS; t++)
                if (i0 + t <= 2 * R)
                {
                    bool take = dy == 0 && i0 + t == R;          // the centre is always taken
                    if (!take)
                    {
                        const float z = vr_dot(np.x, np.y, np.z, pq[t].x - pp.x, pq[t].y - pp.y, pq[t].z - pp.z);
                        const float cn = vr_dot(np.x, np.y, np.z, nq[t].x, nq[t].y, nq[t].z);
                        // (the count of the image is 0 on an invalid pixel, but such a pixel's id differs from the centre's anyway)
                        take = in[t] && __float_as_int(pq[t].w) == id && mq[t].z > 0.0f && z * z <= P.zz && cn >= P.min_normal_dot;
                    }
                    if (take) { s1 = s1 + mq[t].x; s2 = s2 + mq[t].y; k = k + 1.0f; }
                }
        }
    }
    const float a1 = s1 / k, a2 = s2 / k;
    float vs = a2 - (a1 * a1);
    vs = vs > 0.0f ? vs : 0.0f;
    return vs / fr;
}

// The count in the moments image is 0 where the pixel has no variance - an invalid id, no samples -, so the common case, a pixel
// with a long enough history, is one 16-byte load and one store.  A wave none of whose lanes needs the spatial estimate branches
// over the window as a whole (the compiler guards the divergent `if` below with an execz branch).
__global__ __launch_bounds__(VR_BLOCK_X * VR_BLOCK_Y) void variance_kernel(const VarianceParams P)
{
    int x, y;
    if (!vr_pixel(P.width, P.height, x, y)) return;
    const size_t ip = (size_t)y * P.width + x;
    const float4 mp = P.mm[ip];
    float raw;
    if (!(mp.z > 0.0f)) raw = P.mark ? -1.0f : 0.0f;
    else
    {
        const float fr = mp.w > 0.0f ? mp.z / mp.w : 1.0f;
        if (fr >= P.min_frames)
        {
            float v = mp.y - (mp.x * mp.x);
            v = v > 0.0f ? v : 0.0f;
            raw = v / (fr - 1.0f);
        }
        else if (P.radius == 1) raw = vr_spatial<1>(P, x, y, fr);
        else if (P.radius == 2) raw = vr_spatial<2>(P, x, y, fr);
        else raw = vr_spatial<3>(P, x, y, fr);
    }
    P.raw[ip] = raw;
}

// g = (0.25, 0.5, 0.25) in both axes over the taps that are pixels with a variance: a marked pixel (-1) is no tap, and as a centre
// it gets 0.  A raw variance is never negative otherwise (it is >= 0 or NaN), so `< 0` tells the mark.
__global__ __launch_bounds__(VR_BLOCK_X * VR_BLOCK_Y) void variance_prefilter_kernel(const VariancePrefilterParams P)
{
    int x, y;
    if (!vr_pixel(P.width, P.height, x, y)) return;
    const size_t ip = (size_t)y * P.width + x;
    const float g[3] = { 0.25f, 0.5f, 0.25f };
    float rq[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; t++)
    {
        const int qx = x + (t % 3 - 1), qy = y + (t / 3 - 1);
        in[t] = qx >= 0 && qx < P.width && qy >= 0 && qy < P.height;
        rq[t] = P.raw[in[t] ? (size_t)qy * P.width + qx : ip];
    }
    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; t++)
        if (in[t] && !(rq[t] < 0.0f))
        {
            const float w = g[t / 3] * g[t % 3];
            sv = sv + (w * rq[t]); sw = sw + w;
        }
    // (the centre is tap 4: the nine loads go out together, and the one round trip decides everything)
    P.out[ip] = rq[4] < 0.0f ? 0.0f : sv / sw;
}

__global__ __launch_bounds__(VR_BLOCK_X * VR_BLOCK_Y) void temporal_mask_kernel(const float* __restrict__ count, const int32_t* __restrict__ triangle,
                                                                               const float* __restrict__ emission, int32_t* __restrict__ mask,
                                                                               const int width, const int height)
{
    int x, y;
    if (!vr_pixel(width, height, x, y)) return;
    const size_t i = (size_t)y * width + x;
    const bool valid = count[i] > 0.0f && triangle[i] >= 0 && emission[3 * i] == 0.0f && emission[3 * i + 1] == 0.0f && emission[3 * i + 2] == 0.0f;
    mask[i] = valid ? 0 : -1;
}

static dim3 vr_grid(int width, int height) { return dim3((width + VR_BLOCK_X - 1) / VR_BLOCK_X, (height + VR_BLOCK_Y - 1) / VR_BLOCK_Y); }
static const dim3 vr_block(VR_BLOCK_X, VR_BLOCK_Y);

void launch_variance_pack(const VariancePackParams& p, const VarianceImages& im, hipStream_t stream)
{
    hipLaunchKernelGGL(variance_pack_kernel, vr_grid(p.width, p.height), vr_block, 0, stream, p, im);
}

void launch_variance(const VarianceParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(variance_kernel, vr_grid(p.width, p.height), vr_block, 0, stream, p);
}

void launch_variance_prefilter(const VariancePrefilterParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(variance_prefilter_kernel, vr_grid(p.width, p.height), vr_block, 0, stream, p);
}

void launch_temporal_mask(const float* count, const int32_t* triangle, const float* emission, int32_t* mask, int width, int height, hipStream_t stream)
{
    hipLaunchKernelGGL(temporal_mask_kernel, vr_grid(width, height), vr_block, 0, stream, count, triangle, emission, mask, width, height);
}

}  // namespace ptk
