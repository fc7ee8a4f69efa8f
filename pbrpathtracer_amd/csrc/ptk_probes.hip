// HIP kernels for gfx950 of irradiance probe baking (include/ptk.h ptk_bake_probes, ptk_probes_irradiance): the rays of a block of
// probes for rays_kernel (ptk_rays.hip), the projection of the traced radiance table onto nine real spherical harmonics per probe
// and channel, and the lookup of Lambertian irradiance in a probe grid; and of probe visibility (ptk_bake_probe_visibility,
// ptk_probes_irradiance_visible): the projection of a probe's depth table onto the moments of its octahedral texels and the lookup
// that weights the corner probes by them.  Compiled with -ffp-contract=off: every product, sum, difference and quotient is rounded
// on its own, the float32 arithmetic the header states and tests/probe_cases.py, tests/probe_vis_cases.py restate; sqrtf and / are
// the correctly rounded IEEE operations.
#include <algorithm>

#include "ptk_probes.h"

namespace ptk {

#define PTK_PROBES_BLOCK 256

namespace {

// Yk(x, y, z), k = 0..8: the header's expressions, the one text behind the basis table and the sampler
__device__ __forceinline__ void probe_basis(float x, float y, float z, float Y[PTK_PROBE_COEFS])
{
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * (x * y);
    Y[5] = 1.092548f * (y * z);
    Y[6] = 0.315392f * ((3.0f * (z * z)) - 1.0f);
    Y[7] = 1.092548f * (x * z);
    Y[8] = 0.546274f * ((x * x) - (y * y));
}

__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_basis_kernel(const float* __restrict__ dirs, int num_dirs, float* __restrict__ basis)
{
    const int j = blockIdx.x * PTK_PROBES_BLOCK + threadIdx.x;
    if (j >= num_dirs) return;
    float Y[PTK_PROBE_COEFS];
    probe_basis(dirs[j * 3], dirs[j * 3 + 1], dirs[j * 3 + 2], Y);
#pragma unroll
    for (int k = 0; k < PTK_PROBE_COEFS; k++) basis[j * PTK_PROBE_COEFS + k] = Y[k];
}

// One thread per ray of a block of whole probes: ray r = p * num_dirs + j starts at positions[p] along dirs[j], as given.
__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_rays_kernel(const float* __restrict__ positions, const float* __restrict__ dirs, uint32_t num_rays,
                                                                      uint32_t num_dirs, float* __restrict__ origins, float* __restrict__ ray_dirs)
{
    const uint32_t r = blockIdx.x * PTK_PROBES_BLOCK + threadIdx.x;         // num_rays < 2^31
    if (r >= num_rays) return;
    const uint32_t p = r / num_dirs, j = r - p * num_dirs;
    const float* o = positions + (size_t)p * 3, * d = dirs + (size_t)j * 3;
    float* wo = origins + (size_t)r * 3, * wd = ray_dirs + (size_t)r * 3;
    wo[0] = o[0]; wo[1] = o[1]; wo[2] = o[2];
    wd[0] = d[0]; wd[1] = d[1]; wd[2] = d[2];
}

// One thread per (probe, coefficient) carrying the three channels: the sum over the directions is a dependent chain in ascending
// j by definition, so a thread keeps eight rows of the table in flight (rays_fold_kernel's loop) and adds them in order.  The
// nine threads of a probe read the same row of the table.
__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_project_kernel(const float* __restrict__ radiance, const float* __restrict__ basis, uint32_t num_probes,
                                                                         uint32_t num_dirs, float weight, float* __restrict__ coefs)
{
    const size_t i = (size_t)blockIdx.x * PTK_PROBES_BLOCK + threadIdx.x;
    if (i >= (size_t)num_probes * PTK_PROBE_COEFS) return;
    const size_t p = i / PTK_PROBE_COEFS;
    const uint32_t k = (uint32_t)(i - p * PTK_PROBE_COEFS);
    const float* s = radiance + p * num_dirs * 3;
    const float* y = basis + k;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    uint32_t j = 0;
    for (; j + 8 <= num_dirs; j += 8)
    {
        float v[8][3], w[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
        {
            const float* q = s + (size_t)(j + u) * 3;
            v[u][0] = q[0]; v[u][1] = q[1]; v[u][2] = q[2];
            w[u] = y[(size_t)(j + u) * PTK_PROBE_COEFS];
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
        {
            a0 = a0 + (v[u][0] * w[u]); a1 = a1 + (v[u][1] * w[u]); a2 = a2 + (v[u][2] * w[u]);
        }
    }
    for (; j < num_dirs; j++)
    {
        const float* q = s + (size_t)j * 3;
        const float w = y[(size_t)j * PTK_PROBE_COEFS];
        a0 = a0 + (q[0] * w); a1 = a1 + (q[1] * w); a2 = a2 + (q[2] * w);
    }
    float* c = coefs + i * 3;
    c[0] = a0 * weight; c[1] = a1 * weight; c[2] = a2 * weight;
}

__device__ __forceinline__ float probe_lerp(float a, float b, float f) { return a + ((b - a) * f); }

// the header's per-axis rule: the cell (i0, i1) and the fraction f of coordinate q on an axis of n probes
__device__ __forceinline__ void probe_cell(float q, float origin, float spacing, int n, int& i0, int& i1, float& f)
{
    float g = (q - origin) / spacing;
    g = g > 0.0f ? g : 0.0f;                    // (NaN: 0)
    const float top = (float)(n - 1);
    g = g < top ? g : top;
    i0 = (int)g;
    if (i0 > n - 2) i0 = max(n - 2, 0);
    f = g - (float)i0;
    i1 = min(i0 + 1, n - 1);
}

// One thread per query: the eight corner probes' 27 coefficients each, interpolated along x, then y, then z, and evaluated at the
// normal with the Lambertian band factors.
__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_irradiance_kernel(const ProbeGrid G, const float* __restrict__ coefs, int num_points,
                                                                            const float* __restrict__ points, const float* __restrict__ normals,
                                                                            float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * PTK_PROBES_BLOCK + threadIdx.x;
    if (i >= (size_t)num_points) return;
    int x0, x1, y0, y1, z0, z1;
    float fx, fy, fz;
    probe_cell(points[i * 3], G.origin[0], G.spacing[0], G.dims[0], x0, x1, fx);
    probe_cell(points[i * 3 + 1], G.origin[1], G.spacing[1], G.dims[1], y0, y1, fy);
    probe_cell(points[i * 3 + 2], G.origin[2], G.spacing[2], G.dims[2], z0, z1, fz);
    const size_t nx = (size_t)G.dims[0], ny = (size_t)G.dims[1], stride = PTK_PROBE_COEFS * 3;
    const float* r00 = coefs + ((size_t)z0 * ny + y0) * nx * stride, * r10 = coefs + ((size_t)z0 * ny + y1) * nx * stride;
    const float* r01 = coefs + ((size_t)z1 * ny + y0) * nx * stride, * r11 = coefs + ((size_t)z1 * ny + y1) * nx * stride;
    const size_t o0 = (size_t)x0 * stride, o1 = (size_t)x1 * stride;
    float Y[PTK_PROBE_COEFS];
    probe_basis(normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2], Y);
    float E[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int k = 0; k < PTK_PROBE_COEFS; k++)
    {
        const float A = k == 0 ? 3.141593f : (k < 4 ? 2.094395f : 0.785398f);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
        {
            const int e = k * 3 + ch;
            const float c00 = probe_lerp(r00[o0 + e], r00[o1 + e], fx), c10 = probe_lerp(r10[o0 + e], r10[o1 + e], fx);
            const float c01 = probe_lerp(r01[o0 + e], r01[o1 + e], fx), c11 = probe_lerp(r11[o0 + e], r11[o1 + e], fx);
            const float c0 = probe_lerp(c00, c10, fy), c1 = probe_lerp(c01, c11, fy);
            const float c = probe_lerp(c0, c1, fz);
            const float t = (A * c) * Y[k];
            E[ch] = k == 0 ? t : E[ch] + t;
        }
    }
    out[i * 3] = E[0]; out[i * 3 + 1] = E[1]; out[i * 3 + 2] = E[2];
}

// ---- probe visibility -----------------------------------------------------------------------------------------------------------
#define PTK_PVIS_CHUNK 64           // directions staged in LDS per round
#define PTK_PVIS_GROUP 64           // probes of a workgroup at most (res 1 and 2: one wave's worth of texels each way)

__device__ __forceinline__ float probe_sgn(float s) { return s >= 0.0f ? 1.0f : -1.0f; }        // (NaN: -1)

// the header's unit direction of octahedral texel (a, b) of res x res
__device__ __forceinline__ void probe_texel_dir(int a, int b, int res, float& ex, float& ey, float& ez)
{
    const float u = ((((float)a + 0.5f) * 2.0f) / (float)res) - 1.0f;
    const float v = ((((float)b + 0.5f) * 2.0f) / (float)res) - 1.0f;
    const float z = (1.0f - fabsf(u)) - fabsf(v);
    float x = u, y = v;
    if (z < 0.0f) { x = (1.0f - fabsf(v)) * probe_sgn(u); y = (1.0f - fabsf(u)) * probe_sgn(v); }
    const float len = sqrtf(((x * x) + (y * y)) + (z * z));                     // >= 1 / sqrt(3)
    ex = x / len; ey = y / len; ez = z / len;
}

// One thread per (probe, texel), `group` = min(PTK_PVIS_GROUP, 256 / res^2) whole probes per workgroup so that small texel counts
// still fill the waves.  The sums over the directions are dependent chains in ascending j by definition; the directions (shared
// by every probe) and the group's clamped depths go through LDS in rounds of PTK_PVIS_CHUNK: all lanes of a probe read the same
// j - a broadcast -, and the depth rows are PTK_PVIS_CHUNK + 1 dwords apart, so the probes of a wave sit on different banks.
__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_moments_kernel(const float* __restrict__ depth, const float* __restrict__ dirs, uint32_t num_probes,
                                                                         uint32_t num_dirs, int res, uint32_t group, float max_dist,
                                                                         float* __restrict__ moments)
{
    __shared__ float4 s_dir[PTK_PVIS_CHUNK];
    __shared__ float s_depth[PTK_PVIS_GROUP * (PTK_PVIS_CHUNK + 1)];
    const uint32_t tid = threadIdx.x, texels = (uint32_t)(res * res);
    const uint32_t lp = tid / texels, tau = tid - lp * texels;
    const uint32_t p0 = blockIdx.x * group;                                     // < num_probes < 2^31
    const uint32_t np = min(group, num_probes - p0);
    const bool own = lp < np;
    float ex, ey, ez;
    probe_texel_dir((int)(tau % (uint32_t)res), (int)(tau / (uint32_t)res), res, ex, ey, ez);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (uint32_t j0 = 0; j0 < num_dirs; j0 += PTK_PVIS_CHUNK)
    {
        const uint32_t nj = min((uint32_t)PTK_PVIS_CHUNK, num_dirs - j0);
        __syncthreads();                                                        // the round before has been read
        if (tid < nj)
        {
            const float* d = dirs + (size_t)(j0 + tid) * 3;
            s_dir[tid] = make_float4(d[0], d[1], d[2], 0.0f);
        }
        for (uint32_t e = tid; e < np * PTK_PVIS_CHUNK; e += PTK_PROBES_BLOCK)
        {
            const uint32_t q = e / PTK_PVIS_CHUNK, j = e % PTK_PVIS_CHUNK;
            if (j < nj)
            {
                const float t = depth[(size_t)(p0 + q) * num_dirs + j0 + j];
                s_depth[q * (PTK_PVIS_CHUNK + 1) + j] = t < max_dist ? t : max_dist;        // (NaN: max_dist)
            }
        }
        __syncthreads();
        if (own)
        {
            const float* row = s_depth + lp * (PTK_PVIS_CHUNK + 1);
#pragma unroll 4
            for (uint32_t j = 0; j < nj; j++)
            {
                const float4 d = s_dir[j];
                const float R = row[j];
                float c = ((ex * d.x) + (ey * d.y)) + (ez * d.z);
                c = c > 0.0f ? c : 0.0f;                                        // (NaN: 0)
                c = c * c; c = c * c; c = c * c; c = c * c; c = c * c;          // cos^32
                sw = sw + c;
                s1 = s1 + (c * R);
                s2 = s2 + (c * (R * R));
            }
        }
    }
    if (!own) return;
    float* m = moments + ((size_t)(p0 + lp) * texels + tau) * 2;
    const bool any = sw > 0.0f;
    m[0] = any ? s1 / sw : max_dist;
    m[1] = any ? s2 / sw : max_dist * max_dist;
}

// the header's texel coordinate of an octahedral coordinate p in [-1, 1]
__device__ __forceinline__ int probe_texel_coord(float p, int res)
{
    float g = ((p * 0.5f) + 0.5f) * (float)res;
    g = g > 0.0f ? g : 0.0f;                    // (NaN: 0)
    const float top = (float)(res - 1);
    g = g < top ? g : top;
    return (int)g;
}

// One thread per query: the eight corner probes in the order z, y, x, each with its own irradiance at the normal, its trilinear
// factor, back-face term and Chebyshev visibility from the moment texel that faces the (biased) point.
__global__ __launch_bounds__(PTK_PROBES_BLOCK) void probe_irradiance_visible_kernel(const ProbeGrid G, const float* __restrict__ coefs, int res,
                                                                                    const float* __restrict__ moments, float normal_bias, int num_points,
                                                                                    const float* __restrict__ points, const float* __restrict__ normals,
                                                                                    float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * PTK_PROBES_BLOCK + threadIdx.x;
    if (i >= (size_t)num_points) return;
    const float q[3] = { points[i * 3], points[i * 3 + 1], points[i * 3 + 2] };
    const float n[3] = { normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2] };
    int i0[3], i1[3];
    float f[3], bq[3];
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        probe_cell(q[a], G.origin[a], G.spacing[a], G.dims[a], i0[a], i1[a], f[a]);
        bq[a] = q[a] + (n[a] * normal_bias);
    }
    float Y[PTK_PROBE_COEFS];
    probe_basis(n[0], n[1], n[2], Y);
    const size_t nx = (size_t)G.dims[0], ny = (size_t)G.dims[1], texels = (size_t)(res * res);
    float num[3] = { 0.0f, 0.0f, 0.0f }, den = 0.0f;
#pragma unroll
    for (int corner = 0; corner < 8; corner++)
    {
        const int cx = corner & 1, cy = (corner >> 1) & 1, cz = corner >> 2;
        const int ix = cx ? i1[0] : i0[0], iy = cy ? i1[1] : i0[1], iz = cz ? i1[2] : i0[2];
        const float tx = cx ? f[0] : (1.0f - f[0]), ty = cy ? f[1] : (1.0f - f[1]), tz = cz ? f[2] : (1.0f - f[2]);
        const float tri = (tx * ty) * tz;
        const float vx = bq[0] - (G.origin[0] + ((float)ix * G.spacing[0]));
        const float vy = bq[1] - (G.origin[1] + ((float)iy * G.spacing[1]));
        const float vz = bq[2] - (G.origin[2] + ((float)iz * G.spacing[2]));
        const float dist = sqrtf(((vx * vx) + (vy * vy)) + (vz * vz));
        const size_t probe = ((size_t)iz * ny + (size_t)iy) * nx + (size_t)ix;
        float back = 1.0f, vis = 1.0f;
        if (dist > 0.0f)                                                        // (zero and NaN: both terms stay 1)
        {
            const float cosn = (((vx * n[0]) + (vy * n[1])) + (vz * n[2])) / dist;
            const float h = (1.0f - cosn) * 0.5f;
            back = (h * h) + 0.2f;
            const float s = (fabsf(vx) + fabsf(vy)) + fabsf(vz);
            if (s > 0.0f)
            {
                float px = vx / s, py = vy / s;
                if (vz < 0.0f)
                {
                    const float ox = px, oy = py;
                    px = (1.0f - fabsf(oy)) * probe_sgn(ox);
                    py = (1.0f - fabsf(ox)) * probe_sgn(oy);
                }
                const int a = probe_texel_coord(px, res), b = probe_texel_coord(py, res);
                const float* m = moments + (probe * texels + (size_t)(b * res + a)) * 2;
                const float mean = m[0], mean2 = m[1];
                if (dist > mean)
                {
                    float var = mean2 - (mean * mean);
                    var = var > 0.0f ? var : 0.0f;                              // (NaN: 0)
                    const float dd = dist - mean;
                    const float dn = var + (dd * dd);
                    const float ch = dn > 0.0f ? var / dn : 0.0f;
                    vis = (ch * ch) * ch;
                }
            }
        }
        float w = back * vis;
        w = w > 1e-6f ? w : 1e-6f;                                              // (NaN: 1e-6)
        const float W = w * tri;
        const float* c = coefs + probe * (PTK_PROBE_COEFS * 3);
        float E[3];
#pragma unroll
        for (int k = 0; k < PTK_PROBE_COEFS; k++)
        {
            const float A = k == 0 ? 3.141593f : (k < 4 ? 2.094395f : 0.785398f);
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
            {
                const float t = (A * c[k * 3 + ch]) * Y[k];
                E[ch] = k == 0 ? t : E[ch] + t;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) num[ch] = num[ch] + (W * E[ch]);
        den = den + W;
    }
    out[i * 3] = num[0] / den; out[i * 3 + 1] = num[1] / den; out[i * 3 + 2] = num[2] / den;
}

inline unsigned probe_blocks(size_t n) { return (unsigned)((n + PTK_PROBES_BLOCK - 1) / PTK_PROBES_BLOCK); }

}  // namespace

void launch_probe_basis(const float* dirs, int num_dirs, float* basis, hipStream_t stream)
{
    if (num_dirs <= 0) return;
    hipLaunchKernelGGL(probe_basis_kernel, dim3(probe_blocks((size_t)num_dirs)), dim3(PTK_PROBES_BLOCK), 0, stream, dirs, num_dirs, basis);
}

void launch_probe_rays(const float* positions, const float* dirs, int num_probes, int num_dirs, float* origins, float* ray_dirs, hipStream_t stream)
{
    const size_t n = (size_t)num_probes * (size_t)num_dirs;
    if (n == 0) return;
    hipLaunchKernelGGL(probe_rays_kernel, dim3(probe_blocks(n)), dim3(PTK_PROBES_BLOCK), 0, stream, positions, dirs, (uint32_t)n, (uint32_t)num_dirs,
                       origins, ray_dirs);
}

void launch_probe_project(const float* radiance, const float* basis, int num_probes, int num_dirs, float weight, float* coefs, hipStream_t stream)
{
    if (num_probes <= 0) return;
    hipLaunchKernelGGL(probe_project_kernel, dim3(probe_blocks((size_t)num_probes * PTK_PROBE_COEFS)), dim3(PTK_PROBES_BLOCK), 0, stream, radiance, basis,
                       (uint32_t)num_probes, (uint32_t)num_dirs, weight, coefs);
}

void launch_probe_irradiance(const ProbeGrid& grid, const float* coefs, int num_points, const float* points, const float* normals, float* out,
                             hipStream_t stream)
{
    if (num_points <= 0) return;
    hipLaunchKernelGGL(probe_irradiance_kernel, dim3(probe_blocks((size_t)num_points)), dim3(PTK_PROBES_BLOCK), 0, stream, grid, coefs, num_points, points,
                       normals, out);
}

void launch_probe_moments(const float* depth, const float* dirs, int num_probes, int num_dirs, int res, float max_dist, float* moments,
                          hipStream_t stream)
{
    if (num_probes <= 0) return;
    const uint32_t group = std::min<uint32_t>(PTK_PVIS_GROUP, PTK_PROBES_BLOCK / (uint32_t)(res * res));         // res <= 16: at least 1
    hipLaunchKernelGGL(probe_moments_kernel, dim3(((uint32_t)num_probes + group - 1) / group), dim3(PTK_PROBES_BLOCK), 0, stream, depth, dirs,
                       (uint32_t)num_probes, (uint32_t)num_dirs, res, group, max_dist, moments);
}

void launch_probe_irradiance_visible(const ProbeGrid& grid, const float* coefs, int res, const float* moments, float normal_bias, int num_points,
                                     const float* points, const float* normals, float* out, hipStream_t stream)
{
    if (num_points <= 0) return;
    hipLaunchKernelGGL(probe_irradiance_visible_kernel, dim3(probe_blocks((size_t)num_points)), dim3(PTK_PROBES_BLOCK), 0, stream, grid, coefs, res,
                       moments, normal_bias, num_points, points, normals, out);
}

}  // namespace ptk
