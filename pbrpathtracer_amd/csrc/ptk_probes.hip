// HIP kernels for gfx950 of irradiance probe baking (include/ptk.h ptk_bake_probes, ptk_probes_irradiance): the rays of a block of
// probes for rays_kernel (ptk_rays.hip), the projection of the traced radiance table onto nine real spherical harmonics per probe
// and channel, and the lookup of Lambertian irradiance in a probe grid.  Compiled with -ffp-contract=off: every product, sum,
// difference and quotient is rounded on its own, the float32 arithmetic the header states and tests/probe_cases.py restates.
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

}  // namespace ptk
