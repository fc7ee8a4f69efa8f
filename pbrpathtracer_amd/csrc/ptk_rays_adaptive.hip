// HIP kernels for gfx950 of adaptive ray queries and lightmap bakes (include/ptk.h ptk_trace_rays_adaptive,
// ptk_bake_lightmap_adaptive): rounds of `step` samples over the rays that have not met the noise target yet.  The trace is
// rays_keyed_kernel (ptk_rays.hip) as it is, over the round's COMPACTED rays; this file holds what stands around it:
//   * rays_gather_kernel       - the active list -> compacted origins, dirs, RNG pixels and source indices;
//   * rays_fold_moments_kernel - rays_fold_kernel for S1 and S2 of the source ray, and its sample count;
//   * rays_converge_kernel     - the rule of ptk_render_adaptive per active ray; bake_keep_kernel: a lightmap's 3x3 neighbourhood;
//   * rays_keep_count_kernel, the scan of ptk_bake.hip, rays_keep_scatter_kernel - the next active list, stable in ascending index.
// Compiled with -ffp-contract=off like ptk_rays.hip: S2 = S2 + v * v is a multiply and an add, and the test is float32 in the
// documented order - tests/rays_adaptive_rule.py recomputes both in numpy.
#include "ptk_device_fn.h"
#include "ptk_bake.h"
#include "ptk_rays_adaptive.h"

namespace ptk {

namespace {

#define PTK_RADAPT_BLOCK 256        // 4 waves; the compaction counts survivors per block of this many rays

// One thread per FLOAT of the compacted arrays, so that consecutive lanes write consecutive words; the first of a ray's three
// threads also writes its key and source index.
__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void rays_gather_kernel(const uint32_t* __restrict__ list, uint32_t count, const float* __restrict__ origins_in,
                                                                       const float* __restrict__ dirs_in, const uint32_t* __restrict__ keys_in, uint32_t key_base,
                                                                       float* __restrict__ origins, float* __restrict__ dirs, uint32_t* __restrict__ keys,
                                                                       uint32_t* __restrict__ src)
{
    const size_t e = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    if (e >= (size_t)count * 3) return;
    const size_t j = e / 3;
    const uint32_t a = (uint32_t)(e - j * 3);
    const uint32_t i = list ? list[j] : (uint32_t)j;
    origins[e] = origins_in[(size_t)i * 3 + a];
    dirs[e] = dirs_in[(size_t)i * 3 + a];
    if (a == 0)
    {
        keys[j] = keys_in ? keys_in[i] : key_base + i;
        src[j] = i;
    }
}

// rays_fold_kernel (ptk_rays.hip) with the second moment: one thread per compacted ray, eight loads in flight, S1 and S2 of the
// SOURCE ray read, folded strictly in sample order and written back.
__global__ __launch_bounds__(PTK_BLOCK) void rays_fold_moments_kernel(const float4* __restrict__ samples, const uint32_t* __restrict__ src, float* __restrict__ s1,
                                                                      float* __restrict__ s2, uint32_t* __restrict__ counts, int num_rays, int chunk,
                                                                      int num_chunks, uint32_t spp, uint32_t add_count)
{
    const size_t j = (size_t)blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (j >= (size_t)num_rays) return;
    const size_t i = src[j];
    float* o1 = s1 + i * 3;
    float* o2 = s2 + i * 3;
    v3 acc = V(o1[0], o1[1], o1[2]), sq = V(o2[0], o2[1], o2[2]);
    const float4* s = samples + (j >> 6) * (size_t)num_chunks * (size_t)chunk * 64 + (j & 63);
    uint32_t k = 0;
    for (; k + 8 <= spp; k += 8)
    {
        float4 v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = s[(size_t)(k + q) * 64];
#pragma unroll
        for (int q = 0; q < 8; q++)
        {
            acc = add(acc, V(v[q].x, v[q].y, v[q].z));
            const float p0 = v[q].x * v[q].x, p1 = v[q].y * v[q].y, p2 = v[q].z * v[q].z;
            sq = add(sq, V(p0, p1, p2));
        }
    }
    for (; k < spp; k++)
    {
        const float4 v = s[(size_t)k * 64];
        acc = add(acc, V(v.x, v.y, v.z));
        const float p0 = v.x * v.x, p1 = v.y * v.y, p2 = v.z * v.z;
        sq = add(sq, V(p0, p1, p2));
    }
    o1[0] = acc.x; o1[1] = acc.y; o1[2] = acc.z;
    o2[0] = sq.x; o2[1] = sq.y; o2[2] = sq.z;
    if (add_count) counts[i] += add_count;
}

// converge_kernel's test (ptk_adaptive.hip), per active ray
__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void rays_converge_kernel(const uint32_t* __restrict__ src, uint32_t count, const float* __restrict__ s1,
                                                                         const float* __restrict__ s2, const uint32_t* __restrict__ counts, float threshold,
                                                                         uint32_t* __restrict__ keep, uint8_t* __restrict__ need, const uint32_t* __restrict__ texel)
{
    const size_t j = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    if (j >= count) return;
    const size_t i = src[j];
    const float nf = (float)counts[i];
    float m[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        m[k] = s1[i * 3 + k] / nf;
        const float e2 = s2[i * 3 + k] / nf;
        const float mm = m[k] * m[k];
        const float x = e2 - mm;
        v[k] = x < 0.0f ? 0.0f : x;              // (NaN stays NaN)
    }
    const float err2 = ((v[0] + v[1]) + v[2]) / (3.0f * (nf - 1.0f));
    const float lum = ((m[0] + m[1]) + m[2]) / 3.0f;
    const float tol = threshold * (lum + 1.0f / 256.0f);
    const float tol2 = tol * tol;
    const bool open = !(err2 < tol2);            // strict: threshold 0 and NaN never converge
    if (need) need[texel[i]] = open ? 1 : 0;
    else keep[j] = open ? 1u : 0u;
}

// An active texel goes on when some active, not-done texel lies in its 3x3 neighbourhood clipped to the map.  (need is 1 only
// for such texels: a texel that left the active set did so with need 0 and is never written again.)
__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void bake_keep_kernel(const uint32_t* __restrict__ src, uint32_t count, const uint32_t* __restrict__ texel,
                                                                     const uint8_t* __restrict__ need, int width, int height, uint32_t* __restrict__ keep)
{
    const size_t j = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint32_t t = texel[src[j]];
    const int y = (int)(t / (uint32_t)width), x = (int)(t - (uint32_t)y * (uint32_t)width);
    uint32_t any = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++)
        {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || yy < 0 || xx >= width || yy >= height) continue;
            any |= need[(size_t)yy * width + xx];
        }
    keep[j] = any;
}

// survivors of each block of 256 rays (bake_count_kernel's shape)
__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void rays_keep_count_kernel(const uint32_t* __restrict__ keep, uint32_t count, uint32_t* __restrict__ block_counts)
{
    __shared__ uint32_t wave_n[PTK_RADAPT_BLOCK / 64];
    const size_t j = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    const bool k = j < count && keep[j] != 0u;
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// A survivor's slot is the number of survivors before it: those of the blocks before (block_counts, scanned), of the waves before
// it in the block and of the lanes before it in the wave - ascending index whatever order the waves run in (bake_rays_kernel).
__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void rays_keep_scatter_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ keep, uint32_t count,
                                                                             const uint32_t* __restrict__ block_counts, uint32_t* __restrict__ list)
{
    __shared__ uint32_t wave_n[PTK_RADAPT_BLOCK / 64];
    const size_t j = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool k = j < count && keep[j] != 0u;
    const unsigned long long m = __ballot(k);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!k) return;
    uint32_t before = block_counts[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) before += wave_n[w];
    list[before] = src[j];
}

__global__ __launch_bounds__(PTK_RADAPT_BLOCK) void bake_scatter_counts_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ texel, uint32_t count,
                                                                               uint32_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * PTK_RADAPT_BLOCK + threadIdx.x;
    if (i >= count) return;
    out[texel[i]] = counts[i];
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + PTK_RADAPT_BLOCK - 1) / PTK_RADAPT_BLOCK); }

}  // namespace

void launch_rays_gather(const uint32_t* list, uint32_t count, const float* origins_in, const float* dirs_in, const uint32_t* keys_in, uint32_t key_base,
                        float* origins, float* dirs, uint32_t* keys, uint32_t* src, hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(rays_gather_kernel, dim3(blocks_of((size_t)count * 3)), dim3(PTK_RADAPT_BLOCK), 0, stream, list, count, origins_in, dirs_in, keys_in,
                       key_base, origins, dirs, keys, src);
}

void launch_rays_fold_moments(const float4* samples, const uint32_t* src, float* s1, float* s2, uint32_t* counts, int num_rays, int chunk,
                              int num_chunks, uint32_t spp, uint32_t add_count, hipStream_t stream)
{
    if (num_rays <= 0) return;
    hipLaunchKernelGGL(rays_fold_moments_kernel, dim3((num_rays + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, samples, src, s1, s2, counts,
                       num_rays, chunk, num_chunks, spp, add_count);
}

void launch_rays_converge(const uint32_t* src, uint32_t count, const float* s1, const float* s2, const uint32_t* counts, float threshold,
                          uint32_t* keep, uint8_t* need, const uint32_t* texel, hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(rays_converge_kernel, dim3(blocks_of(count)), dim3(PTK_RADAPT_BLOCK), 0, stream, src, count, s1, s2, counts, threshold, keep, need,
                       texel);
}

void launch_bake_keep(const uint32_t* src, uint32_t count, const uint32_t* texel, const uint8_t* need, int width, int height, uint32_t* keep,
                      hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(bake_keep_kernel, dim3(blocks_of(count)), dim3(PTK_RADAPT_BLOCK), 0, stream, src, count, texel, need, width, height, keep);
}

void launch_rays_compact(const uint32_t* src, const uint32_t* keep, uint32_t count, uint32_t* block_counts, uint32_t* total, uint32_t* list,
                         hipStream_t stream)
{
    if (count == 0) return;
    const unsigned blocks = blocks_of(count);
    hipLaunchKernelGGL(rays_keep_count_kernel, dim3(blocks), dim3(PTK_RADAPT_BLOCK), 0, stream, keep, count, block_counts);
    launch_bake_scan(block_counts, blocks, total, stream);
    hipLaunchKernelGGL(rays_keep_scatter_kernel, dim3(blocks), dim3(PTK_RADAPT_BLOCK), 0, stream, src, keep, count, block_counts, list);
}

void launch_bake_scatter_counts(const uint32_t* counts, const uint32_t* texel, uint32_t count, uint32_t* out, hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(bake_scatter_counts_kernel, dim3(blocks_of(count)), dim3(PTK_RADAPT_BLOCK), 0, stream, counts, texel, count, out);
}

}  // namespace ptk
