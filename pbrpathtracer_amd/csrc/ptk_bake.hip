// HIP kernels for gfx950 of lightmap baking (include/ptk.h ptk_bake_lightmap): which triangle owns each texel of a uv chart
// layout, the surface point and the ray of every owned texel - compacted in ascending texel index for rays_kernel (ptk_rays.hip) -,
// the scatter of the traced sums back into the image, and the chart padding.  Compiled with -ffp-contract=off: every product,
// difference and quotient is rounded on its own, the float32 arithmetic the header states and tests/bake_cases.py restates.
#include "ptk_bake.h"

namespace ptk {

#define PTK_BAKE_BLOCK 256          // texel kernels: 4 waves; bake_cover_kernel: 4 triangles

namespace {

struct Chart { float ax, ay, bx, by, cx, cy; };

// triangle k's corners in texel space: uv * (float)W, uv * (float)H
__device__ __forceinline__ Chart load_chart(const BakeParams& p, int k)
{
    float u[6];
    if (p.uvs)
    {
        const float* q = p.uvs + (size_t)k * 6;
#pragma unroll
        for (int i = 0; i < 6; i++) u[i] = q[i];
    }
    else
    {
        const float4 s1 = p.shade[(size_t)k * SHADE_F4 + 1], s2 = p.shade[(size_t)k * SHADE_F4 + 2];
        u[0] = s1.x; u[1] = s1.y; u[2] = s1.z; u[3] = s1.w; u[4] = s2.x; u[5] = s2.y;
    }
    const float W = (float)p.width, H = (float)p.height;
    Chart c;
    c.ax = u[0] * W; c.ay = u[1] * H; c.bx = u[2] * W; c.by = u[3] * H; c.cx = u[4] * W; c.cy = u[5] * H;
    return c;
}

// The coverage rule of the header for the texel centre (px, py); area, w2, w3 are what the surface point is made of.
__device__ __forceinline__ bool chart_covers(const Chart& c, float px, float py, float& area, float& w2, float& w3)
{
    area = (c.bx - c.ax) * (c.cy - c.ay) - (c.by - c.ay) * (c.cx - c.ax);
    const float w1 = (c.cx - c.bx) * (py - c.by) - (c.cy - c.by) * (px - c.bx);
    w2 = (px - c.ax) * (c.cy - c.ay) - (py - c.ay) * (c.cx - c.ax);
    w3 = (c.bx - c.ax) * (py - c.ay) - (c.by - c.ay) * (px - c.ax);
    if (!(fabsf(area) < __builtin_inff()) || area == 0.0f) return false;        // NaN, infinite or degenerate
    // (a NaN edge function fails every comparison)
    return area > 0.0f ? (w1 >= 0.0f) & (w2 >= 0.0f) & (w3 >= 0.0f) : (w1 <= 0.0f) & (w2 <= 0.0f) & (w3 <= 0.0f);
}

// One wave per triangle: the lanes stride over the triangle's texel box - one texel wider on every side than floor / ceil of its
// corners, clipped to the map - and atomicMin the triangle index into the texels whose centre the rule says it covers.
__global__ __launch_bounds__(PTK_BAKE_BLOCK) void bake_cover_kernel(const BakeParams p)
{
    const int k = blockIdx.x * (PTK_BAKE_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= p.num_tris) return;
    const Chart c = load_chart(p, k);
    const float lo_x = fminf(c.ax, fminf(c.bx, c.cx)), hi_x = fmaxf(c.ax, fmaxf(c.bx, c.cx));
    const float lo_y = fminf(c.ay, fminf(c.by, c.cy)), hi_y = fmaxf(c.ay, fmaxf(c.by, c.cy));
    // a corner that is NaN or infinite makes the area NaN or infinite: nothing is covered (fminf / fmaxf would skip a NaN)
    const float inf = __builtin_inff();
    if (!((fabsf(c.ax) < inf) && (fabsf(c.ay) < inf) && (fabsf(c.bx) < inf) && (fabsf(c.by) < inf) && (fabsf(c.cx) < inf) && (fabsf(c.cy) < inf))) return;
    const float W = (float)p.width, H = (float)p.height;
    if (hi_x < -1.0f || hi_y < -1.0f || lo_x > W + 1.0f || lo_y > H + 1.0f) return;
    // clamped in float before the conversion: the corners may lie far outside the range of an int
    const int x0 = max(0, (int)floorf(fmaxf(lo_x, -1.0f)) - 1), x1 = min(p.width - 1, (int)ceilf(fminf(hi_x, W + 1.0f)) + 1);
    const int y0 = max(0, (int)floorf(fmaxf(lo_y, -1.0f)) - 1), y1 = min(p.height - 1, (int)ceilf(fminf(hi_y, H + 1.0f)) + 1);
    if (x1 < x0 || y1 < y0) return;
    const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);         // <= 16384^2 = 2^28
    for (int i = lane; i < n; i += 64)
    {
        const int yy = i / bw, x = x0 + (i - yy * bw), y = y0 + yy;
        float area, w2, w3;
        if (chart_covers(c, (float)x + 0.5f, (float)y + 0.5f, area, w2, w3)) atomicMin(&p.plane[(size_t)y * p.width + x], k);
    }
}

// covered texels of each block of 256 texels
__global__ __launch_bounds__(PTK_BAKE_BLOCK) void bake_count_kernel(const int* __restrict__ plane, size_t texels, uint32_t* __restrict__ block_counts)
{
    __shared__ uint32_t wave_n[PTK_BAKE_BLOCK / 64];
    const size_t t = (size_t)blockIdx.x * PTK_BAKE_BLOCK + threadIdx.x;
    const bool covered = t < texels && plane[t] != PTK_BAKE_UNOWNED;
    const unsigned long long m = __ballot(covered);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// counts[0 .. n) <- their exclusive prefix sums, *total <- their sum.  One workgroup: thread i sums a run of consecutive counts,
// the runs' sums are scanned in LDS, then every thread rewrites its run.  (n <= 2^20 blocks of 256 texels: 1024 counts per thread.)
#define PTK_BAKE_SCAN 1024
__global__ __launch_bounds__(PTK_BAKE_SCAN) void bake_scan_kernel(uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ total)
{
    __shared__ uint32_t part[PTK_BAKE_SCAN];
    const uint32_t run = (n + PTK_BAKE_SCAN - 1) / PTK_BAKE_SCAN, i0 = min(n, threadIdx.x * run), i1 = min(n, i0 + run);
    uint32_t s = 0;
    for (uint32_t i = i0; i < i1; i++) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < PTK_BAKE_SCAN; d <<= 1)
    {
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t acc = part[threadIdx.x] - s;       // the runs before this one
    for (uint32_t i = i0; i < i1; i++) { const uint32_t v = counts[i]; counts[i] = acc; acc += v; }
    if (threadIdx.x == PTK_BAKE_SCAN - 1) *total = part[PTK_BAKE_SCAN - 1];
}

// One thread per texel: the owner's edge functions once more - the same expressions as in bake_cover_kernel, hence the same bits -,
// the surface point and the ray.  A covered texel's slot in the compacted arrays is the number of covered texels before it: those
// of the blocks before (block_counts, scanned), of the waves before it in the block and of the lanes before it in the wave, so
// the arrays are in ascending texel index whatever order the waves run in.
__global__ __launch_bounds__(PTK_BAKE_BLOCK) void bake_rays_kernel(const BakeParams p)
{
    __shared__ uint32_t wave_n[PTK_BAKE_BLOCK / 64];
    const size_t texels = (size_t)p.width * p.height, t = (size_t)blockIdx.x * PTK_BAKE_BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = t < texels ? p.plane[t] : PTK_BAKE_UNOWNED;
    const bool covered = k != PTK_BAKE_UNOWNED;
    const unsigned long long m = __ballot(covered);
    if (p.origins)
    {
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
        __syncthreads();
    }
    if (t >= texels) return;
    float b2 = 0.0f, b3 = 0.0f;
    float P[3] = { 0.0f, 0.0f, 0.0f }, n[3] = { 0.0f, 0.0f, 0.0f };
    if (covered)
    {
        const int y = (int)(t / (size_t)p.width), x = (int)(t - (size_t)y * p.width);
        const Chart c = load_chart(p, k);
        float area, w2, w3;
        (void)chart_covers(c, (float)x + 0.5f, (float)y + 0.5f, area, w2, w3);
        b2 = w2 / area; b3 = w3 / area;
        const float b1 = (1.0f - b2) - b3;
        const float* v = p.verts + (size_t)k * 9;
        const float4 s0 = p.shade[(size_t)k * SHADE_F4];
        n[0] = s0.x; n[1] = s0.y; n[2] = s0.z;
#pragma unroll
        for (int a = 0; a < 3; a++)
        {
            P[a] = ((v[a] * b1) + (v[3 + a] * b2)) + (v[6 + a] * b3);
            if (p.back) n[a] = -n[a];
        }
    }
    if (p.owner) p.owner[t] = covered ? k : -1;
    if (p.bary) { p.bary[t * 2] = b2; p.bary[t * 2 + 1] = b3; }
    if (p.pos) { p.pos[t * 3] = P[0]; p.pos[t * 3 + 1] = P[1]; p.pos[t * 3 + 2] = P[2]; }
    if (!p.origins || !covered) return;
    uint32_t before = p.block_counts[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) before += wave_n[w];
    const size_t i = before;
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        p.origins[i * 3 + a] = P[a] + n[a] * p.offset;
        p.dirs[i * 3 + a] = -n[a];
        if (p.out) p.sums[i * 3 + a] = p.out[t * 3 + a];
    }
    p.keys[i] = p.key_base + (uint32_t)t;
    p.texel[i] = (uint32_t)t;
}

__global__ __launch_bounds__(PTK_BAKE_BLOCK) void bake_scatter_kernel(const float* __restrict__ sums, const uint32_t* __restrict__ texel, uint32_t count,
                                                                      float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * PTK_BAKE_BLOCK + threadIdx.x;
    if (i >= count) return;
    const size_t t = texel[i];
    out[t * 3] = sums[i * 3]; out[t * 3 + 1] = sums[i * 3 + 1]; out[t * 3 + 2] = sums[i * 3 + 2];
}

// One dilation pass, out of place: an uncovered texel (owner -1) with a covered or filled 8-neighbour becomes the mean of those
// neighbours - summed in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, divided by their number - and gets owner -2.
__global__ __launch_bounds__(PTK_BAKE_BLOCK) void dilate_kernel(const float* __restrict__ src, const int32_t* __restrict__ src_owner, float* __restrict__ dst,
                                                                int32_t* __restrict__ dst_owner, int width, int height)
{
    const size_t t = (size_t)blockIdx.x * PTK_BAKE_BLOCK + threadIdx.x;
    if (t >= (size_t)width * height) return;
    int32_t o = src_owner[t];
    float r = src[t * 3], g = src[t * 3 + 1], b = src[t * 3 + 2];
    if (o == -1)
    {
        const int y = (int)(t / (size_t)width), x = (int)(t - (size_t)y * width);
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        int cnt = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++)
            {
                const int xx = x + dx, yy = y + dy;
                if (xx < 0 || yy < 0 || xx >= width || yy >= height) continue;
                const size_t q = (size_t)yy * width + xx;
                if (src_owner[q] == -1) continue;           // (the texel itself is among these)
                sr = sr + src[q * 3]; sg = sg + src[q * 3 + 1]; sb = sb + src[q * 3 + 2];
                cnt++;
            }
        if (cnt > 0)
        {
            const float d = (float)cnt;
            r = sr / d; g = sg / d; b = sb / d;
            o = -2;
        }
    }
    dst_owner[t] = o;
    dst[t * 3] = r; dst[t * 3 + 1] = g; dst[t * 3 + 2] = b;
}

inline unsigned texel_blocks(size_t n) { return (unsigned)((n + PTK_BAKE_BLOCK - 1) / PTK_BAKE_BLOCK); }

}  // namespace

void launch_bake_cover(const BakeParams& p, hipStream_t stream)
{
    if (p.num_tris <= 0) return;
    const int per_block = PTK_BAKE_BLOCK / 64;
    hipLaunchKernelGGL(bake_cover_kernel, dim3((p.num_tris + per_block - 1) / per_block), dim3(PTK_BAKE_BLOCK), 0, stream, p);
}

void launch_bake_count(const BakeParams& p, uint32_t* total, hipStream_t stream)
{
    const size_t texels = (size_t)p.width * p.height;
    hipLaunchKernelGGL(bake_count_kernel, dim3(texel_blocks(texels)), dim3(PTK_BAKE_BLOCK), 0, stream, p.plane, texels, p.block_counts);
    launch_bake_scan(p.block_counts, (uint32_t)texel_blocks(texels), total, stream);
}

void launch_bake_scan(uint32_t* counts, uint32_t n, uint32_t* total, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_scan_kernel, dim3(1), dim3(PTK_BAKE_SCAN), 0, stream, counts, n, total);
}

void launch_bake_rays(const BakeParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(bake_rays_kernel, dim3(texel_blocks((size_t)p.width * p.height)), dim3(PTK_BAKE_BLOCK), 0, stream, p);
}

void launch_bake_scatter(const float* sums, const uint32_t* texel, uint32_t count, float* out, hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(bake_scatter_kernel, dim3(texel_blocks(count)), dim3(PTK_BAKE_BLOCK), 0, stream, sums, texel, count, out);
}

void launch_dilate(const float* src_image, const int32_t* src_owner, float* dst_image, int32_t* dst_owner, int width, int height, hipStream_t stream)
{
    hipLaunchKernelGGL(dilate_kernel, dim3(texel_blocks((size_t)width * height)), dim3(PTK_BAKE_BLOCK), 0, stream, src_image, src_owner, dst_image,
                       dst_owner, width, height);
}

}  // namespace ptk
