// HIP kernels for gfx950 of the adaptive render (include/ptk.h ptk_render_adaptive): rounds of `step` samples, after each of
// which converge_kernel decides which pixels need more.  The trace kernels of ptk_kernels.hip run unchanged, fed the round's
// traced mask and list; this file holds what differs from a plain render:
//   * accumulate_adaptive_kernel - accumulate_kernel (ptk_kernels.hip) for the round's active set: S1 and S2 folded in sample
//     order, a per-pixel sample count, the 8-bit resolve by that count;
//   * converge_kernel - the test, the 3x3 dilation within the 16x16 tile, the next round's active and traced masks and the
//     active count that tells the host when to stop;
//   * mask_compact_kernel - the ordered list of quadrants of the traced mask (live_compact_kernel's contract).
// Separate from ptk_kernels.hip so that the plain render's kernels stay exactly as they are.  Compiled with -ffp-contract=off
// like the exact build: S2 = S2 + v * v is a multiply and an add, and the test is float32 in the documented order - the
// tests recompute both in numpy.
#include "ptk_adaptive.h"

namespace ptk {

#define PTK_ABLOCK 256

// One workgroup per owned 16x16 tile, one wave per 8x8 quadrant, one thread per pixel (accumulate_kernel's layout).
__global__ __launch_bounds__(PTK_ABLOCK) void accumulate_adaptive_kernel(const RenderParams P, const AdaptiveParams A)
{
    // an aborted pass adds and counts nothing (the trace waves that saw the exit flag stored nothing)
    if (P.exit_flag && __hip_atomic_load(P.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.exit_gen) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63, quad = tid >> 6;
    const int owned = blockIdx.x;
    const int tile = owned * P.world + P.rank;
    if (tile >= P.num_tiles) return;
    const int ty = tile / P.tiles_x, tx = (tile % P.tiles_x + P.tiles_x - (3 * ty) % P.tiles_x) % P.tiles_x;
    const int px = tx * PTK_TILE + (quad & 1) * 8 + (lane & 7);
    const int py = ty * PTK_TILE + (quad >> 1) * 8 + (lane >> 3);
    if (px >= P.width || py >= P.height) return;
    const size_t pix = (size_t)(P.height - 1 - py) * P.width + px;      // bottom-up, like the accumulator
    const size_t accidx = pix * 3;
    const size_t subtile = (size_t)owned * 4 + quad;
    const unsigned long long am = A.active[subtile];
    const bool active = ((am >> lane) & 1ull) != 0ull;
    const bool traced = ((P.live_mask[subtile] >> lane) & 1ull) != 0ull;     // (traced implies active)
    float a0 = P.accum[accidx], a1 = P.accum[accidx + 1], a2 = P.accum[accidx + 2];
    uint32_t cnt = A.counts[pix];
    if (active)
    {
        if (traced)
        {
            float q0 = A.moments[accidx], q1 = A.moments[accidx + 1], q2 = A.moments[accidx + 2];
            // sample s of this pixel sits at in[s * 64] (chunk after chunk of its quadrant's items); added in sample order
            const float4* in = P.samples + (subtile * P.num_chunks * P.chunk) * 64 + lane;
            for (uint32_t s = 0; s < P.spp; s++)
            {
                const float4 v = in[(size_t)s * 64];
                a0 = a0 + v.x; a1 = a1 + v.y; a2 = a2 + v.z;
                const float s0 = v.x * v.x, s1 = v.y * v.y, s2 = v.z * v.z;
                q0 = q0 + s0; q1 = q1 + s1; q2 = q2 + s2;
            }
            P.accum[accidx] = a0; P.accum[accidx + 1] = a1; P.accum[accidx + 2] = a2;
            A.moments[accidx] = q0; A.moments[accidx + 1] = q1; A.moments[accidx + 2] = q2;
        }
        cnt += P.spp;                                // (an active pixel that is never traced receives black samples: S1, S2 stay 0)
        A.counts[pix] = cnt;
        // every active pixel holds the same count (the set only shrinks): the quadrant's first one reports for all
        if (lane == __ffsll((unsigned long long)am) - 1)
        {
            atomicAdd(&A.stats[0], (unsigned long long)__popcll(am) * P.spp);
            atomicMax(&A.stats[1], (unsigned long long)cnt);
        }
    }
    // the 8-bit resolve (pathtracer.cpp:802-812) by the pixel's own count
    const float ns = (float)cnt;
    const float c3[3] = { a0 / ns, a1 / ns, a2 / ns };
    uint8_t b3[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        float x = c3[k];
        x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
        if (!(x == x)) x = 0.0f;
        b3[k] = (uint8_t)(x * 255);
        if (active) P.rgb8[accidx + k] = b3[k];
    }
    if (P.rgb8_host)
    {
        // the bound hand-off buffer, as accumulate_kernel writes it (a row of the quadrant gathered with lane shuffles into six
        // dwords).  A pixel outside the active set is skipped: the pass of the round it left the set in wrote its final value.
        const bool skip_host = !active && !P.rgb8_host_full;
        const uint32_t mine = (uint32_t)b3[0] | ((uint32_t)b3[1] << 8) | ((uint32_t)b3[2] << 16);
        const unsigned long long row_live = (__ballot(!skip_host) >> (lane & ~7)) & 0xffull;
        const int d = lane & 7;
        const int p0 = (4 * d) / 3, p1 = min(7, (4 * d + 3) / 3), sh = (4 * d) % 3;
        const uint32_t w0 = (uint32_t)__shfl((int)mine, (lane & ~7) + min(p0, 7)), w1 = (uint32_t)__shfl((int)mine, (lane & ~7) + p1);
        const uint32_t word = (w0 >> (8 * sh)) | (w1 << (8 * (3 - sh)));
        const bool aligned = (((size_t)P.width * 3) & 3) == 0 && (((uintptr_t)P.rgb8_host) & 3) == 0;
        const int row_px = min(8, P.width - (px - (lane & 7)));
        if (aligned && row_px == 8)
        {
            if (d < 6 && row_live != 0ull) *(uint32_t*)(P.rgb8_host + accidx - (size_t)(lane & 7) * 3 + d * 4) = word;
        }
        else if (!skip_host)
        {
            P.rgb8_host[accidx] = b3[0]; P.rgb8_host[accidx + 1] = b3[1]; P.rgb8_host[accidx + 2] = b3[2];
        }
    }
}

// After a round: which pixels go on.  One workgroup per owned tile, one wave per quadrant, one lane per pixel.  A lane tests its
// pixel; the quadrants' "active and not done" ballots meet in LDS; a pixel stays active when some such pixel lies in its 3x3
// neighbourhood clipped to the tile (pixels off the image are never active, which clips to the image).  Writes the new active
// mask in place (each workgroup reads and writes only its own tile's four words), the traced mask base & active, and adds the
// active pixels to the count the host reads.
__global__ __launch_bounds__(PTK_ABLOCK) void converge_kernel(const RenderParams P, const ConvergeParams C)
{
    __shared__ unsigned long long need[4];
    __shared__ int stand_down;
    const int tid = threadIdx.x, lane = tid & 63, quad = tid >> 6;
    // (read once for the workgroup: its four waves exchange masks, so they stand down together or not at all)
    if (tid == 0) stand_down = P.exit_flag && __hip_atomic_load(P.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.exit_gen;
    __syncthreads();
    if (stand_down) return;
    const int owned = blockIdx.x, tile = owned * P.world + P.rank;
    if (tile >= P.num_tiles) return;                 // (uniform over the workgroup)
    const int ty = tile / P.tiles_x, tx = (tile % P.tiles_x + P.tiles_x - (3 * ty) % P.tiles_x) % P.tiles_x;
    const int lx = (quad & 1) * 8 + (lane & 7), ly = (quad >> 1) * 8 + (lane >> 3);
    const int px = tx * PTK_TILE + lx, py = ty * PTK_TILE + ly;
    const size_t subtile = (size_t)owned * 4 + quad;
    const bool act = px < P.width && py < P.height && (C.init || ((C.active[subtile] >> lane) & 1ull) != 0ull);
    bool open = act;
    if (act && C.test)
    {
        const size_t pix = (size_t)(P.height - 1 - py) * P.width + px;
        const float nf = (float)C.counts[pix];
        float m[3], v[3];
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            m[k] = C.accum[pix * 3 + k] / nf;
            const float e2 = C.moments[pix * 3 + k] / nf;
            const float mm = m[k] * m[k];
            const float x = e2 - mm;
            v[k] = x < 0.0f ? 0.0f : x;              // (NaN stays NaN)
        }
        const float err2 = ((v[0] + v[1]) + v[2]) / (3.0f * (nf - 1.0f));
        const float lum = ((m[0] + m[1]) + m[2]) / 3.0f;
        const float tol = C.threshold * (lum + 1.0f / 256.0f);
        const float tol2 = tol * tol;
        open = !(err2 < tol2);                       // strict: threshold 0 and NaN never converge
    }
    const unsigned long long nm = __ballot(open);
    if (lane == 0) need[quad] = nm;
    __syncthreads();
    bool keep = false;
    if (act)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++)
            {
                const int nx = lx + dx, ny = ly + dy;
                if (nx < 0 || ny < 0 || nx >= PTK_TILE || ny >= PTK_TILE) continue;
                keep = keep || ((need[(ny >> 3) * 2 + (nx >> 3)] >> ((ny & 7) * 8 + (nx & 7))) & 1ull) != 0ull;
            }
    const unsigned long long am = __ballot(keep);
    if (lane == 0)
    {
        C.active[subtile] = am;
        C.traced[subtile] = am & C.base[subtile];
        if (am) atomicAdd(C.active_count, (unsigned)__popcll(am));
    }
}

// Ordered list of the quadrants with a non-zero mask, and their number (one workgroup: a few hundred thousand quadrants at most)
__global__ __launch_bounds__(1024) void mask_compact_kernel(const unsigned long long* mask, int num_subtiles, unsigned* list, unsigned* count)
{
    __shared__ unsigned wave_total[16];
    __shared__ unsigned base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int s0 = 0; s0 < num_subtiles; s0 += 1024)
    {
        const int sidx = s0 + t;
        const bool live = sidx < num_subtiles && mask[sidx] != 0ull;
        const unsigned long long b = __ballot(live);
        if (lane == 0) wave_total[wave] = (unsigned)__popcll(b);
        __syncthreads();
        unsigned before = base;
        for (int w = 0; w < wave; w++) before += wave_total[w];
        if (live) list[before + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = (unsigned)sidx;
        __syncthreads();
        if (t == 0) { unsigned sum = 0; for (int w = 0; w < 16; w++) sum += wave_total[w]; base += sum; }
        __syncthreads();
    }
    if (t == 0) *count = base;
}

void launch_accumulate_adaptive(const RenderParams& p, const AdaptiveParams& a, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles > 0) hipLaunchKernelGGL(accumulate_adaptive_kernel, dim3(owned_tiles), dim3(PTK_ABLOCK), 0, stream, p, a);
}
void launch_converge(const RenderParams& p, const ConvergeParams& cp, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles > 0) hipLaunchKernelGGL(converge_kernel, dim3(owned_tiles), dim3(PTK_ABLOCK), 0, stream, p, cp);
}
void launch_mask_compact(const unsigned long long* mask, int num_subtiles, unsigned* list, unsigned* count, hipStream_t stream)
{
    if (num_subtiles > 0) hipLaunchKernelGGL(mask_compact_kernel, dim3(1), dim3(1024), 0, stream, mask, num_subtiles, list, count);
}

}  // namespace ptk
