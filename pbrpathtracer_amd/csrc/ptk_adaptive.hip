// HIP kernels for gfx950 of the adaptive render (include/ptk.h ptk_render_adaptive): rounds of `step` samples, after each of
// which converge_kernel decides which pixels need more.  The trace kernels of ptk_kernels.hip run unchanged, fed the round's
// traced mask and list (the list by launch_compact_list, ptk_frame.hip); this file holds what differs from a plain render:
//   * accumulate_adaptive_kernel - accumulate_kernel (ptk_frame.hip) for the round's active set: S1 and S2 folded in sample
//     order, a per-pixel sample count, the 8-bit resolve by that count (the pixel mapping and the resolve are the shared ones of
//     ptk_device_fn.h);
//   * converge_kernel - the test, the 3x3 dilation within the 16x16 tile, the next round's active and traced masks and the
//     active count that tells the host when to stop.
// Compiled with -ffp-contract=off like the exact build: S2 = S2 + v * v is a multiply and an add, and the test is float32 in
// the documented order - the tests recompute both in numpy.
#include "ptk_device_fn.h"
#include "ptk_adaptive.h"

namespace ptk {

// One workgroup per owned 16x16 tile, one wave per 8x8 quadrant, one thread per pixel (accumulate_kernel's layout).
__global__ __launch_bounds__(PTK_BLOCK) void accumulate_adaptive_kernel(const RenderParams P, const AdaptiveParams A)
{
    // an aborted pass adds and counts nothing (the trace waves that saw the exit flag stored nothing)
    if (P.exit_flag && __hip_atomic_load(P.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.exit_gen) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63, quad = tid >> 6;
    const int owned = blockIdx.x;
    const int tile = owned * P.world + P.rank;
    if (tile >= P.num_tiles) return;
    int tx, ty, px, py; tile_origin(tile, P.tiles_x, tx, ty);
    quadrant_pixel(tx, ty, quad, lane, px, py);
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
        b3[k] = resolve8(c3[k]);
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
__global__ __launch_bounds__(PTK_BLOCK) void converge_kernel(const RenderParams P, const ConvergeParams C)
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
    int tx, ty, px, py; tile_origin(tile, P.tiles_x, tx, ty);
    quadrant_pixel(tx, ty, quad, lane, px, py);
    const int lx = px - tx * PTK_TILE, ly = py - ty * PTK_TILE;      // the pixel within its tile
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

void launch_accumulate_adaptive(const RenderParams& p, const AdaptiveParams& a, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles > 0) hipLaunchKernelGGL(accumulate_adaptive_kernel, dim3(owned_tiles), dim3(PTK_BLOCK), 0, stream, p, a);
}
void launch_converge(const RenderParams& p, const ConvergeParams& cp, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles > 0) hipLaunchKernelGGL(converge_kernel, dim3(owned_tiles), dim3(PTK_BLOCK), 0, stream, p, cp);
}

}  // namespace ptk
