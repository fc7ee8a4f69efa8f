// HIP kernels for gfx950 of the display transform (include/ptk.h ptk_display_planes, ptk_display_frame).
//   * display_meter_kernel - the luminance histogram: a thread takes four consecutive pixels (three 16-byte loads), a block bins
//     into 2048 LDS counters with LDS atomics and sends its non-zero bins to the global histogram with 32-bit atomic adds;
//   * display_exposure_kernel - one workgroup: prefix sum over the bins, the kept range, its bin sum, the division, the state
//     update; clears the histogram for the next call;
//   * display_apply_kernel - exposure, tone curve and encoding of the same four pixels, twelve bytes as three dword stores.
// Compiled once, with -ffp-contract=off: every expression below is the rule of ptk.h operation by operation, and `/` is the IEEE
// quotient (the numpy restatement is tests/display_rule.py).  The histogram is summed with integer atomics, so the order of the adds
// does not matter.  No persistent waves: the meter's grid-stride loop is bounded by the image, everything else is one pass.
#include "ptk_device_fn.h"
#include "ptk_display.h"

namespace ptk {

__device__ const float d_display_srgb[256] = { PTK_DISPLAY_SRGB_VALUES };

// The pixels of quad q - 4q .. 4q+n-1, n in 1..4 - as the source defines them: v[3k + c] is channel c of pixel 4q+k.  `vec`: the
// colour plane starts on a 16-byte boundary, so a whole quad is three 16-byte loads.  Unused slots are 0.
template <int KIND>
__device__ __forceinline__ void display_load(const DisplaySource& S, const bool vec, const size_t q, const int n, float v[12])
{
    if (vec && n == 4)
    {
        const float4* p = (const float4*)(S.color + 12 * q);
        const float4 a = p[0], b = p[1], c = p[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = k < 3 * n ? S.color[12 * q + k] : 0.0f;
    }
    if (KIND == DISPLAY_SRC_PLANE) return;
    // the accumulator: S1 / (float)n_p, 0 where n_p = 0
    uint32_t cnt[4];
    if (KIND == DISPLAY_SRC_ACCUM_COUNTS)
    {
        if (n == 4) { const uint4 u = *(const uint4*)(S.counts + 4 * q); cnt[0] = u.x; cnt[1] = u.y; cnt[2] = u.z; cnt[3] = u.w; }
        else
        {
#pragma unroll
            for (int k = 0; k < 4; k++) cnt[k] = k < n ? S.counts[4 * q + k] : 0u;
        }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            cnt[k] = (uint32_t)S.samples;
            if (S.world > 1)
            {
                // rows are stored bottom-up; the tiles count from the image's top-left (tile_origin's map, inverted)
                const size_t i = 4 * q + k;
                const int y = (int)(i / (size_t)S.width), x = (int)(i - (size_t)y * S.width);
                const int ty = (S.height - 1 - y) / PTK_TILE, tx = x / PTK_TILE, tiles_x = (S.width + PTK_TILE - 1) / PTK_TILE;
                const int tile = ty * tiles_x + (tx + 3 * ty) % tiles_x;
                if (tile % S.world != S.rank) cnt[k] = 0u;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const float nf = (float)cnt[k];
        const bool have = k < n && cnt[k] > 0u;
        v[3 * k] = have ? v[3 * k] / nf : 0.0f;
        v[3 * k + 1] = have ? v[3 * k + 1] / nf : 0.0f;
        v[3 * k + 2] = have ? v[3 * k + 2] / nf : 0.0f;
    }
}

// Neighbouring pixels usually share a bin.  A thread folds equal neighbours among its four pixels into one add; a wave whose
// lanes all hold the same single bin - a flat region - sends one add for all of them.
template <int KIND>
__global__ __launch_bounds__(DISPLAY_BLOCK) void display_meter_kernel(const DisplayMeterParams P)
{
    __shared__ uint32_t h[DISPLAY_BINS];
    for (int b = threadIdx.x; b < DISPLAY_BINS; b += DISPLAY_BLOCK) h[b] = 0u;
    __syncthreads();
    const size_t px = (size_t)P.src.width * P.src.height, nq = (px + 3) / 4;
    const bool vec = ((uintptr_t)P.src.color & 15) == 0;
    const int lane = threadIdx.x & 63;
    // (the bound is uniform over the block, so every lane of a wave reaches the wave-wide operations below)
    for (size_t q0 = (size_t)blockIdx.x * DISPLAY_BLOCK; q0 < nq; q0 += (size_t)gridDim.x * DISPLAY_BLOCK)
    {
        const size_t q = q0 + threadIdx.x;
        int n = 0;
        if (q < nq) { const size_t rem = px - 4 * q; n = rem < 4 ? (int)rem : 4; }
        float v[12];
        if (n > 0) display_load<KIND>(P.src, vec, q, n, v);
        const uint32_t NONE = 0xffffffffu;
        uint32_t bin[4], cnt[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            bin[k] = NONE; cnt[k] = 0u;
            if (k < n)
            {
                const float L = ((0.2126f * v[3 * k]) + (0.7152f * v[3 * k + 1])) + (0.0722f * v[3 * k + 2]);
                if (L >= P.min_lum && L <= P.max_lum) { bin[k] = __float_as_uint(L) >> 20; cnt[k] = 1u; }
            }
        }
        // a run of equal bins collects in its last pixel
#pragma unroll
        for (int k = 1; k < 4; k++)
            if (bin[k] == bin[k - 1] && bin[k] != NONE) { cnt[k] += cnt[k - 1]; cnt[k - 1] = 0u; }
        uint32_t tb = NONE, tc = 0u;
        int runs = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (cnt[k] > 0u) { tb = bin[k]; tc = cnt[k]; runs++; }
        const unsigned long long holders = __ballot(runs > 0);
        if (holders == 0ull) continue;
        const uint32_t ref = (uint32_t)__shfl((int)tb, __ffsll((long long)holders) - 1);
        if (__all(runs == 0 || (runs == 1 && tb == ref)))
        {
            uint32_t total = tc;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) total += (uint32_t)__shfl_xor((int)total, off);
            if (lane == 0) atomicAdd(&h[ref], total);
        }
        else
        {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (cnt[k] > 0u) atomicAdd(&h[bin[k]], cnt[k]);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < DISPLAY_BINS; b += DISPLAY_BLOCK)
    {
        const uint32_t n = h[b];
        if (n != 0u) atomicAdd(&P.hist[b], n);
    }
}

// One workgroup; thread t owns the bins 8t .. 8t+7.
__global__ __launch_bounds__(DISPLAY_BLOCK) void display_exposure_kernel(const DisplayExposureParams P)
{
    static_assert(DISPLAY_BINS == 8 * DISPLAY_BLOCK, "eight bins per thread");
    __shared__ unsigned long long scan[DISPLAY_BLOCK], red[DISPLAY_BLOCK];
    const int t = threadIdx.x;
    uint32_t c[8];
    unsigned long long own = 0ull;
#pragma unroll
    for (int k = 0; k < 8; k++) { c[k] = P.hist[8 * t + k]; own += c[k]; }
#pragma unroll
    for (int k = 0; k < 8; k++) P.hist[8 * t + k] = 0u;          // cleared for the next call
    scan[t] = own;
    __syncthreads();
    for (int off = 1; off < DISPLAY_BLOCK; off <<= 1)
    {
        const unsigned long long below = t >= off ? scan[t - off] : 0ull;
        __syncthreads();
        scan[t] += below;
        __syncthreads();
    }
    const unsigned long long N = scan[DISPLAY_BLOCK - 1];
    const unsigned long long lo = N * P.low_permille / 1000ull;
    unsigned long long hi = N * P.high_permille / 1000ull;
    if (hi <= lo) hi = lo + 1ull;
    // the pixels of rank [lo, hi) in bin order: this thread's share of S = the sum of their bins
    unsigned long long r = scan[t] - own, S = 0ull;
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        const unsigned long long a = r > lo ? r : lo, e = r + c[k];
        const unsigned long long b = e < hi ? e : hi;
        if (b > a) S += (b - a) * (unsigned long long)(8 * t + k);
        r = e;
    }
    red[t] = S;
    __syncthreads();
    for (int off = DISPLAY_BLOCK / 2; off > 0; off >>= 1)
    {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t != 0) return;
    S = red[0];
    const ptk_exposure_state prev = *P.state;
    const bool has_prev = prev.has_prev != 0u;
    float target, lavg = 0.0f;
    unsigned long long K = 0ull;
    if (N > 0ull)
    {
        K = hi - lo;
        const unsigned long long mbits = ((S << 20) + (K << 19)) / K;
        lavg = __uint_as_float((uint32_t)mbits);
        target = P.key / lavg;
        target = target > P.min_exposure ? target : P.min_exposure;
        target = target < P.max_exposure ? target : P.max_exposure;
    }
    else target = has_prev ? prev.exposure : 1.0f;
    const float e = (!has_prev || P.adapt >= 1.0f) ? target : prev.exposure + ((target - prev.exposure) * P.adapt);
    ptk_exposure_state now;
    now.exposure = e; now.target = target; now.lavg = lavg; now.has_prev = (has_prev || N > 0ull) ? 1u : 0u;
    now.counted = N; now.kept = K;
    *P.state = now;
}

template <int KIND>
__global__ __launch_bounds__(DISPLAY_BLOCK) void display_apply_kernel(const DisplayApplyParams P)
{
    __shared__ float T[256];
    static_assert(DISPLAY_BLOCK == 256, "one table entry per thread");
    if (P.transfer == PTK_TRANSFER_SRGB)
    {
        T[threadIdx.x] = d_display_srgb[threadIdx.x];
        __syncthreads();
    }
    const size_t px = (size_t)P.src.width * P.src.height, nq = (px + 3) / 4;
    const size_t q = (size_t)blockIdx.x * DISPLAY_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const size_t rem = px - 4 * q;
    const int n = rem < 4 ? (int)rem : 4;
    const float e = P.state ? P.state->exposure : P.exposure;
    float v[12];
    display_load<KIND>(P.src, ((uintptr_t)P.src.color & 15) == 0, q, n, v);
    uint32_t byte[12];
#pragma unroll
    for (int k = 0; k < 12; k++)
    {
        float x = v[k] * e;
        x = x > 0.0f ? x : 0.0f;
        float y;
        if (P.op == PTK_DISPLAY_REINHARD) y = (x * (1.0f + (x * P.iw2))) / (1.0f + x);
        else if (P.op == PTK_DISPLAY_ACES) y = (x * ((2.51f * x) + 0.03f)) / ((x * ((2.43f * x) + 0.59f)) + 0.14f);
        else y = x;
        y = y < 1.0f ? y : 1.0f;
        if (P.transfer == PTK_TRANSFER_SRGB)
        {
            // the largest k with T[k] <= y (T[0] = 0 <= y always) is the count of the thresholds 1..255 at or below y
            uint32_t at = 0u;
#pragma unroll
            for (uint32_t step = 128u; step > 0u; step >>= 1)
                if (T[at + step] <= y) at += step;
            byte[k] = at;
        }
        else byte[k] = (uint32_t)(uint8_t)(y * 255);
    }
    uint8_t* out = P.rgb8 + 12 * q;
    if (n == 4 && ((uintptr_t)P.rgb8 & 3) == 0)
    {
        uint32_t* o = (uint32_t*)out;
#pragma unroll
        for (int w = 0; w < 3; w++) o[w] = byte[4 * w] | (byte[4 * w + 1] << 8) | (byte[4 * w + 2] << 16) | (byte[4 * w + 3] << 24);
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (k < 3 * n) out[k] = (uint8_t)byte[k];
    }
}

static unsigned quad_blocks(const DisplaySource& s)
{
    const size_t nq = ((size_t)s.width * s.height + 3) / 4;
    return (unsigned)((nq + DISPLAY_BLOCK - 1) / DISPLAY_BLOCK);
}

void launch_display_meter(const DisplayMeterParams& p, hipStream_t stream)
{
    unsigned blocks = quad_blocks(p.src);
    if (blocks > (unsigned)DISPLAY_METER_BLOCKS) blocks = DISPLAY_METER_BLOCKS;
    const dim3 grid(blocks), block(DISPLAY_BLOCK);
    if (p.src.kind == DISPLAY_SRC_ACCUM_COUNTS) hipLaunchKernelGGL(display_meter_kernel<DISPLAY_SRC_ACCUM_COUNTS>, grid, block, 0, stream, p);
    else if (p.src.kind == DISPLAY_SRC_ACCUM_SAMPLES) hipLaunchKernelGGL(display_meter_kernel<DISPLAY_SRC_ACCUM_SAMPLES>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(display_meter_kernel<DISPLAY_SRC_PLANE>, grid, block, 0, stream, p);
}

void launch_display_exposure(const DisplayExposureParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(display_exposure_kernel, dim3(1), dim3(DISPLAY_BLOCK), 0, stream, p);
}

void launch_display_apply(const DisplayApplyParams& p, hipStream_t stream)
{
    const dim3 grid(quad_blocks(p.src)), block(DISPLAY_BLOCK);
    if (p.src.kind == DISPLAY_SRC_ACCUM_COUNTS) hipLaunchKernelGGL(display_apply_kernel<DISPLAY_SRC_ACCUM_COUNTS>, grid, block, 0, stream, p);
    else if (p.src.kind == DISPLAY_SRC_ACCUM_SAMPLES) hipLaunchKernelGGL(display_apply_kernel<DISPLAY_SRC_ACCUM_SAMPLES>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(display_apply_kernel<DISPLAY_SRC_PLANE>, grid, block, 0, stream, p);
}

}  // namespace ptk
