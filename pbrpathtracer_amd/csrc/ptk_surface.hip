// HIP kernels for gfx950 of surface sampling (include/ptk.h ptk_sample_surface): area-weighted points on the scene's triangles.
// Four steps, each its own launch: the weight of every triangle with the largest one folded as a bit pattern
// (surface_weights_kernel); the weights as integers of 36 bits (surface_quantise_kernel); their inclusive sums, exact in uint64 and
// therefore the same bits in any order - reduce-then-scan over separate launches, no workgroup ever waits for another
// (scan_reduce_kernel, scan_apply_kernel, launch_scan_u64) -; and the sampler, one thread per sample: four integer draws, the high
// half of a 64 x 64 bit product, a binary search over the sums, a 36-byte vertex gather (surface_sample_kernel).  No BVH, no
// state of the render.  Compiled once, with -ffp-contract=off: the float operations are the rule of ptk.h one by one (the numpy
// restatement is tests/surface_sample_rule.py).
#include "ptk_device_fn.h"
#include "ptk_surface.h"

namespace ptk {

#define PTK_SURF_BLOCK 256
#define PTK_SURF_COARSE 1024        // entries of the coarse table (8 KiB)

static unsigned surf_blocks(size_t n) { return (unsigned)((n + PTK_SURF_BLOCK - 1) / PTK_SURF_BLOCK); }

// ---- the weight table ---------------------------------------------------------------------------------------------------------
// a_i = 0.5 * |cross(v2 - v1, v3 - v1)| (* w_i), and what the host needs of all of them in eight bytes: the largest as the bit
// pattern of a non-negative float - patterns of non-negative floats order as the floats do, so the maximum is exact and free of
// order -, one atomicMax per wave, and a flag word for an area that is not finite or a weight that is negative or not finite.
__global__ __launch_bounds__(PTK_SURF_BLOCK) void surface_weights_kernel(const float* __restrict__ verts, const float* __restrict__ weights,
                                                                         int num_tris, uint64_t* __restrict__ table, uint32_t* __restrict__ red)
{
    const int i = blockIdx.x * PTK_SURF_BLOCK + threadIdx.x;
    uint32_t bits = 0u, flag = 0u;
    if (i < num_tris)
    {
        const float* v = verts + (size_t)i * 9;
        const v3 v1 = V(v[0], v[1], v[2]), v2 = V(v[3], v[4], v[5]), v3_ = V(v[6], v[7], v[8]);
        const v3 c = cross(sub(v2, v1), sub(v3_, v1));
        float a = 0.5f * sqrt_ieee((c.x * c.x + c.y * c.y) + c.z * c.z);
        if (weights)
        {
            const float w = weights[i];
            if (!(w >= 0.0f) || w == __builtin_inff()) flag |= SURF_FLAG_WEIGHT;
            a = a * w;
        }
        if (!(a <= 3.40282347e38f)) flag |= SURF_FLAG_AREA;               // (inf and NaN)
        bits = flag ? 0u : (__float_as_uint(a) & 0x7fffffffu);             // (a weight of -0 makes a -0: a zero like the other)
        table[i] = bits;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        bits = max(bits, (uint32_t)__shfl_xor((int)bits, d));
        flag |= (uint32_t)__shfl_xor((int)flag, d);
    }
    if ((threadIdx.x & 63) == 0)
    {
        if (bits) atomicMax(&red[SURF_RED_MAX], bits);
        if (flag) atomicOr(&red[SURF_RED_FLAG], flag);
    }
}

__global__ __launch_bounds__(PTK_SURF_BLOCK) void surface_check_weights_kernel(const float* __restrict__ weights, int num_tris, uint32_t* __restrict__ flag)
{
    const int i = blockIdx.x * PTK_SURF_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < num_tris) { const float w = weights[i]; bad = !(w >= 0.0f) || w == __builtin_inff(); }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, (uint32_t)SURF_FLAG_WEIGHT);
}

// q_i = trunc(a_i * 2^shift), shift = 35 - floor(log2 max a): the scaling is a change of exponent in float64, exact, so q_i < 2^36
__global__ __launch_bounds__(PTK_SURF_BLOCK) void surface_quantise_kernel(uint64_t* __restrict__ table, int num_tris, int shift, uint32_t* __restrict__ red)
{
    const int i = blockIdx.x * PTK_SURF_BLOCK + threadIdx.x;
    uint64_t q = 0;
    if (i < num_tris)
    {
        q = (uint64_t)ldexp((double)__uint_as_float((uint32_t)table[i]), shift);
        table[i] = q;
    }
    const unsigned long long m = __ballot(q != 0);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&red[SURF_RED_DRAWABLE], (uint32_t)__popcll(m));
}

// every ceil(N / 1024)-th inclusive sum, for the sampler's COARSE variant: coarse[k] closes the triangles [k S, (k + 1) S)
__global__ __launch_bounds__(PTK_SURF_BLOCK) void surface_coarse_kernel(const uint64_t* __restrict__ incl, int num_tris, uint64_t* __restrict__ coarse)
{
    const int k = blockIdx.x * PTK_SURF_BLOCK + threadIdx.x;
    if (k >= PTK_SURF_COARSE) return;
    const int64_t stride = ((int64_t)num_tris + PTK_SURF_COARSE - 1) / PTK_SURF_COARSE;
    const int64_t last = min((int64_t)num_tris - 1, (int64_t)(k + 1) * stride - 1);
    coarse[k] = incl[last];
}

// ---- the exact prefix sum ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}
__device__ __forceinline__ uint64_t wave_inclusive(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, (unsigned)d);
        if (lane >= (uint32_t)d) v += t;
    }
    return v;
}

// sums[g] = the sum of workgroup g's items [g items, min(n, (g + 1) items))
__global__ __launch_bounds__(PTK_SURF_BLOCK) void scan_reduce_kernel(const uint64_t* __restrict__ in, size_t n, int items, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wave_tot[PTK_SURF_BLOCK / 64];
    const size_t begin = (size_t)blockIdx.x * (size_t)items, end = min(n, begin + (size_t)items);
    uint64_t s = 0;
    for (size_t i = begin + threadIdx.x; i < end; i += PTK_SURF_BLOCK) s += in[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = ((wave_tot[0] + wave_tot[1]) + wave_tot[2]) + wave_tot[3];
}

// out[i] = offsets[g - 1] + in[g items] + .. + in[i] for the items of workgroup g: the scan of one workgroup's items in rounds of 256,
// on top of the scanned sums of the workgroups before it (offsets null: there is one workgroup)
__global__ __launch_bounds__(PTK_SURF_BLOCK) void scan_apply_kernel(const uint64_t* in, uint64_t* out, size_t n, int items, const uint64_t* __restrict__ offsets)
{
    __shared__ uint64_t wave_tot[PTK_SURF_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t begin = (size_t)blockIdx.x * (size_t)items, end = min(n, begin + (size_t)items);
    uint64_t carry = (offsets && blockIdx.x > 0) ? offsets[blockIdx.x - 1] : 0;
    for (size_t base = begin; base < end; base += PTK_SURF_BLOCK)
    {
        const size_t i = base + threadIdx.x;
        uint64_t v = wave_inclusive(i < end ? in[i] : 0, lane);
        if (lane == 63) wave_tot[wave] = v;
        __syncthreads();
        const uint64_t t0 = wave_tot[0], t1 = wave_tot[1], t2 = wave_tot[2], t3 = wave_tot[3];
        v += carry + (wave > 0 ? t0 : 0) + (wave > 1 ? t1 : 0) + (wave > 2 ? t2 : 0);
        if (i < end) out[i] = v;
        carry += ((t0 + t1) + t2) + t3;
        __syncthreads();
    }
}

size_t scan_u64_sums(size_t n, int items)
{
    size_t total = 0;
    if (items < 2) return 0;
    for (size_t g = (n + items - 1) / items; g > 1; g = (g + items - 1) / items) total += g;
    return total;
}

void launch_scan_u64(const uint64_t* d_in, uint64_t* d_out, size_t n, int items, uint64_t* d_sums, hipStream_t stream)
{
    if (n == 0 || items < 2) return;
    const size_t groups = (n + items - 1) / items;
    if (groups == 1)
    {
        hipLaunchKernelGGL(scan_apply_kernel, dim3(1), dim3(PTK_SURF_BLOCK), 0, stream, d_in, d_out, n, items, (const uint64_t*)nullptr);
        return;
    }
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)groups), dim3(PTK_SURF_BLOCK), 0, stream, d_in, n, items, d_sums);
    launch_scan_u64(d_sums, d_sums, groups, items, d_sums + groups, stream);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)groups), dim3(PTK_SURF_BLOCK), 0, stream, d_in, d_out, n, items, (const uint64_t*)d_sums);
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------
// Sample j of the call: the stream of (seed, RNG pixel key_base + j, sample) as rays_kernel sets it up, four raw outputs; the first
// two pick the triangle - target = floor(r64 total / 2^64) < total, tri = the first inclusive sum above it, which is never a
// triangle with q = 0 -, the other two the point, in sample_direct_light's form.
// COARSE: the workgroup stages the coarse table in LDS and searches it first, then its stride of the sums; speed only, the
// default (DESIGN.md 4.26 has both measured, and the LDS transposition of the outputs that lost: tools/experiments/surface_deal.patch).
template <bool COARSE>
__global__ __launch_bounds__(PTK_SURF_BLOCK) void surface_sample_kernel(const SurfaceSampleParams P)
{
    __shared__ uint64_t lds_coarse[COARSE ? PTK_SURF_COARSE : 1];
    const uint32_t j = blockIdx.x * PTK_SURF_BLOCK + threadIdx.x;
    const bool live = j < (uint32_t)P.num;
    const int num_tris = P.num_tris;
    const uint64_t* __restrict__ incl = P.incl;
    if (COARSE)
    {
        const uint64_t* coarse = incl + num_tris;                          // (the table's 1024 words behind the sums)
#pragma unroll
        for (int k = 0; k < PTK_SURF_COARSE / PTK_SURF_BLOCK; k++) lds_coarse[k * PTK_SURF_BLOCK + threadIdx.x] = coarse[k * PTK_SURF_BLOCK + threadIdx.x];
        __syncthreads();
    }
    if (!live) return;

    const uint32_t pkey = pixel_key(P.seed_lo, P.seed_hi, P.key_base + j);
    const uint32_t inc = (hash32(pkey ^ 0x9E3779B9u) << 1) | 1u;
    uint32_t state = hash32(P.sample + pkey);
    const uint32_t r0 = pcg_out(state); state = state * 747796405u + inc;
    const uint32_t r1 = pcg_out(state); state = state * 747796405u + inc;
    const uint32_t r2 = pcg_out(state); state = state * 747796405u + inc;
    const uint32_t r3 = pcg_out(state);
    const uint64_t total = incl[num_tris - 1];
    const uint64_t target = __umul64hi(((uint64_t)r0 << 32) | (uint64_t)r1, total);
    int lo = 0, hi = num_tris - 1;
    if (COARSE)
    {
        int clo = 0, chi = PTK_SURF_COARSE - 1;
        while (clo < chi)
        {
            const int mid = (clo + chi) >> 1;
            if (lds_coarse[mid] > target) chi = mid; else clo = mid + 1;
        }
        const int64_t stride = ((int64_t)num_tris + PTK_SURF_COARSE - 1) / PTK_SURF_COARSE;
        lo = (int)min((int64_t)num_tris - 1, (int64_t)clo * stride);
        hi = (int)min((int64_t)num_tris - 1, (int64_t)(clo + 1) * stride - 1);
    }
    while (lo < hi)                                                    // at most 27 probes: num_tris < 2^27
    {
        const int mid = (int)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (incl[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int tri = lo;
    const float su = sqrt_ieee(u01(r2)), sv = u01(r3);
    const float w0 = 1.0f - su, w1 = su * (1.0f - sv), w2 = su * sv;
    const float* v = P.verts + (size_t)tri * 9;
    const v3 v1 = V(v[0], v[1], v[2]), v2 = V(v[3], v[4], v[5]), v3_ = V(v[6], v[7], v[8]);
    const v3 pos = add(add(muls(v1, w0), muls(v2, w1)), muls(v3_, w2));
    v3 nrm = V(0.0f, 0.0f, 0.0f);
    int mat = 0;
    if (P.normal || P.material)
    {
        const float4 s0 = ldg4(P.shade + (size_t)tri * SHADE_F4);
        nrm = V(s0.x, s0.y, s0.z);
        mat = __float_as_int(s0.w) & 0x7fffffff;
    }
    if (P.tri) P.tri[j] = tri;
    if (P.material) P.material[j] = mat;
    if (P.bary) *reinterpret_cast<float2*>(P.bary + (size_t)j * 2) = make_float2(w1, w2);          // (8-byte aligned: ptk.h)
    if (P.position) { float* o = P.position + (size_t)j * 3; o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; }
    if (P.normal) { float* o = P.normal + (size_t)j * 3; o[0] = nrm.x; o[1] = nrm.y; o[2] = nrm.z; }
}

void launch_surface_weights(const float* d_verts, const float* d_weights, int num_tris, uint64_t* d_table, uint32_t* d_red, hipStream_t stream)
{
    if (num_tris > 0) hipLaunchKernelGGL(surface_weights_kernel, dim3(surf_blocks(num_tris)), dim3(PTK_SURF_BLOCK), 0, stream, d_verts, d_weights, num_tris, d_table, d_red);
}
void launch_surface_check_weights(const float* d_weights, int num_tris, uint32_t* d_flag, hipStream_t stream)
{
    if (num_tris > 0) hipLaunchKernelGGL(surface_check_weights_kernel, dim3(surf_blocks(num_tris)), dim3(PTK_SURF_BLOCK), 0, stream, d_weights, num_tris, d_flag);
}
void launch_surface_quantise(uint64_t* d_table, int num_tris, int shift, uint32_t* d_red, hipStream_t stream)
{
    if (num_tris > 0) hipLaunchKernelGGL(surface_quantise_kernel, dim3(surf_blocks(num_tris)), dim3(PTK_SURF_BLOCK), 0, stream, d_table, num_tris, shift, d_red);
}
void launch_surface_coarse(uint64_t* d_table, int num_tris, hipStream_t stream)
{
    if (num_tris > 0) hipLaunchKernelGGL(surface_coarse_kernel, dim3(PTK_SURF_COARSE / PTK_SURF_BLOCK), dim3(PTK_SURF_BLOCK), 0, stream, d_table, num_tris, d_table + num_tris);
}

void launch_surface_sample(const SurfaceSampleParams& p, int variant, hipStream_t stream)
{
    if (p.num <= 0 || p.num_tris <= 0) return;
    const dim3 grid(surf_blocks((size_t)p.num)), block(PTK_SURF_BLOCK);
    if (variant & SURF_VARIANT_COARSE) hipLaunchKernelGGL(surface_sample_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(surface_sample_kernel<false>, grid, block, 0, stream, p);
}

}  // namespace ptk
