// Geometry updates after ptk_upload_scene: see ptk_refit.h and DESIGN.md §4.10.
//
// Nothing here decides topology: the node links, the leaf order and the leaf sizes stay what the builder made.  The records
// are rewritten with the packers' own subtractions (bvh_device.hip pack_tris_kernel / pack_shade_kernel, ptk_api.hip's host
// packing), the child boxes with the builders' own padding and quantiser (bvh_quantise.h), so that an update with the
// uploaded arrays changes no bit and an update with moved arrays leaves what an upload of them would compute per record.
// Levels are separate launches on one stream: stream order is the only barrier between them.
#include "ptk_refit.h"

#include "bvh_quantise.h"

namespace ptk {
namespace {

constexpr int kThreads = 256;

// order-preserving encoding of a float as an unsigned integer (the one of bvh_device.hip)
__device__ __forceinline__ uint32_t enc(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__device__ __forceinline__ float half_area(const float* mn, const float* mx)
{
    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    if (!(dx >= 0.0f)) return 0.0f;
    return dx * dy + dy * dz + dz * dx;
}

__global__ __launch_bounds__(kThreads) void inverse_order_kernel(const float4* __restrict__ tris, int32_t* __restrict__ tri_pos, int n)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const int tri = __float_as_int(tris[(size_t)k * TRI_F4 + 2].y);
    if (tri >= 0 && tri < n) tri_pos[tri] = k;
}

__global__ __launch_bounds__(kThreads) void geometry_bounds_kernel(const float* __restrict__ verts, const float* __restrict__ staged, int first, int count, int n,
                                                                   uint32_t* __restrict__ red)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY }, ext = 0.0f;
    uint32_t bad = 0u;
    if (i < n)
    {
        const bool moved = i >= first && i < first + count;
        const float* p = moved ? staged + (size_t)(i - first) * 9 : verts + (size_t)i * 9;
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++)
            {
                const float v = p[k * 3 + a];
                if (!(fabsf(v) < 2.305843e18f)) bad = 1u;          // the bound of ptk_upload_scene: not finite, or 2^61 and beyond
                mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v);
                ext = fmaxf(ext, fabsf(v));
            }
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        for (int a = 0; a < 3; a++) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], off)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off)); }
        ext = fmaxf(ext, __shfl_xor(ext, off));
        bad |= (uint32_t)__shfl_xor((int)bad, off);
    }
    if ((threadIdx.x & 63) != 0) return;
    if (bad) atomicMax(&red[7], 1u);
    if (!(mn[0] <= mx[0])) return;                                  // a wave past the end (or all NaN: the flag is set)
    for (int a = 0; a < 3; a++) { atomicMax(&red[a], ~enc(mn[a])); atomicMax(&red[3 + a], enc(mx[a])); }
    atomicMax(&red[6], __float_as_uint(ext));                       // non-negative floats order as unsigned integers
}

__global__ __launch_bounds__(kThreads) void repack_geometry_kernel(const float* __restrict__ sv, const float* __restrict__ sn, const float* __restrict__ st, int first,
                                                                   int count, float* __restrict__ verts, const int32_t* __restrict__ tri_pos,
                                                                   float4* __restrict__ tris, float4* __restrict__ flat_tris, float4* __restrict__ shade)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= count) return;
    const int i = first + j;
    float v[9];
    for (int k = 0; k < 9; k++) v[k] = sv[(size_t)j * 9 + k];
    float* r = verts + (size_t)i * 9;
    for (int k = 0; k < 9; k++) r[k] = v[k];
    // edge1 = v2 - v1, edge2 = v3 - v1 (pack_tris_kernel); t2.yzw - index, opacity texture, 0 - stay
    const float4 t0 = make_float4(v[0], v[1], v[2], v[3] - v[0]);
    const float4 t1 = make_float4(v[4] - v[1], v[5] - v[2], v[6] - v[0], v[7] - v[1]);
    const float t2x = v[8] - v[2];
    float4* q = tris + (size_t)tri_pos[i] * TRI_F4;
    q[0] = t0; q[1] = t1; reinterpret_cast<float*>(q + 2)[0] = t2x;
    if (flat_tris)
    {
        float4* f = flat_tris + (size_t)i * TRI_F4;
        f[0] = t0; f[1] = t1; reinterpret_cast<float*>(f + 2)[0] = t2x;
    }
    if (!sn) return;
    // s0.xyz, s2.zw, s3 .. s6 (pack_shade_kernel); s0.w - material | smoothing - and the uvs s1, s2.xy stay
    const float* nn = sn + (size_t)j * 9; const float* tb = st + (size_t)j * 9;
    float4* s = shade + (size_t)i * SHADE_F4;
    float* s0 = reinterpret_cast<float*>(s);
    *reinterpret_cast<float2*>(s0) = make_float2(tb[0], tb[1]); s0[2] = tb[2];
    *reinterpret_cast<float2*>(reinterpret_cast<float*>(s + 2) + 2) = make_float2(nn[0], nn[1]);
    s[3] = make_float4(nn[2], nn[3], nn[4], nn[5]);
    s[4] = make_float4(nn[6], nn[7], nn[8], tb[3]);
    s[5] = make_float4(tb[4], tb[5], tb[6], tb[7]);
    s[6] = make_float4(tb[8], 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(64) void repack_lights_kernel(const float* __restrict__ verts, int first, int count, float4* __restrict__ lights, int num_lights)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= num_lights) return;
    float* l = reinterpret_cast<float*>(lights + (size_t)k * LIGHT_F4);
    const int tri = __float_as_int(l[3]);
    if (tri < first || tri >= first + count) return;
    const float* v = verts + (size_t)tri * 9;
    for (int c = 0; c < 3; c++)                                     // l0.xyz, l1.xyz, l2.xyz; the .w words (index, colour) stay
        for (int a = 0; a < 3; a++) l[c * 4 + a] = v[c * 3 + a];
}

__global__ __launch_bounds__(kThreads) void refit_kernel(const int32_t* __restrict__ level_nodes, int count, float4* __restrict__ nodes, const float4* __restrict__ tris,
                                                         const float* __restrict__ verts, float4* __restrict__ side, float pad, int write_nodes)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= count) return;
    const int id = level_nodes[t];
    float4* rec = nodes + (size_t)id * NODE_F4;
    const float4 q1 = rec[1], q2 = rec[2];
    const int32_t link[4] = { __float_as_int(q1.z), __float_as_int(q1.w), __float_as_int(q2.x), __float_as_int(q2.y) };
    int nc = 0;
    while (nc < 4 && link[nc] != NODE_EXIT) nc++;                   // both builders fill the slots from 0 (checked when the levels are made)
    float cmn[4][3], cmx[4][3];
    float area = 0.0f;
    for (int k = 0; k < nc; k++)
    {
        if (link[k] < 0)
        {
            // leaf: the union of its triangles' vertex boxes, padded as the builders pad every triangle box
            const int code = ~link[k], first = code >> 3, cnt = (code & 7) + 1;
            float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (int j = 0; j < cnt; j++)
            {
                const int tri = __float_as_int(tris[(size_t)(first + j) * TRI_F4 + 2].y);
                const float* p = verts + (size_t)tri * 9;
                for (int c = 0; c < 3; c++)
                    for (int a = 0; a < 3; a++) { const float v = p[c * 3 + a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
            }
            for (int a = 0; a < 3; a++) { cmn[k][a] = mn[a] - pad; cmx[k][a] = mx[a] + pad; }
        }
        else
        {
            // interior: the union box its own thread wrote one launch ago (already padded)
            const float4 lo = side[(size_t)link[k] * 2], hi = side[(size_t)link[k] * 2 + 1];
            cmn[k][0] = lo.x; cmn[k][1] = lo.y; cmn[k][2] = lo.z; cmx[k][0] = hi.x; cmx[k][1] = hi.y; cmx[k][2] = hi.z;
        }
        area += half_area(cmn[k], cmx[k]);
    }
    float umn[3], umx[3];
    if (write_nodes) emit_wide_node(cmn, cmx, nc, link, rec, umn, umx);
    else
    {
        for (int a = 0; a < 3; a++) { umn[a] = INFINITY; umx[a] = -INFINITY; }
        for (int k = 0; k < nc; k++)
            for (int a = 0; a < 3; a++) { umn[a] = fminf(umn[a], cmn[k][a]); umx[a] = fmaxf(umx[a], cmx[k][a]); }
    }
    side[(size_t)id * 2] = make_float4(umn[0], umn[1], umn[2], area);
    side[(size_t)id * 2 + 1] = make_float4(umx[0], umx[1], umx[2], 0.0f);
}

// The SAH sum in two passes of fixed order (no float atomics: the result is the same bits every time).  Pass 1: one workgroup per
// 256 consecutive nodes, a lane per node, added pairwise through LDS into one double per workgroup.  Pass 2: one workgroup adds
// the partial sums - lane t takes t, t + 1024, ... so neighbouring lanes read neighbouring doubles - and divides by the root's
// half-area.
__global__ __launch_bounds__(kThreads) void refit_cost_partial_kernel(const float4* __restrict__ side, int num_nodes, double* __restrict__ partial)
{
    __shared__ double s[kThreads];
    const int t = threadIdx.x, i = blockIdx.x * kThreads + t;
    s[t] = i < num_nodes ? (double)side[(size_t)i * 2].w : 0.0;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1)
    {
        if (t < off) s[t] += s[t + off];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(1024) void refit_cost_kernel(const float4* __restrict__ side, const double* __restrict__ partial, int num_partial, double* __restrict__ cost)
{
    __shared__ double s[1024];
    const int t = threadIdx.x;
    double sum = 0.0;
    for (int i = t; i < num_partial; i += 1024) sum += partial[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1)
    {
        if (t < off) s[t] += s[t + off];
        __syncthreads();
    }
    if (t != 0) return;
    const float4 lo = side[0], hi = side[1];
    const float mn[3] = { lo.x, lo.y, lo.z }, mx[3] = { hi.x, hi.y, hi.z };
    cost[0] = s[0] / (double)fmaxf(half_area(mn, mx), 1e-30f);
}

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_inverse_order(const float4* d_tris, int32_t* d_tri_pos, int n, hipStream_t stream)
{
    if (n > 0) hipLaunchKernelGGL(inverse_order_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_tris, d_tri_pos, n);
}
void launch_geometry_bounds(const float* d_verts, const float* d_staged, int first, int count, int n, uint32_t* d_red, hipStream_t stream)
{
    if (n > 0) hipLaunchKernelGGL(geometry_bounds_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_verts, d_staged, first, count, n, d_red);
}
void launch_repack_geometry(const float* d_staged_verts, const float* d_staged_normals, const float* d_staged_tbn, int first, int count,
                            float* d_verts, const int32_t* d_tri_pos, float4* d_tris, float4* d_flat_tris, float4* d_shade, hipStream_t stream)
{
    if (count > 0)
        hipLaunchKernelGGL(repack_geometry_kernel, dim3(blocks_for(count, kThreads)), dim3(kThreads), 0, stream, d_staged_verts, d_staged_normals, d_staged_tbn, first,
                           count, d_verts, d_tri_pos, d_tris, d_flat_tris, d_shade);
}
void launch_repack_lights(const float* d_verts, int first, int count, float4* d_lights, int num_lights, hipStream_t stream)
{
    if (num_lights > 0 && count > 0)
        hipLaunchKernelGGL(repack_lights_kernel, dim3(blocks_for(num_lights, 64)), dim3(64), 0, stream, d_verts, first, count, d_lights, num_lights);
}
void launch_refit_level(const int32_t* d_level_nodes, int count, float4* d_nodes, const float4* d_tris, const float* d_verts, float4* d_side,
                        float pad, int write_nodes, hipStream_t stream)
{
    if (count > 0)
        hipLaunchKernelGGL(refit_kernel, dim3(blocks_for(count, kThreads)), dim3(kThreads), 0, stream, d_level_nodes, count, d_nodes, d_tris, d_verts, d_side, pad, write_nodes);
}
void launch_refit_cost(const float4* d_side, int num_nodes, double* d_partial, double* d_cost, hipStream_t stream)
{
    if (num_nodes <= 0) return;
    const unsigned blocks = blocks_for(num_nodes, kThreads);
    hipLaunchKernelGGL(refit_cost_partial_kernel, dim3(blocks), dim3(kThreads), 0, stream, d_side, num_nodes, d_partial);
    hipLaunchKernelGGL(refit_cost_kernel, dim3(1), dim3(1024), 0, stream, d_side, d_partial, (int)blocks, d_cost);
}

}  // namespace ptk
