// HIP kernel for gfx950 of surface attribute queries (include/ptk.h ptk_surface_attributes): what is AT the surface
// points (triangle, u, v) every other query answers with - material, texture coordinate, position, face and shading normal, diffuse
// colour, emission, gloss, opacity texel.  No BVH, no random draw, no state of the render: a gather of the triangle's records and
// the shading operations of ptk_surface_attrs.h, the function features_kernel calls for a pixel's camera ray.  Compiled once, with
// -ffp-contract=off: the float operations are the rule of ptk.h one by one (the numpy restatement is tests/surface_attr_rule.py).
#include "ptk_device_fn.h"
#include "ptk_attributes.h"
#include "ptk_surface_attrs.h"

namespace ptk {

#define PTK_ATTR_BLOCK 256

__device__ __forceinline__ void store3(float* base, size_t i, v3 a) { float* o = base + i * 3; o[0] = a.x; o[1] = a.y; o[2] = a.z; }

// One query per lane.  tri (4 B) and bary (8 B, one float2) are read coalesced.  dirs has 12 B per lane and is read where it lies:
// a wave's 64 directions are 768 consecutive bytes, every byte of every line it touches is used, and dealing the workgroup's floats
// through LDS the way stage_rows does for the ray queries - three coalesced loads, a barrier, three LDS reads - did not win where
// it was measured (tools/experiments/attributes_stage_dirs.patch).  Which outputs are computed is a
// matter of the kernel arguments - uniform branches -, and so is which records are read: s0 alone for MATERIAL and NORMAL_GEOM, the
// vertices for POSITION, the material record and texels only for 4..8.  A miss - a triangle index outside [0, num_tris) - reads no
// scene memory.  Outputs are stored by their own lane (the LDS transposition of 12-byte outputs lost in surface_sample_kernel:
// tools/experiments/surface_deal.patch).
__global__ __launch_bounds__(PTK_ATTR_BLOCK) void attributes_kernel(const AttributeParams P)
{
    const uint32_t i = blockIdx.x * (uint32_t)PTK_ATTR_BLOCK + threadIdx.x;         // < 2^31 + 255
    if (i >= (uint32_t)P.num) return;
    const bool flip = P.dirs != nullptr;
    const uint32_t want = (P.material ? SA_MATERIAL : 0u) | (P.uv ? SA_UV : 0u) | (P.position ? SA_POSITION : 0u) |
                          (P.normal_geom ? SA_NORMAL_GEOM : 0u) | (P.normal ? SA_NORMAL : 0u) | (P.albedo ? SA_ALBEDO : 0u) |
                          (P.emission ? SA_EMISSION : 0u) | (P.gloss ? SA_GLOSS : 0u) | (P.opacity ? SA_OPACITY : 0u);
    v3 rd = V(0.0f, 0.0f, 0.0f);
    if (flip && (want & SA_NORMAL))
    {
        const float* d = P.dirs + (size_t)i * 3;
        rd = V(d[0], d[1], d[2]);
    }
    const int tri = P.tri[i];
    const float2 b = *reinterpret_cast<const float2*>(P.bary + (size_t)i * 2);      // (8-byte aligned: ptk.h)
    const float u = b.x, v = b.y;
    SurfaceAttrs A;
    A.material = -1;
    A.uvx = A.uvy = 0.0f;
    A.ng = A.n = A.albedo = A.emission = V(0.0f, 0.0f, 0.0f);
    A.roughness = A.reflectiveness = A.opacity = 0.0f;
    v3 pos = V(0.0f, 0.0f, 0.0f);
    if ((uint32_t)tri < (uint32_t)P.num_tris)
    {
        if (want & ~SA_POSITION) surface_attrs(P, tri, u, v, flip, rd, want, A);
        if (want & SA_POSITION)
        {
            const float* q = P.verts + (size_t)tri * 9;
            const v3 v1 = V(q[0], q[1], q[2]), v2 = V(q[3], q[4], q[5]), v3_ = V(q[6], q[7], q[8]);
            const float w = 1.0f - u - v;
            pos = add(add(muls(v1, w), muls(v2, u)), muls(v3_, v));
        }
    }
    if (P.material) P.material[i] = A.material;
    if (P.uv) *reinterpret_cast<float2*>(P.uv + (size_t)i * 2) = make_float2(A.uvx, A.uvy);
    if (P.position) store3(P.position, i, pos);
    if (P.normal_geom) store3(P.normal_geom, i, A.ng);
    if (P.normal) store3(P.normal, i, A.n);
    if (P.albedo) store3(P.albedo, i, A.albedo);
    if (P.emission) store3(P.emission, i, A.emission);
    if (P.gloss) *reinterpret_cast<float2*>(P.gloss + (size_t)i * 2) = make_float2(A.roughness, A.reflectiveness);
    if (P.opacity) P.opacity[i] = A.opacity;
}

void launch_attributes(const AttributeParams& p, hipStream_t stream)
{
    if (p.num <= 0) return;
    const dim3 grid((unsigned)(((size_t)p.num + PTK_ATTR_BLOCK - 1) / PTK_ATTR_BLOCK)), block(PTK_ATTR_BLOCK);
    hipLaunchKernelGGL(attributes_kernel, grid, block, 0, stream, p);
}

}  // namespace ptk
