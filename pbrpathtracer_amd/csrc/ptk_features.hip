// HIP kernels for gfx950 of the first-hit feature planes and of picking (include/ptk.h ptk_render_features, ptk_pick).
// They are built from the trace kernels' own device functions (ptk_device_fn.h: the exact normalize, tex2d, Walk, tri_test,
// walk_step, the RNG keys) and compiled once, with -ffp-contract=off like the exact build, so every operation below is the IEEE
// operation of the exact trace kernel.
#include "ptk_device_fn.h"
#include "ptk_features.h"
#include "ptk_surface_attrs.h"

namespace ptk {

// the feature ray of pixel `pix` (top-down index): the camera-ray block at zero lens offset
template <class PT>
__device__ __forceinline__ v3 feature_ray(const PT& P, v3 ro, size_t pix)
{
    const float4 d = P.primary[pix];
    return normalize(sub(add(ro, muls(V(d.x, d.y, d.z), P.focal_dist)), ro));
}

// ... and its closest accepted hit: a walk whose opacity draws are keyed as the trace kernel keys ray 0 of (seed, pixel, sample)
template <class PT>
__device__ __forceinline__ Hit feature_walk(const PT& P, const FeatureParams& F, v3 ro, v3 rd, size_t pix, int* stack)
{
    Rng rng; rng.inc = 1u; rng.state = 0u;                                 // (no draws from the stream: only the key counts)
    rng.key = hash32(F.sample + pixel_key(F.seed_lo, F.seed_hi, (uint32_t)pix));
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    Walk W;
    W.occl_tri = -1;
    W.begin(ro, rd, P.num_nodes, stack, P.scene_bound);
    while (!W.done()) walk_step<false, PTK_BLOCK>(P, W, rng, 0u, stack, cnt);
    return W.best;
}

// First-hit feature planes (include/ptk.h ptk_render_features): per owned pixel the closest accepted hit of its camera ray with the
// lens closed, and the surface quantities shade_interaction computes at that interaction - the same IEEE operations in the same
// order, on the records of the accepted hit only.  One workgroup per owned 16x16 tile, one wave per 8x8 quadrant
// (accumulate_kernel's pixel mapping: a wave's 64 rays are one coherent bundle).  The hit comes from the primary-hit cache where
// that is valid (the same walk of the same ray, done once), otherwise from a walk whose opacity draws are keyed as the trace
// kernel keys ray 0 of (seed, pixel, sample).  Only planes with a non-null pointer are computed and stored (kernel arguments:
// uniform branches); a pixel's element is 4, 8 or 12 bytes, stored by its own lane.
__global__ __launch_bounds__(PTK_BLOCK) void features_kernel(const RenderParams P, const FeatureParams F)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, quad = tid >> 6;
    const int tile = blockIdx.x * P.world + P.rank;
    if (tile >= P.num_tiles) return;
    int tx, ty, px, py; tile_origin(tile, P.tiles_x, tx, ty);
    quadrant_pixel(tx, ty, quad, lane, px, py);
    if (px >= P.width || py >= P.height) return;
    const size_t pix = (size_t)py * P.width + px;                          // top-down: primary, primary_hit, the RNG's pixel
    const size_t o = (size_t)(P.height - 1 - py) * P.width + px;           // bottom-up, like the accumulator
    const v3 ro = V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    v3 rd;
    Hit h;
    if (P.primary_hit)
    {
        const float4 c = P.primary_hit[pix], r = P.primary_rd[pix];
        rd = V(r.x, r.y, r.z);
        h.tri = __float_as_int(c.x); h.t = c.y; h.u = c.z; h.v = c.w;
    }
    else
    {
        rd = feature_ray(P, ro, pix);
        h = feature_walk(P, F, ro, rd, pix, lds_stack + tid);
    }
    const bool hit = h.tri != PTK_NOHIT;
    if (F.depth) F.depth[o] = hit ? h.t : __builtin_inff();
    if (F.triangle) F.triangle[o] = hit ? h.tri : -1;
    if (F.bary) *(float2*)(F.bary + o * 2) = hit ? make_float2(h.u, h.v) : make_float2(0.0f, 0.0f);
    if (F.position)
    {
        const v3 p = hit ? add(ro, muls(rd, h.t)) : V(0.0f, 0.0f, 0.0f);   // :553, before the offset of :569
        F.position[o * 3] = p.x; F.position[o * 3 + 1] = p.y; F.position[o * 3 + 2] = p.z;
    }
    if (!(F.material || F.normal_geom || F.normal || F.albedo || F.emission || F.gloss)) return;
    // the surface quantities: the one statement of them (ptk_surface_attrs.h), shared with attributes_kernel
    const uint32_t want = (F.material ? SA_MATERIAL : 0u) | (F.normal_geom ? SA_NORMAL_GEOM : 0u) | (F.normal ? SA_NORMAL : 0u) |
                          (F.albedo ? SA_ALBEDO : 0u) | (F.emission ? SA_EMISSION : 0u) | (F.gloss ? SA_GLOSS : 0u);
    SurfaceAttrs A;
    A.material = -1;
    A.ng = A.n = A.albedo = A.emission = V(0.0f, 0.0f, 0.0f);
    A.roughness = A.reflectiveness = 0.0f;
    if (hit) surface_attrs(P, h.tri, h.u, h.v, true, rd, want, A);
    const int matid = A.material;
    const v3 ng = A.ng, n = A.n, albedo = A.albedo, emission = A.emission;
    const float roughness = A.roughness, reflectiveness = A.reflectiveness;
    if (F.material) F.material[o] = matid;
    if (F.normal_geom) { F.normal_geom[o * 3] = ng.x; F.normal_geom[o * 3 + 1] = ng.y; F.normal_geom[o * 3 + 2] = ng.z; }
    if (F.normal) { F.normal[o * 3] = n.x; F.normal[o * 3 + 1] = n.y; F.normal[o * 3 + 2] = n.z; }
    if (F.albedo) { F.albedo[o * 3] = albedo.x; F.albedo[o * 3 + 1] = albedo.y; F.albedo[o * 3 + 2] = albedo.z; }
    if (F.emission) { F.emission[o * 3] = emission.x; F.emission[o * 3 + 1] = emission.y; F.emission[o * 3 + 2] = emission.z; }
    if (F.gloss) *(float2*)(F.gloss + o * 2) = make_float2(roughness, reflectiveness);
}

// ptk_pick: the feature ray of ONE pixel - one lane of one workgroup (the stack layout is that of a whole workgroup)
__global__ __launch_bounds__(PTK_BLOCK) void pick_kernel(const RenderParams P, const FeatureParams F, int pixel, int32_t* out3)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_BLOCK];
    if (threadIdx.x != 0) return;
    const v3 ro = V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    const v3 rd = feature_ray(P, ro, (size_t)pixel);
    const Hit h = feature_walk(P, F, ro, rd, (size_t)pixel, lds_stack);
    const bool hit = h.tri != PTK_NOHIT;
    out3[0] = hit ? h.tri : -1;
    out3[1] = hit ? (__float_as_int(ldg4(P.shade + (size_t)h.tri * SHADE_F4).w) & 0x7fffffff) : -1;
    out3[2] = __float_as_int(hit ? h.t : __builtin_inff());
}

void launch_features(const RenderParams& p, const FeatureParams& f, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles > 0) hipLaunchKernelGGL(features_kernel, dim3(owned_tiles), dim3(PTK_BLOCK), 0, stream, p, f);
}
void launch_pick(const RenderParams& p, const FeatureParams& f, int pixel, int32_t* out3, hipStream_t stream)
{
    hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(PTK_BLOCK), 0, stream, p, f, pixel, out3);
}

}  // namespace ptk
