// HIP kernels for gfx950 of crossing counts and point containment (include/ptk.h ptk_crossings_rays, ptk_contains_points,
// ptk_signed_distance).  The shape and the walk are the one-wave ray queries' (ptk_query_walk.h: one-wave
// workgroups, one query per lane, origins and directions staged through the stack rows of LDS, query_walk over walk_step_with of
// ptk_device_fn.h) with a triangle arm that COUNTS every triangle the ray crosses instead of keeping the nearest.  Nothing tightens:
// W.best.t is the ray's tmax from begin to end, the node arm culls against it as the occlusion walk does against its bound, and no
// triangle ends a walk.  Compiled once, with -ffp-contract=off: the triangle arm is tri_test's Moeller-Trumbore (mt_auvt, the same
// function; the numpy restatement is tests/crossings_rule.py); the node arm is acceleration only.
#include "ptk_query_walk.h"
#include "ptk_crossings.h"
#include "ptk.h"

namespace ptk {

// The rule of ptk.h for one 48-byte record: tri_test's a, u, v, t and its tests with the ray's bound in the place of the closest
// hit; no opacity, no tie rule, nothing kept but the two counts.
__device__ __forceinline__ void cross_tri(const Walk& W, const float4 t0, const float4 t1, const float4 t2, int& front, int& back)
{
    float a, u, v, t;
    mt_auvt(W.ro, W.rd, t0, t1, t2, a, u, v, t);
    const bool ok = !(fabsf(a) < PTK_EPS) & !(u < 0.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t > PTK_EPS) & (t < W.best.t);
    front += (ok & (a > 0.0f)) ? 1 : 0;
    back += (ok & (a < 0.0f)) ? 1 : 0;
}

// Every lane's walk of the ray (o, d) bounded by tmax to its end (walks false: the lane has no ray, or a bound that admits nothing);
// front and back are added to.  The arm never stops the walk, so every record of every leaf it reaches is tested exactly once.
__device__ __forceinline__ void cross_walk(const QueryWalkParams& WP, const CrossingsParams& H, int* stack, const v3 o, const v3 d, const float tmax,
                                           const bool walks, int& front, int& back)
{
    Walk W;
    W.occl_tri = -1;
    W.begin(o, d, walks ? H.num_nodes : 0, stack, H.scene_bound);                   // (no nodes: done at once)
    W.best.t = tmax;
    query_walk(WP, W, stack, [&](const float4 t0, const float4 t1, const float4 t2, uint32_t) {
        cross_tri(W, t0, t1, t2, front, back);
        return false;
    });
}

// front / back of every ray
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void crossings_kernel(const CrossingsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    v3 ro, rd;
    const QueryGroup G = query_group<true>(lds_stack, H.num, H.origins, ro, H.dirs, &rd);
    float tmax;
    const bool walks = query_bound(G, H.tmax, tmax);
    int front = 0, back = 0;
    cross_walk(query_walk_params(H), H, lds_stack + threadIdx.x, ro, rd, tmax, walks, front, back);
    if (H.front && G.live) H.front[G.i] = front;
    if (H.back && G.live) H.back[G.i] = back;
}

// the built-in direction set of ptk_contains_points (ptk.h)
__constant__ float k_inside_dirs[9] = PTK_INSIDE_DEFAULT_DIRS;

// inside / winding of every point; the sign of dist.  The directions are wave-uniform: all lanes walk direction j at the same time
// (a coherent walk: the lanes' rays are parallel and their origins neighbours), each direction a walk begun afresh on the same
// stack column - empty again when a walk has ended - and the vote is kept in a register, so the kernel needs no memory of its own.
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void contains_kernel(const CrossingsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    const uint32_t lane = threadIdx.x;
    v3 p;
    const QueryGroup G = query_group(lds_stack, H.num, H.origins, p);
    const bool live = G.live;
    const uint32_t i = G.i;
    const QueryWalkParams WP = query_walk_params(H);
    const float* const dirs = H.dirs ? H.dirs : (const float*)k_inside_dirs;
    const int D = __builtin_amdgcn_readfirstlane(H.num_dirs);
    int count = 0;
    for (int j = 0; j < D; j++)
    {
        const v3 d = V(dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]);
        int front = 0, back = 0;
        cross_walk(WP, H, lds_stack + lane, p, d, __builtin_inff(), live, front, back);
        const bool vote = H.mode == PTK_INSIDE_PARITY ? (((front + back) & 1) != 0) : (back != front);
        count += vote ? 1 : 0;
        if (H.winding && live) H.winding[(size_t)i * (uint32_t)D + (uint32_t)j] = back - front;
    }
    const bool inside = 2 * count > D;
    if (H.inside && live) H.inside[i] = inside ? 1 : 0;
    if (H.dist && live && inside) H.dist[i] = __uint_as_float(__float_as_uint(H.dist[i]) | 0x80000000u);
}

static dim3 cross_grid(const CrossingsParams& h) { return dim3((unsigned)(((size_t)h.num + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK)); }

void launch_crossings(const CrossingsParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(crossings_kernel, cross_grid(h), dim3(PTK_QUERY_BLOCK), 0, stream, h);
}

void launch_contains(const CrossingsParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(contains_kernel, cross_grid(h), dim3(PTK_QUERY_BLOCK), 0, stream, h);
}

}  // namespace ptk
