// HIP kernel for gfx950 of closest-point queries (include/ptk.h ptk_closest_points): for every caller point the nearest point of the
// scene's surface.  The shape is hits_kernel's (ptk_hits.hip) - one-wave workgroups, one query per lane, the points staged through
// LDS (query_group, ptk_query_walk.h), the per-lane LDS stack of links - around a walk of its own: a distance-ordered,
// distance-pruned descent of the 4-wide quantised BVH, whose node arm and bound nearest_kernel shares (ptk_point_walk.h).  Compiled
// once, with -ffp-contract=off: the triangle arm is the rule of ptk.h operation by operation (closest_rule, ptk_closest_rule.h; the
// numpy restatement is tests/closest_rule.py); the box arm is acceleration only, behind the slack derived in DESIGN.md §4.17.
#include "ptk_point_walk.h"
#include "ptk_closest_rule.h"

namespace ptk {

struct Closest { float d2; int tri; float v, w, qx, qy, qz; };

// The rule of ptk.h for one 48-byte record (closest_rule), then the accept against the best so far: a strict bound, a tie to the
// smaller index (best.tri = -1 while nothing is accepted: the tie arm cannot fire on the seed, so the bound is strict).
__device__ __forceinline__ void closest_tri(const v3 p, const float4 t0, const float4 t1, const float4 t2, Closest& best)
{
    const ClosestRule r = closest_rule(p, t0, t1, t2);
    const int tri = __float_as_int(t2.y);
    const bool ok = (r.d2k < best.d2) | ((r.d2k == best.d2) & (tri < best.tri));
    best.d2 = ok ? r.d2k : best.d2; best.tri = ok ? tri : best.tri;
    best.v = ok ? r.v : best.v; best.w = ok ? r.w : best.w;
    best.qx = ok ? r.q.x : best.qx; best.qy = ok ? r.q.y : best.qy; best.qz = ok ? r.q.z : best.qz;
}

template <bool STATS>
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void closest_kernel(const ClosestParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    const uint32_t lane = threadIdx.x;
    int* const stack = lds_stack + lane;
    float* const stage = (float*)lds_stack;
    v3 p;
    const QueryGroup G = query_group(lds_stack, H.num_points, H.points, p);
    float md;
    const bool walks = query_bound(G, H.max_dist, md);                              // a NaN, zero or negative radius accepts nothing
    Closest best;
    best.d2 = md * md; best.tri = -1; best.v = 0.0f; best.w = 0.0f; best.qx = 0.0f; best.qy = 0.0f; best.qz = 0.0f;
    const float E = prune_slack(p, H.scene_bound);
    float thr2 = prune_bound(best.d2, E);

    const float4* const nodes = uniform_ptr(H.nodes);
    const float4* const tris = uniform_ptr(H.tris);
    int node = walks ? 0 : NODE_EXIT;
    int* top = stack;
    uint32_t n_nodes = 0, n_tris = 0;
    while (__ballot(node != NODE_EXIT))
    {
        if (node >= 0)                                        // ---- one 4-wide interior node
        {
            if (STATS) n_nodes++;
            node = ordered_node_arm(nodes, node, p, thr2, stack, top);
        }
        else if (node != NODE_EXIT)                           // ---- a leaf: its 1 .. 8 records, then the next deferred link
        {
            const int code = ~node;
            const uint32_t first = (uint32_t)(code >> 3), count = (uint32_t)(code & 7) + 1u;
            const float before = best.d2;
            const int before_tri = best.tri;
            for (uint32_t k = 0; k < count; k++)
            {
                const float4* tp = (const float4*)((const char*)tris + (first + k) * (uint32_t)(TRI_F4 * 16));
                const float4 t0 = ldg4(tp), t1 = ldg4(tp + 1), t2 = ldg4(tp + 2);
                closest_tri(p, t0, t1, t2, best);
            }
            if (STATS) n_tris += count;
            if ((best.d2 != before) | (best.tri != before_tri)) thr2 = prune_bound(best.d2, E);
            node = pop_link(stack, top);
        }
    }
    __syncthreads();                                                                // every lane's stack is done: the rows stage the outputs

    const bool hit = best.tri >= 0;
    if (H.tri && G.live) H.tri[G.i] = hit ? best.tri : -1;
    if (H.dist && G.live) H.dist[G.i] = hit ? sqrt_ieee(best.d2) : __builtin_inff();
    if (H.point)
    {
        stage[lane * 3] = hit ? best.qx : 0.0f; stage[lane * 3 + 1] = hit ? best.qy : 0.0f; stage[lane * 3 + 2] = hit ? best.qz : 0.0f;
        __syncthreads();
        float* const gq = H.point + (size_t)G.first * 3;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t e = lane + k * PTK_QUERY_BLOCK;
            if (e < G.n * 3u) gq[e] = stage[e];
        }
        __syncthreads();
    }
    if (H.bary)
    {
        stage[lane * 2] = hit ? best.v : 0.0f; stage[lane * 2 + 1] = hit ? best.w : 0.0f;
        __syncthreads();
        float* const gb = H.bary + (size_t)G.first * 2;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++)
        {
            const uint32_t e = lane + k * PTK_QUERY_BLOCK;
            if (e < G.n * 2u) gb[e] = stage[e];
        }
    }
    if (STATS)
    {
        atomicAdd(H.stats, (unsigned long long)n_nodes);
        atomicAdd(H.stats + 1, (unsigned long long)n_tris);
    }
}

void launch_closest(const ClosestParams& h, hipStream_t stream)
{
    if (h.num_points <= 0 || h.num_nodes <= 0) return;
    const dim3 grid((unsigned)(((size_t)h.num_points + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK));
    if (h.stats) hipLaunchKernelGGL(closest_kernel<true>, grid, dim3(PTK_QUERY_BLOCK), 0, stream, h);
    else hipLaunchKernelGGL(closest_kernel<false>, grid, dim3(PTK_QUERY_BLOCK), 0, stream, h);
}

}  // namespace ptk
