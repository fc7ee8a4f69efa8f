// What the one-wave ray queries share (ptk_hits.hip, ptk_crossings.hip, ptk_multihit.hip): one-wave workgroups, one query per lane,
// the group's origins and directions staged through the stack rows of LDS, and each lane's walk to its end - the walk of
// rays_kernel (ptk_rays.hip) with everything but the walk taken out: the per-lane LDS stack of links, one node record in flight
// across iterations, the triangle arm voted by the wave.  The step is walk_step_with (ptk_device_fn.h); a query kind is its
// triangle arm.  The point and region queries (ptk_closest.hip, ptk_knearest.hip, ptk_overlap.hip) have the prologue from here -
// query_group, query_bound - and walks of another kind from ptk_point_walk.h (DESIGN.md §4.24 "The walk").
#pragma once
#include "ptk_device_fn.h"

namespace ptk {

#define PTK_QUERY_BLOCK 64          // one wave per workgroup, one query per lane

// what the step reads of the launch parameters, held in SGPRs for the length of the loop (WalkParams without the shading tables)
struct QueryWalkParams { const float4* nodes; const float4* tris; int tri_thr; };
template <class PT>
__device__ __forceinline__ QueryWalkParams query_walk_params(const PT& H)
{
    QueryWalkParams WP;
    WP.nodes = uniform_ptr(H.nodes); WP.tris = uniform_ptr(H.tris);
    WP.tri_thr = __builtin_amdgcn_readfirstlane(H.tri_thr);
    return WP;
}

// The group's 3 n consecutive floats of `origins` into rows [0, 3) of the stack and, with DIRS, those of `dirs` into rows [3, 6):
// consecutive lanes read consecutive floats (three instructions per array instead of three of stride 12 B).  One pass over both
// arrays, as hits_kernel's own text had it: a pass each costs hits_kernel 48 instructions more (three more predicated regions, and
// no paired LDS stores).  crossings_kernel and multihit_kernel staged a pass per array before they came here, so this changed
// their prologues too (the crossings unit: 1131 -> 1098 instructions); that choice was made on instruction counts, and what was
// timed is the whole kernel against its predecessor, not the two staging forms against each other.
template <bool DIRS>
__device__ __forceinline__ void stage_rows(float* stage, uint32_t first, uint32_t n, const float* origins, const float* dirs)
{
    const uint32_t lane = threadIdx.x;
    const float* const go = origins + (size_t)first * 3, * const gd = DIRS ? dirs + (size_t)first * 3 : nullptr;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
    {
        const uint32_t e = lane + k * PTK_QUERY_BLOCK;
        if (e < n * 3u)
        {
            stage[e] = go[e];
            if (DIRS) stage[3 * PTK_QUERY_BLOCK + e] = gd[e];
        }
    }
}

// The queries of the workgroup: 64 consecutive ones from `first`, fewer (n) in the last group; the lane's is i, if it has one (live)
struct QueryGroup { uint32_t first, n, i; bool live; };

// The group and its lanes' origins and, with DIRS, directions (3 floats per query in `origins` and `dirs`), which come through
// the rows of the stack the walk does not use yet.  A lane without a query gets the origin 0 and the direction +z.
template <bool DIRS = false>
__device__ __forceinline__ QueryGroup query_group(int* lds_stack, const int num, const float* origins, v3& ro, const float* dirs = nullptr, v3* rd = nullptr)
{
    static_assert(PTK_STACK_ROWS >= (DIRS ? 6 : 3), "the staging area is three rows of the stack per array");
    const uint32_t lane = threadIdx.x;
    QueryGroup G;
    G.first = blockIdx.x * (uint32_t)PTK_QUERY_BLOCK;                               // < num <= 2^31 - 1
    G.n = min((uint32_t)PTK_QUERY_BLOCK, (uint32_t)num - G.first);
    G.live = lane < G.n;
    G.i = G.first + lane;
    float* const stage = (float*)lds_stack;
    stage_rows<DIRS>(stage, G.first, G.n, origins, dirs);
    __syncthreads();
    // (stride 3 dwords: no two lanes of a half-wave on one bank)
    ro = G.live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    if (DIRS)
        *rd = G.live ? V(stage[3 * PTK_QUERY_BLOCK + lane * 3], stage[3 * PTK_QUERY_BLOCK + lane * 3 + 1], stage[3 * PTK_QUERY_BLOCK + lane * 3 + 2])
                     : V(0.0f, 0.0f, 1.0f);
    __syncthreads();                                                                // the rows are the stack from here on
    return G;
}

// The lane's bound, +inf without an array of them, and whether the lane walks at all: a NaN, zero or negative bound admits nothing
__device__ __forceinline__ bool query_bound(const QueryGroup& G, const float* bounds, float& tmax)
{
    tmax = __builtin_inff();
    if (G.live && bounds) tmax = bounds[G.i];
    return G.live & (tmax > 0.0f);
}

// Every lane's walk, begun (Walk::begin) by the caller, to its end; tri is walk_step_with's triangle arm
template <class PT, class TRI>
__device__ __forceinline__ void query_walk(const PT& WP, Walk& W, int* stack, TRI tri)
{
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };           // (the step's; no STATS: never touched.  An arm that needs one, as tri_test does in hits_walk, brings its own)
    NodeRec nrec;
    request_node(WP, W, nrec);                                                      // one node record in flight across iterations (walk_step_with)
    while (__ballot(!W.done()))
    {
        // rays_kernel's vote: the triangle arm runs when enough lanes have triangles queued, and always when no lane has a node
        const int n_tq = __popcll(__ballot(W.tri_left > 0)), n_nr = __popcll(__ballot(W.node >= 0));
        const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));
        if (!W.done()) walk_step_with<false, PTK_QUERY_BLOCK, true>(WP, W, stack, cnt, run_tri_arm, &nrec, tri);
    }
}

}  // namespace ptk
