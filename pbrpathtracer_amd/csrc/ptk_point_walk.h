// What the point and region queries share (ptk_closest.hip, ptk_knearest.hip, ptk_overlap.hip) on top of the one-wave prologue of
// ptk_query_walk.h (query_group, query_bound): the prune's bound, the decode of a 4-wide quantised node's child boxes, the per-lane
// LDS stack's pop, and the distance-ordered node arm of the two point walks.  Each kernel keeps its own list, triangle arm, bound
// update and epilogue; overlap_kernel keeps its own node arm too (first survivor entered, nothing ordered: another rule).  The box
// arm is acceleration only and uses fused multiply-adds and 1-ulp roots freely, behind the slack derived in DESIGN.md §4.17.
#pragma once
#include "ptk_query_walk.h"
#include "ptk_closest.h"
#ifdef PTK_DEBUG
#include <cassert>
#endif

namespace ptk {

// What box distances and triangle distances can disagree by around a query whose largest |coordinate| is m, in position units
// 
__device__ __forceinline__ float prune_slack(float m, float scene_bound) { return (m + scene_bound) * (PTK_CLOSEST_K * 0x1p-21f); }
__device__ __forceinline__ float prune_slack(const v3 p, float scene_bound)
{
    return prune_slack(fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)), scene_bound);
}

// The squared box distance a child must exceed to be dropped: (sqrt(bound) * (1 + REL) + E)^2, rounded up.  +inf while nothing
// bounds the query; a NaN (a non-finite point) drops nothing.
__device__ __forceinline__ float prune_bound(float bound_d2, float E)
{
    const float thr = __builtin_fmaf(__builtin_amdgcn_sqrtf(bound_d2), 1.0f + PTK_CLOSEST_REL, E);
    return thr * thr * (1.0f + 0x1p-20f);
}

// One 4-wide interior node as the walks read it: origin and scale of its planes, the planes' bytes - child k's in byte k of each
// word - and the four links
struct PointNode { float4 q0, q1; uint32_t lox, loy, loz, hix, hiy, hiz; int link[4]; };
__device__ __forceinline__ PointNode point_node(const float4* nodes, const int node)
{
    const float4* np = (const float4*)((const char*)nodes + (uint32_t)node * (uint32_t)(NODE_F4 * 16));
    const float4 q0 = ldg4(np), q1 = ldg4(np + 1), q2 = ldg4(np + 2), q3 = ldg4(np + 3);
    PointNode N;
    N.q0 = q0; N.q1 = q1;
    N.lox = __float_as_uint(q2.z); N.loy = __float_as_uint(q2.w); N.loz = __float_as_uint(q3.x);
    N.hix = __float_as_uint(q3.y); N.hiy = __float_as_uint(q3.z); N.hiz = __float_as_uint(q3.w);
    N.link[0] = __float_as_int(q1.z); N.link[1] = __float_as_int(q1.w); N.link[2] = __float_as_int(q2.x); N.link[3] = __float_as_int(q2.y);
    return N;
}

// Child k's planes: plane = origin + q * scale.  An empty slot has an inverted box, lo = 255 and hi = 0, which says nothing about
// distance: its link does.
struct ChildBox { float lx, hx, ly, hy, lz, hz; };
__device__ __forceinline__ ChildBox child_box(const PointNode& N, const int k)
{
    ChildBox b;
    b.lx = __builtin_fmaf((float)((N.lox >> (8 * k)) & 255u), N.q0.w, N.q0.x); b.hx = __builtin_fmaf((float)((N.hix >> (8 * k)) & 255u), N.q0.w, N.q0.x);
    b.ly = __builtin_fmaf((float)((N.loy >> (8 * k)) & 255u), N.q1.x, N.q0.y); b.hy = __builtin_fmaf((float)((N.hiy >> (8 * k)) & 255u), N.q1.x, N.q0.y);
    b.lz = __builtin_fmaf((float)((N.loz >> (8 * k)) & 255u), N.q1.y, N.q0.z); b.hz = __builtin_fmaf((float)((N.hiz >> (8 * k)) & 255u), N.q1.y, N.q0.z);
    return b;
}
// ... and its squared distance from p: per axis the distance to the slab, max(lo - p, p - hi, 0)
__device__ __forceinline__ float child_dist2(const PointNode& N, const int k, const v3 p)
{
    const ChildBox b = child_box(N, k);
    const float dx = fmaxf(fmaxf(b.lx - p.x, p.x - b.hx), 0.0f), dy = fmaxf(fmaxf(b.ly - p.y, p.y - b.hy), 0.0f), dz = fmaxf(fmaxf(b.lz - p.z, p.z - b.hz), 0.0f);
    return __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
}

// The next deferred link of the lane's stack, NODE_EXIT when there is none
__device__ __forceinline__ int pop_link(const int* stack, int*& top)
{
    if (top == stack) return NODE_EXIT;
    top -= PTK_QUERY_BLOCK;
    return *top;
}
// (make EXTRA=-DPTK_DEBUG: DESIGN.md §4.17) the pushes of one node stayed inside the rows
__device__ __forceinline__ void check_stack(const int* stack, const int* top)
{
#ifdef PTK_DEBUG
    assert(top - stack <= (PTK_STACK_ROWS - 1) * PTK_QUERY_BLOCK);
#endif
}

// The distance-ordered node arm: the children of `node` whose box lies within thr2 of p, the nearest entered - its link is
// returned - and the others deferred; with no survivor the next deferred link.  The order key is the squared box distance (>= 0,
// so its bits order as integers) with the slot in its low bits.  A child is dropped only when db2 > thr2: a box at exactly the
// bound may hold an equal distance with a smaller index
// (a non-finite point can give db2 the bits 0x7fffffff, in slot 3 the key of "no survivor": that child is then neither entered
// nor deferred - such a point's output is unspecified, and the walk still ends)
__device__ __forceinline__ int ordered_node_arm(const float4* nodes, const int node, const v3 p, const float thr2, const int* stack, int*& top)
{
    const PointNode N = point_node(nodes, node);
    int key[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const float db2 = child_dist2(N, k, p);
        in[k] = (N.link[k] != NODE_EXIT) & !(db2 > thr2);
        key[k] = in[k] ? ((__float_as_int(db2) & ~3) | k) : 0x7fffffff;
    }
    const int kmin = min(min(key[0], key[1]), min(key[2], key[3]));
    const bool o0 = key[0] != kmin, o1 = key[1] != kmin, o2 = key[2] != kmin, o3 = key[3] != kmin;
    int next = !o0 ? N.link[0] : (!o1 ? N.link[1] : (!o2 ? N.link[2] : N.link[3]));
    // walk_step's pushes: every link is written at the running top, which moves on only behind a link that stays - at most
    // three per node, the nearest survivor being descended into: the discipline the builders' stack_need counts
    *top = N.link[0]; top += (in[0] & o0) ? PTK_QUERY_BLOCK : 0;
    *top = N.link[1]; top += (in[1] & o1) ? PTK_QUERY_BLOCK : 0;
    *top = N.link[2]; top += (in[2] & o2) ? PTK_QUERY_BLOCK : 0;
    *top = N.link[3]; top += (in[3] & o3) ? PTK_QUERY_BLOCK : 0;
    check_stack(stack, top);
    if (kmin == 0x7fffffff) next = pop_link(stack, top);
    return next;
}

}  // namespace ptk
