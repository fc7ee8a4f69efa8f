// HIP kernel for gfx950 of closest-point queries (include/ptk.h ptk_closest_points): for every caller point the nearest point of the
// scene's surface.  The shape is hits_kernel's (ptk_hits.hip) - one-wave workgroups, one query per lane, the points staged through
// LDS, the per-lane LDS stack of links - around a walk of its own: a distance-ordered, distance-pruned descent of the 4-wide
// quantised BVH.  Compiled once, with -ffp-contract=off: the triangle arm is the rule of ptk.h operation by operation (the numpy
// restatement is tests/closest_rule.py); the box arm is acceleration only and uses fused multiply-adds and 1-ulp roots freely,
// behind the slack derived in DESIGN.md §4.17.
#include "ptk_device_fn.h"
#include "ptk_closest.h"
#ifdef PTK_DEBUG
#include <cassert>
#endif

namespace ptk {

#define PTK_CLOSEST_BLOCK 64        // one wave per workgroup, one query per lane

struct Closest { float d2; int tri; float v, w, qx, qy, qz; };

// The rule of ptk.h for one 48-byte record: Ericson's regions with the final clamp, then the strict bound / tie arm against the
// best so far (best.tri = -1 while nothing is accepted: the tie arm cannot fire on the seed, so the bound is strict).
__device__ __forceinline__ void closest_tri(const v3 p, const float4 t0, const float4 t1, const float4 t2, Closest& best)
{
    const v3 a = V(t0.x, t0.y, t0.z), e1 = V(t0.w, t1.x, t1.y), e2 = V(t1.z, t1.w, t2.x);
    const int tri = __float_as_int(t2.y);
    const v3 ap = sub(p, a), bp = sub(ap, e1), cp = sub(ap, e2);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap), d3 = dot(e1, bp), d4 = dot(e2, bp), d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    const bool r0 = (d1 <= 0.0f) & (d2 <= 0.0f);
    const bool r1 = (d3 >= 0.0f) & (d4 <= d3);
    const bool r3 = (vc <= 0.0f) & (d1 >= 0.0f) & (d3 <= 0.0f);
    const bool r2 = (d6 >= 0.0f) & (d5 <= d6);
    const bool r4 = (vb <= 0.0f) & (d2 >= 0.0f) & (d6 <= 0.0f);
    const bool r5 = (va <= 0.0f) & (e43 >= 0.0f) & (e56 >= 0.0f);
    const int reg = r0 ? 0 : (r1 ? 1 : (r3 ? 3 : (r2 ? 2 : (r4 ? 4 : (r5 ? 5 : 7)))));
    // two IEEE divisions serve every region: A = v of the edge 1-2 / the face, B = w of the edges 1-3, 2-3 / the face
    const float den = (va + vb) + vc;
    const bool useA = (reg == 3) | (reg == 7), useB = reg >= 4;
    const float numA = reg == 3 ? d1 : vb, denA = reg == 3 ? d1 - d3 : den;
    const float numB = reg == 4 ? d2 : (reg == 5 ? e43 : vc), denB = reg == 4 ? d2 - d6 : (reg == 5 ? e43 + e56 : den);
    const float A = (useA ? numA : 0.0f) / (useA ? denA : 1.0f), B = (useB ? numB : 0.0f) / (useB ? denB : 1.0f);
    float v = reg == 1 ? 1.0f : (reg == 5 ? 1.0f - B : (useA ? A : 0.0f));
    float w = reg == 2 ? 1.0f : (useB ? B : 0.0f);
    v = v > 0.0f ? v : 0.0f;                 // (a NaN becomes 0)
    v = v < 1.0f ? v : 1.0f;
    w = w > 0.0f ? w : 0.0f;
    const float top = 1.0f - v;
    w = w < top ? w : top;
    const v3 q = V((a.x + e1.x * v) + e2.x * w, (a.y + e1.y * v) + e2.y * w, (a.z + e1.z * v) + e2.z * w);
    const v3 d = sub(p, q);
    const float dd = dot(d, d);
    const bool ok = (dd < best.d2) | ((dd == best.d2) & (tri < best.tri));
    best.d2 = ok ? dd : best.d2; best.tri = ok ? tri : best.tri;
    best.v = ok ? v : best.v; best.w = ok ? w : best.w;
    best.qx = ok ? q.x : best.qx; best.qy = ok ? q.y : best.qy; best.qz = ok ? q.z : best.qz;
}

// The squared box distance a child must exceed to be dropped: (sqrt(best) * (1 + REL) + E)^2, rounded up.  +inf while nothing
// bounds the query; a NaN (a non-finite point) drops nothing.
__device__ __forceinline__ float prune_bound(float best_d2, float E)
{
    const float thr = __builtin_fmaf(__builtin_amdgcn_sqrtf(best_d2), 1.0f + PTK_CLOSEST_REL, E);
    return thr * thr * (1.0f + 0x1p-20f);
}

template <bool STATS>
__global__ __launch_bounds__(PTK_CLOSEST_BLOCK) void closest_kernel(const ClosestParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_CLOSEST_BLOCK];
    const uint32_t lane = threadIdx.x;
    const uint32_t p0 = blockIdx.x * (uint32_t)PTK_CLOSEST_BLOCK;                   // < num_points <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_CLOSEST_BLOCK, (uint32_t)H.num_points - p0);
    const bool live = lane < n;
    const uint32_t i = p0 + lane;
    int* const stack = lds_stack + lane;
    float* const stage = (float*)lds_stack;
    static_assert(PTK_STACK_ROWS >= 3, "the staging area is three rows of the stack");

    // The group's points are 3 n consecutive floats: consecutive lanes read consecutive floats, through the rows of the stack the
    // walk does not use yet (stride 3 dwords on the way out: no two lanes of a half-wave on one bank).
    {
        const float* const gp = H.points + (size_t)p0 * 3;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t e = lane + k * PTK_CLOSEST_BLOCK;
            if (e < n * 3u) stage[e] = gp[e];
        }
    }
    __syncthreads();
    const v3 p = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    __syncthreads();                                                                // the rows are the stack from here on

    float md = __builtin_inff();
    if (live && H.max_dist) md = H.max_dist[i];
    const bool walks = live & (md > 0.0f);                                          // a NaN, zero or negative radius accepts nothing
    Closest best;
    best.d2 = md * md; best.tri = -1; best.v = 0.0f; best.w = 0.0f; best.qx = 0.0f; best.qy = 0.0f; best.qz = 0.0f;
    // what box distances and triangle distances can disagree by for this point, in position units
    const float E = (fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)) + H.scene_bound) * (PTK_CLOSEST_K * 0x1p-21f);
    float thr2 = prune_bound(best.d2, E);

    const float4* const nodes = uniform_ptr(H.nodes);
    const float4* const tris = uniform_ptr(H.tris);
    int node = walks ? 0 : NODE_EXIT;
    int* top = stack;
    uint32_t n_nodes = 0, n_tris = 0;
    // the next deferred link, NODE_EXIT when there is none
#define PTK_CLOSEST_POP(into) { if (top == stack) into = NODE_EXIT; else { top -= PTK_CLOSEST_BLOCK; into = *top; } }
    while (__ballot(node != NODE_EXIT))
    {
        if (node >= 0)                                        // ---- one 4-wide interior node
        {
            if (STATS) n_nodes++;
            const float4* np = (const float4*)((const char*)nodes + (uint32_t)node * (uint32_t)(NODE_F4 * 16));
            const float4 q0 = ldg4(np), q1 = ldg4(np + 1), q2 = ldg4(np + 2), q3 = ldg4(np + 3);
            const uint32_t lox = __float_as_uint(q2.z), loy = __float_as_uint(q2.w), loz = __float_as_uint(q3.x);
            const uint32_t hix = __float_as_uint(q3.y), hiy = __float_as_uint(q3.z), hiz = __float_as_uint(q3.w);
            const int link0 = __float_as_int(q1.z), link1 = __float_as_int(q1.w), link2 = __float_as_int(q2.x), link3 = __float_as_int(q2.y);
            // per child: plane = origin + q * scale; per axis the distance to the slab, max(lo - p, p - hi, 0); the order key is the
            // squared box distance (>= 0, so its bits order as integers) with the slot in its low bits.  An empty slot has an
            // inverted box, lo = 255 and hi = 0, which says nothing about distance: its link does
            // (a non-finite point can give db2 the bits 0x7fffffff, in slot 3 the key of "no survivor": that child is then neither
            // entered nor deferred - such a point's output is unspecified, and the walk still ends)
            int key[4];
            bool in[4];
#define PTK_CLOSEST_CHILD(k, link)                                                                                                              \
            {                                                                                                                                   \
                const float lx = __builtin_fmaf((float)((lox >> (8 * k)) & 255u), q0.w, q0.x), hx = __builtin_fmaf((float)((hix >> (8 * k)) & 255u), q0.w, q0.x); \
                const float ly = __builtin_fmaf((float)((loy >> (8 * k)) & 255u), q1.x, q0.y), hy = __builtin_fmaf((float)((hiy >> (8 * k)) & 255u), q1.x, q0.y); \
                const float lz = __builtin_fmaf((float)((loz >> (8 * k)) & 255u), q1.y, q0.z), hz = __builtin_fmaf((float)((hiz >> (8 * k)) & 255u), q1.y, q0.z); \
                const float dx = fmaxf(fmaxf(lx - p.x, p.x - hx), 0.0f), dy = fmaxf(fmaxf(ly - p.y, p.y - hy), 0.0f), dz = fmaxf(fmaxf(lz - p.z, p.z - hz), 0.0f); \
                const float db2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));                                                      \
                in[k] = ((link) != NODE_EXIT) & !(db2 > thr2);                                                                                  \
                key[k] = in[k] ? ((__float_as_int(db2) & ~3) | k) : 0x7fffffff;                                                                 \
            }
            PTK_CLOSEST_CHILD(0, link0) PTK_CLOSEST_CHILD(1, link1) PTK_CLOSEST_CHILD(2, link2) PTK_CLOSEST_CHILD(3, link3)
#undef PTK_CLOSEST_CHILD
            const int kmin = min(min(key[0], key[1]), min(key[2], key[3]));
            const bool o0 = key[0] != kmin, o1 = key[1] != kmin, o2 = key[2] != kmin, o3 = key[3] != kmin;
            int next = !o0 ? link0 : (!o1 ? link1 : (!o2 ? link2 : link3));
            // walk_step's pushes: every link is written at the running top, which moves on only behind a link that stays - at most
            // three per node, the nearest survivor being descended into: the discipline the builders' stack_need counts
            *top = link0; top += (in[0] & o0) ? PTK_CLOSEST_BLOCK : 0;
            *top = link1; top += (in[1] & o1) ? PTK_CLOSEST_BLOCK : 0;
            *top = link2; top += (in[2] & o2) ? PTK_CLOSEST_BLOCK : 0;
            *top = link3; top += (in[3] & o3) ? PTK_CLOSEST_BLOCK : 0;
#ifdef PTK_DEBUG                                                // (make EXTRA=-DPTK_DEBUG: DESIGN.md §4.17)
            assert(top - stack <= (PTK_STACK_ROWS - 1) * PTK_CLOSEST_BLOCK);
#endif
            if (kmin == 0x7fffffff) PTK_CLOSEST_POP(next)
            node = next;
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
            PTK_CLOSEST_POP(node)
        }
    }
#undef PTK_CLOSEST_POP
    __syncthreads();                                                                // every lane's stack is done: the rows stage the outputs

    const bool hit = best.tri >= 0;
    if (H.tri && live) H.tri[i] = hit ? best.tri : -1;
    if (H.dist && live) H.dist[i] = hit ? sqrt_ieee(best.d2) : __builtin_inff();
    if (H.point)
    {
        stage[lane * 3] = hit ? best.qx : 0.0f; stage[lane * 3 + 1] = hit ? best.qy : 0.0f; stage[lane * 3 + 2] = hit ? best.qz : 0.0f;
        __syncthreads();
        float* const gq = H.point + (size_t)p0 * 3;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t e = lane + k * PTK_CLOSEST_BLOCK;
            if (e < n * 3u) gq[e] = stage[e];
        }
        __syncthreads();
    }
    if (H.bary)
    {
        stage[lane * 2] = hit ? best.v : 0.0f; stage[lane * 2 + 1] = hit ? best.w : 0.0f;
        __syncthreads();
        float* const gb = H.bary + (size_t)p0 * 2;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++)
        {
            const uint32_t e = lane + k * PTK_CLOSEST_BLOCK;
            if (e < n * 2u) gb[e] = stage[e];
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
    const dim3 grid((unsigned)(((size_t)h.num_points + PTK_CLOSEST_BLOCK - 1) / PTK_CLOSEST_BLOCK));
    if (h.stats) hipLaunchKernelGGL(closest_kernel<true>, grid, dim3(PTK_CLOSEST_BLOCK), 0, stream, h);
    else hipLaunchKernelGGL(closest_kernel<false>, grid, dim3(PTK_CLOSEST_BLOCK), 0, stream, h);
}

}  // namespace ptk
