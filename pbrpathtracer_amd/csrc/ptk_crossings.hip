// HIP kernels for gfx950 of crossing counts and point containment (include/ptk.h ptk_crossings_rays, ptk_contains_points,
// ptk_signed_distance).  The shape is hits_kernel's (ptk_hits.hip) - one-wave workgroups, one query per lane,
// origins and directions staged through the stack rows of LDS, the per-lane LDS stack of links, one node record in flight across
// iterations, the triangle arm voted by the wave - around a step of its own: walk_step's (ptk_device_fn.h) with a triangle arm that
// COUNTS every triangle the ray crosses instead of keeping the nearest.  Nothing tightens: W.best.t is the ray's tmax from begin to
// end, the node arm culls against it as the occlusion walk does against its bound, and no triangle ends a walk.  Compiled once,
// with -ffp-contract=off: the triangle arm is tri_test's Moeller-Trumbore operation by operation (the numpy restatement is
// tests/crossings_rule.py); the node arm is acceleration only.
#include "ptk_device_fn.h"
#include "ptk_crossings.h"
#include "ptk.h"

namespace ptk {

#define PTK_CROSS_BLOCK 64          // one wave per workgroup, one query per lane

// what the step reads of the launch parameters, held in SGPRs for the length of the loop (WalkParams without the shading tables)
struct CrossWalkParams { const float4* nodes; const float4* tris; int tri_thr; };

// The rule of ptk.h for one 48-byte record: tri_test's a, u, v, t - the same float32 operations in the same order - and its tests
// with the ray's bound in the place of the closest hit; no opacity, no tie rule, nothing kept but the two counts.
__device__ __forceinline__ void cross_tri(const Walk& W, const float4 t0, const float4 t1, const float4 t2, int& front, int& back)
{
    const v3 ro = W.ro, rd = W.rd;
    const v3 v0 = V(t0.x, t0.y, t0.z);
    const v3 edge1 = V(t0.w, t1.x, t1.y);
    const v3 edge2 = V(t1.z, t1.w, t2.x);
    const v3 h = cross(rd, edge2);
    const float a = dot(edge1, h);
    const float f = rcp_ieee(a);                // (|a| < EPS, a NaN or infinite: rejected below whatever f is)
    const v3 s = sub(ro, v0);
    const float u = f * dot(s, h);
    const v3 q = cross(s, edge1);
    const float v = f * dot(rd, q);
    const float t = f * dot(edge2, q);
    const bool ok = !(fabsf(a) < PTK_EPS) & !(u < 0.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t > PTK_EPS) & (t < W.best.t);
    front += (ok & (a > 0.0f)) ? 1 : 0;
    back += (ok & (a < 0.0f)) ? 1 : 0;
}

// One step of a lane: walk_step<.., PIPELINED> with cross_tri in arm A and no way out of the walk but its end.  Arm A tests up to
// two records - the pending leaf's next two, or its last and the first of the leaf the lane is blocked on - and every record of a
// leaf is queued exactly once, so every record of every leaf the walk reaches is tested exactly once: what counting needs.  Arm B
// is walk_step's node arm as it stands, the bound being W.best.t = tmax throughout.
template <int STRIDE>
__device__ __forceinline__ void cross_step(const CrossWalkParams& P, Walk& W, int* stack, const bool run_tri_arm, NodeRec& rec, int& front, int& back)
{
    const float4 q0 = rec.q0, q1 = rec.q1, q2 = rec.q2, q3 = rec.q3;
    asm volatile("" ::: "memory");
    const bool node_was = W.node >= 0;
    if (run_tri_arm && W.tri_left > 0)                    // ---- arm A: up to TWO triangles
    {
        const bool two = W.tri_left >= 2;
        const bool blocked = !two & (W.node < 0) & (W.node != NODE_EXIT);
        const int code = ~W.node;
        const int iA = W.tri_next, iB = two ? iA + 1 : (blocked ? (code >> 3) : iA);
        const float4* tpa = (const float4*)((const char*)P.tris + (uint32_t)iA * (uint32_t)(TRI_F4 * 16));
        const float4* tpb = (const float4*)((const char*)P.tris + (uint32_t)iB * (uint32_t)(TRI_F4 * 16));
        const float4 a0 = ldg4(tpa), a1 = ldg4(tpa + 1), a2 = ldg4(tpa + 2);
        const float4 b0 = ldg4(tpb), b1 = ldg4(tpb + 1), b2 = ldg4(tpb + 2);
        cross_tri(W, a0, a1, a2, front, back);
        if (two | blocked) cross_tri(W, b0, b1, b2, front, back);
        if (blocked)
        {
            W.tri_next = (code >> 3) + 1; W.tri_left = code & 7;
            W.node = W.template pop<STRIDE>(stack);
        }
        else { W.tri_next = iA + (two ? 2 : 1); W.tri_left -= two ? 2 : 1; }
    }
    if (node_was && W.node >= 0)                          // ---- arm B: one 4-wide interior node (its record is `rec`)
    {
        const float Ax = q0.w * W.inv.x, Ay = q1.x * W.inv.y, Az = q1.y * W.inv.z;
        const float Bnx = __builtin_fmaf(q0.x, W.inv.x, W.cn.x), Bny = __builtin_fmaf(q0.y, W.inv.y, W.cn.y), Bnz = __builtin_fmaf(q0.z, W.inv.z, W.cn.z);
        const float Bfx = __builtin_fmaf(q0.x, W.inv.x, W.cf.x), Bfy = __builtin_fmaf(q0.y, W.inv.y, W.cf.y), Bfz = __builtin_fmaf(q0.z, W.inv.z, W.cf.z);
        const uint32_t mx = W.sgnx, my = W.sgny, mz = W.sgnz;
        const uint32_t lox = __float_as_uint(q2.z), loy = __float_as_uint(q2.w), loz = __float_as_uint(q3.x);
        const uint32_t hix = __float_as_uint(q3.y), hiy = __float_as_uint(q3.z), hiz = __float_as_uint(q3.w);
        const uint32_t nx = (hix & mx) | (lox & ~mx), fx = (lox & mx) | (hix & ~mx);
        const uint32_t ny = (hiy & my) | (loy & ~my), fy = (loy & my) | (hiy & ~my);
        const uint32_t nz = (hiz & mz) | (loz & ~mz), fz = (loz & mz) | (hiz & ~mz);
        const int link0 = __float_as_int(q1.z), link1 = __float_as_int(q1.w), link2 = __float_as_int(q2.x), link3 = __float_as_int(q2.y);
        // the occlusion walk's bound with its margin for Moeller-Trumbore's own error in t; +inf without a tmax: nothing is pruned
        const float tmax = W.best.t * 1.0000153f;
        int key[4];
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const float tnx = __builtin_fmaf((float)((nx >> (8 * k)) & 255u), Ax, Bnx), tfx = __builtin_fmaf((float)((fx >> (8 * k)) & 255u), Ax, Bfx);
            const float tny = __builtin_fmaf((float)((ny >> (8 * k)) & 255u), Ay, Bny), tfy = __builtin_fmaf((float)((fy >> (8 * k)) & 255u), Ay, Bfy);
            const float tnz = __builtin_fmaf((float)((nz >> (8 * k)) & 255u), Az, Bnz), tfz = __builtin_fmaf((float)((fz >> (8 * k)) & 255u), Az, Bfz);
            const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            hit[k] = fmaxf(tn, 0.0f) <= fminf(tf, tmax);
            key[k] = hit[k] ? ((__float_as_int(tn) & ~3) | k) : 0x7fffffff;
        }
        const int kmin = min(min(key[0], key[1]), min(key[2], key[3]));
        const bool o0 = key[0] != kmin, o1 = key[1] != kmin, o2 = key[2] != kmin;
        int next = !o0 ? link0 : (!o1 ? link1 : (!o2 ? link2 : link3));
        // walk_step's pushes: every link is written at the running top, which moves on only behind a link that stays
        *W.top = link0; W.top += (hit[0] & o0) ? STRIDE : 0;
        *W.top = link1; W.top += (hit[1] & o1) ? STRIDE : 0;
        *W.top = link2; W.top += (hit[2] & o2) ? STRIDE : 0;
        *W.top = link3; W.top += (hit[3] & (key[3] != kmin)) ? STRIDE : 0;
        if (kmin == 0x7fffffff) next = W.template pop<STRIDE>(stack);
        W.node = next;
    }
    if (W.node < 0 && W.node != NODE_EXIT && W.tri_left == 0)   // a leaf and the triangle queue is free
    {
        const int code = ~W.node;
        W.tri_next = code >> 3;
        W.tri_left = (code & 7) + 1;
        W.node = W.template pop<STRIDE>(stack);
    }
    request_node(P, W, rec);                                    // for this lane's next step (a finished walk asks for the root)
}

// Every lane's walk of the ray (o, d) bounded by tmax to its end (walks false: the lane has no ray, or a bound that admits nothing);
// front and back are added to.
__device__ __forceinline__ void cross_walk(const CrossWalkParams& WP, const CrossingsParams& H, int* stack, const v3 o, const v3 d, const float tmax,
                                           const bool walks, int& front, int& back)
{
    Walk W;
    W.occl_tri = -1;
    W.begin(o, d, walks ? H.num_nodes : 0, stack, H.scene_bound);                   // (no nodes: done at once)
    W.best.t = tmax;
    NodeRec nrec;
    request_node(WP, W, nrec);
    while (__ballot(!W.done()))
    {
        // rays_kernel's vote: the triangle arm runs when enough lanes have triangles queued, and always when no lane has a node
        const int n_tq = __popcll(__ballot(W.tri_left > 0)), n_nr = __popcll(__ballot(W.node >= 0));
        const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));
        if (!W.done()) cross_step<PTK_CROSS_BLOCK>(WP, W, stack, run_tri_arm, nrec, front, back);
    }
}

__device__ __forceinline__ CrossWalkParams cross_params(const CrossingsParams& H)
{
    CrossWalkParams WP;
    WP.nodes = uniform_ptr(H.nodes); WP.tris = uniform_ptr(H.tris);
    WP.tri_thr = __builtin_amdgcn_readfirstlane(H.tri_thr);
    return WP;
}

// The group's 3 n consecutive floats of `src`, consecutive lanes reading consecutive floats, into rows [row0, row0 + 3) of the stack
__device__ __forceinline__ void stage_rows(float* stage, const float* src, uint32_t first, uint32_t n, uint32_t row0)
{
    const uint32_t lane = threadIdx.x;
    const float* const g = src + (size_t)first * 3;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
    {
        const uint32_t e = lane + k * PTK_CROSS_BLOCK;
        if (e < n * 3u) stage[row0 * PTK_CROSS_BLOCK + e] = g[e];
    }
}

// front / back of every ray
__global__ __launch_bounds__(PTK_CROSS_BLOCK) void crossings_kernel(const CrossingsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_CROSS_BLOCK];
    static_assert(PTK_STACK_ROWS >= 6, "the staging area is six rows of the stack");
    const uint32_t lane = threadIdx.x;
    const uint32_t ray0 = blockIdx.x * (uint32_t)PTK_CROSS_BLOCK;                  // < num <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_CROSS_BLOCK, (uint32_t)H.num - ray0);
    const bool live = lane < n;
    const uint32_t i = ray0 + lane;
    float* const stage = (float*)lds_stack;
    stage_rows(stage, H.origins, ray0, n, 0);
    stage_rows(stage, H.dirs, ray0, n, 3);
    __syncthreads();
    // (stride 3 dwords: no two lanes of a half-wave on one bank)
    const v3 ro = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    const v3 rd = live ? V(stage[3 * PTK_CROSS_BLOCK + lane * 3], stage[3 * PTK_CROSS_BLOCK + lane * 3 + 1], stage[3 * PTK_CROSS_BLOCK + lane * 3 + 2])
                       : V(0.0f, 0.0f, 1.0f);
    __syncthreads();                                                                // the rows are the stack from here on
    float tmax = __builtin_inff();
    if (live && H.tmax) tmax = H.tmax[i];
    const bool walks = live & (tmax > 0.0f);                                        // a NaN, zero or negative bound admits nothing
    int front = 0, back = 0;
    cross_walk(cross_params(H), H, lds_stack + lane, ro, rd, tmax, walks, front, back);
    if (H.front && live) H.front[i] = front;
    if (H.back && live) H.back[i] = back;
}

// the built-in direction set of ptk_contains_points (ptk.h)
__constant__ float k_inside_dirs[9] = PTK_INSIDE_DEFAULT_DIRS;

// inside / winding of every point; the sign of dist.  The directions are wave-uniform: all lanes walk direction j at the same time
// (a coherent walk: the lanes' rays are parallel and their origins neighbours), each direction a walk begun afresh on the same
// stack column - empty again when a walk has ended - and the vote is kept in a register, so the kernel needs no memory of its own.
__global__ __launch_bounds__(PTK_CROSS_BLOCK) void contains_kernel(const CrossingsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_CROSS_BLOCK];
    static_assert(PTK_STACK_ROWS >= 3, "the staging area is three rows of the stack");
    const uint32_t lane = threadIdx.x;
    const uint32_t p0 = blockIdx.x * (uint32_t)PTK_CROSS_BLOCK;                    // < num <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_CROSS_BLOCK, (uint32_t)H.num - p0);
    const bool live = lane < n;
    const uint32_t i = p0 + lane;
    float* const stage = (float*)lds_stack;
    stage_rows(stage, H.origins, p0, n, 0);
    __syncthreads();
    const v3 p = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    __syncthreads();                                                                // the rows are the stack from here on
    const CrossWalkParams WP = cross_params(H);
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

static dim3 cross_grid(const CrossingsParams& h) { return dim3((unsigned)(((size_t)h.num + PTK_CROSS_BLOCK - 1) / PTK_CROSS_BLOCK)); }

void launch_crossings(const CrossingsParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(crossings_kernel, cross_grid(h), dim3(PTK_CROSS_BLOCK), 0, stream, h);
}

void launch_contains(const CrossingsParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(contains_kernel, cross_grid(h), dim3(PTK_CROSS_BLOCK), 0, stream, h);
}

}  // namespace ptk
