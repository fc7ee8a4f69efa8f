// HIP kernel for gfx950 of ordered multi-hit ray queries (include/ptk.h ptk_multihit_rays).  The shape is
// crossings_kernel's (ptk_crossings.hip) - one-wave workgroups, one ray per lane, origins and directions staged through the stack
// rows of LDS, the per-lane LDS stack of links, one node record in flight across iterations, the triangle arm voted by the wave -
// around a step of its own: cross_step's with a bounded sorted list per lane in the place of the two counters, and the list's worst
// entry as the bound once the list is full.  Every record of every leaf the walk reaches is tested exactly once, and a node is only
// culled when nothing in it can enter the list, so the list ends as the first K of the ray's crossings in (t, triangle index)
// order whatever the tree.  Compiled once, with -ffp-contract=off: the triangle arm is tri_test's Moeller-Trumbore operation by
// operation (the numpy restatement is tests/multihit_rule.py); the node arm is acceleration only.
#include "ptk_device_fn.h"
#include "ptk_multihit.h"
#include "ptk.h"

namespace ptk {

#define PTK_MH_BLOCK 64             // one wave per workgroup, one ray per lane

// what the step reads of the launch parameters, held in SGPRs for the length of the loop
struct MhWalkParams { const float4* nodes; const float4* tris; int tri_thr; };

// An entry's key: the crossing's t (positive, so its bits order as the floats do) above the triangle index - one unsigned 64-bit
// compare is the rule's (t, index) order.  The key of a free slot, (+inf, -1), is above every crossing's: t < tmax <= inf.
#define PTK_MH_FREE 0x7f800000ffffffffull

// The list of one lane, in registers: every index below is a compile-time constant (the loops are unrolled), so nothing of it is
// addressed at run time.  It is kept DESCENDING - key[0] is the worst entry kept, key[K - 1] the ray's first crossing - so that
// the bound both arms read is always key[0], whatever K is.  Slots K .. KT - 1 stay free and are never touched.
// pos: the record's position in the triangle table, from which the epilogue finds u, v and the sign of a again.
template <int KT>
struct MhList {
    uint64_t key[KT];
    uint32_t pos[KT];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < KT; j++) { key[j] = PTK_MH_FREE; pos[j] = 0u; }
    }
    // (ck, cp) replaces the worst entry in the lanes where `in`, then sinks to its place: one compare-exchange per slot.  A lane
    // that takes nothing in finds its list in order and exchanges nothing.
    __device__ __forceinline__ void insert(const bool in, const uint64_t ck, const uint32_t cp, const int K)
    {
        key[0] = in ? ck : key[0];
        pos[0] = in ? cp : pos[0];
#pragma unroll
        for (int j = 0; j + 1 < KT; j++)
        {
            const bool sw = (j + 1 < K) & (key[j] < key[j + 1]);
            const uint64_t k0 = key[j], k1 = key[j + 1];
            const uint32_t p0 = pos[j], p1 = pos[j + 1];
            key[j] = sw ? k1 : k0; key[j + 1] = sw ? k0 : k1;
            pos[j] = sw ? p1 : p0; pos[j + 1] = sw ? p0 : p1;
        }
    }
};

// tri_test's a, u, v, t for one 48-byte record - the same float32 operations in the same order.  The walk and the epilogue both
// come through here, so what the epilogue writes is what the walk decided on.
__device__ __forceinline__ void mh_mt(const v3 ro, const v3 rd, const float4 t0, const float4 t1, const float4 t2, float& a, float& u, float& v, float& t)
{
    const v3 v0 = V(t0.x, t0.y, t0.z);
    const v3 edge1 = V(t0.w, t1.x, t1.y);
    const v3 edge2 = V(t1.z, t1.w, t2.x);
    const v3 h = cross(rd, edge2);
    a = dot(edge1, h);
    const float f = rcp_ieee(a);                // (|a| < EPS, a NaN or infinite: rejected below whatever f is)
    const v3 s = sub(ro, v0);
    u = f * dot(s, h);
    const v3 q = cross(s, edge1);
    v = f * dot(rd, q);
    t = f * dot(edge2, q);
}

// The rule of ptk.h for the record at `pos`: the crossings predicate with the ray's own bound, and then the list's - the key must
// be below the worst kept one, which lets a crossing that ties its t with a smaller index in.  W.best.t is refreshed: the ray's
// tmax while the list has a free slot (its key[0] holds +inf), the worst kept t afterwards.
template <int KT>
__device__ __forceinline__ void mh_tri(Walk& W, const float4 t0, const float4 t1, const float4 t2, const uint32_t pos, const float tmax, MhList<KT>& L,
                                       const int K)
{
    float a, u, v, t;
    mh_mt(W.ro, W.rd, t0, t1, t2, a, u, v, t);
    const uint64_t key = ((uint64_t)__float_as_uint(t) << 32) | (uint64_t)__float_as_uint(t2.y);
    bool ok = !(fabsf(a) < PTK_EPS) & !(u < 0.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t > PTK_EPS) & (t < tmax);
    ok = ok & (key < L.key[0]);
    if (__ballot(ok))
    {
        L.insert(ok, key, pos, K);
        W.best.t = fminf(tmax, __uint_as_float((uint32_t)(L.key[0] >> 32)));
    }
}

// One step of a lane: cross_step with mh_tri in arm A.  Arm B is walk_step's node arm as it stands - its margin and its <= - against
// W.best.t, which arm A keeps at the list's bound.
template <int STRIDE, int KT>
__device__ __forceinline__ void mh_step(const MhWalkParams& P, Walk& W, int* stack, const bool run_tri_arm, NodeRec& rec, const float tmax, MhList<KT>& L,
                                        const int K)
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
        mh_tri(W, a0, a1, a2, (uint32_t)iA, tmax, L, K);
        if (two | blocked) mh_tri(W, b0, b1, b2, (uint32_t)iB, tmax, L, K);
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
        // walk_step's bound with its margin for Moeller-Trumbore's own error in t: a node is culled only when it lies beyond the
        // worst kept crossing by more than that error, so a crossing that ties it is still reached
        const float bound = W.best.t * 1.0000153f;
        int key[4];
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const float tnx = __builtin_fmaf((float)((nx >> (8 * k)) & 255u), Ax, Bnx), tfx = __builtin_fmaf((float)((fx >> (8 * k)) & 255u), Ax, Bfx);
            const float tny = __builtin_fmaf((float)((ny >> (8 * k)) & 255u), Ay, Bny), tfy = __builtin_fmaf((float)((fy >> (8 * k)) & 255u), Ay, Bfy);
            const float tnz = __builtin_fmaf((float)((nz >> (8 * k)) & 255u), Az, Bnz), tfz = __builtin_fmaf((float)((fz >> (8 * k)) & 255u), Az, Bfz);
            const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            hit[k] = fmaxf(tn, 0.0f) <= fminf(tf, bound);
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

// The group's 3 n consecutive floats of `src`, consecutive lanes reading consecutive floats, into rows [row0, row0 + 3) of the stack
__device__ __forceinline__ void mh_stage_rows(float* stage, const float* src, uint32_t first, uint32_t n, uint32_t row0)
{
    const uint32_t lane = threadIdx.x;
    const float* const g = src + (size_t)first * 3;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
    {
        const uint32_t e = lane + k * PTK_MH_BLOCK;
        if (e < n * 3u) stage[row0 * PTK_MH_BLOCK + e] = g[e];
    }
}

// The first K crossings of every ray, K <= KT.  Column c of a ray's answer is the list's slot K - 1 - c.
template <int KT>
__global__ __launch_bounds__(PTK_MH_BLOCK) void multihit_kernel(const MultihitParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_MH_BLOCK];
    static_assert(PTK_STACK_ROWS >= 6, "the staging area is six rows of the stack");
    static_assert(KT >= 1 && KT <= PTK_MULTIHIT_MAX, "the list holds at most PTK_MULTIHIT_MAX entries");
    const uint32_t lane = threadIdx.x;
    const uint32_t ray0 = blockIdx.x * (uint32_t)PTK_MH_BLOCK;                     // < num <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_MH_BLOCK, (uint32_t)H.num - ray0);
    const bool live = lane < n;
    const uint32_t i = ray0 + lane;
    float* const stage = (float*)lds_stack;
    mh_stage_rows(stage, H.origins, ray0, n, 0);
    mh_stage_rows(stage, H.dirs, ray0, n, 3);
    __syncthreads();
    // (stride 3 dwords: no two lanes of a half-wave on one bank)
    const v3 ro = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    const v3 rd = live ? V(stage[3 * PTK_MH_BLOCK + lane * 3], stage[3 * PTK_MH_BLOCK + lane * 3 + 1], stage[3 * PTK_MH_BLOCK + lane * 3 + 2])
                       : V(0.0f, 0.0f, 1.0f);
    __syncthreads();                                                                // the rows are the stack from here on
    float tmax = __builtin_inff();
    if (live && H.tmax) tmax = H.tmax[i];
    const bool walks = live & (tmax > 0.0f);                                        // a NaN, zero or negative bound admits nothing
    const int K = min(__builtin_amdgcn_readfirstlane(H.max_hits), KT);              // (the launcher's choice: K <= KT)

    MhWalkParams WP;
    WP.nodes = uniform_ptr(H.nodes); WP.tris = uniform_ptr(H.tris);
    WP.tri_thr = __builtin_amdgcn_readfirstlane(H.tri_thr);
    MhList<KT> L;
    L.clear();
    int* const stack = lds_stack + lane;
    Walk W;
    W.occl_tri = -1;
    W.begin(ro, rd, walks ? H.num_nodes : 0, stack, H.scene_bound);                 // (no nodes: done at once)
    W.best.t = tmax;
    NodeRec nrec;
    request_node(WP, W, nrec);
    while (__ballot(!W.done()))
    {
        // rays_kernel's vote: the triangle arm runs when enough lanes have triangles queued, and always when no lane has a node
        const int n_tq = __popcll(__ballot(W.tri_left > 0)), n_nr = __popcll(__ballot(W.node >= 0));
        const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));
        if (!W.done()) mh_step<PTK_MH_BLOCK>(WP, W, stack, run_tri_arm, nrec, tmax, L, K);
    }

    // The answers leave through the stack rows, free again: a group's part of an output is one contiguous run of n * K elements
    // (2 n K for bary), laid out in LDS as it lies in memory - column c of lane l at l * K + c - and then stored by consecutive
    // lanes to consecutive addresses.  Stored straight from the registers, each lane would write K words a row apart from its
    // neighbour's: K partial lines per store instruction.
    static_assert(PTK_STACK_ROWS >= 2 * PTK_MULTIHIT_MAX, "a group's bary, 2 x 64 x 16 words, passes through the stack rows");
    uint32_t* const out = (uint32_t*)lds_stack;
    const uint32_t nk = n * (uint32_t)K;
    const size_t first = (size_t)ray0 * (uint32_t)K;
    const uint32_t mine = lane * (uint32_t)K;
    int count = 0;
#pragma unroll
    for (int j = 0; j < KT; j++) count += (j < K && L.key[j] != PTK_MH_FREE) ? 1 : 0;
    if (H.count && live) H.count[i] = count;
    if (H.tri)
    {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && live) out[mine + (uint32_t)(K - 1 - j)] = (uint32_t)L.key[j];
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_MH_BLOCK) H.tri[first + e] = (int32_t)out[e];
    }
    if (H.t)
    {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && live) out[mine + (uint32_t)(K - 1 - j)] = (uint32_t)(L.key[j] >> 32);
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_MH_BLOCK) H.t[first + e] = __uint_as_float(out[e]);
    }
    if (H.bary || H.side)
    {
        // u, v and the sign of a once more, from the records the entries name: mh_mt again, so the bits the walk decided on.  side
        // waits in the key's low word, which has been stored
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
        {
            if (j < K && live)
            {
                const bool kept = L.key[j] != PTK_MH_FREE;
                float a = 0.0f, u = 0.0f, v = 0.0f, t;
                if (kept)
                {
                    const float4* tp = (const float4*)((const char*)WP.tris + L.pos[j] * (uint32_t)(TRI_F4 * 16));
                    mh_mt(ro, rd, ldg4(tp), ldg4(tp + 1), ldg4(tp + 2), a, u, v, t);
                }
                L.pos[j] = kept ? (a > 0.0f ? 1u : 0xffu) : 0u;
                const uint32_t at = 2u * (mine + (uint32_t)(K - 1 - j));
                out[at] = __float_as_uint(u); out[at + 1] = __float_as_uint(v);
            }
        }
        __syncthreads();
        if (H.bary)
            for (uint32_t e = lane; e < 2u * nk; e += PTK_MH_BLOCK) H.bary[2 * first + e] = __uint_as_float(out[e]);
        if (H.side)
        {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KT; j++)
                if (j < K && live) out[mine + (uint32_t)(K - 1 - j)] = L.pos[j];
            __syncthreads();
            for (uint32_t e = lane; e < nk; e += PTK_MH_BLOCK) H.side[first + e] = (int8_t)out[e];
        }
    }
}

void launch_multihit(const MultihitParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0 || h.max_hits < 1 || h.max_hits > PTK_MULTIHIT_MAX) return;
    const dim3 grid((unsigned)(((size_t)h.num + PTK_MH_BLOCK - 1) / PTK_MH_BLOCK)), block(PTK_MH_BLOCK);
    if (h.max_hits <= 1) hipLaunchKernelGGL(multihit_kernel<1>, grid, block, 0, stream, h);
    else if (h.max_hits <= 2) hipLaunchKernelGGL(multihit_kernel<2>, grid, block, 0, stream, h);
    else if (h.max_hits <= 4) hipLaunchKernelGGL(multihit_kernel<4>, grid, block, 0, stream, h);
    else if (h.max_hits <= 8) hipLaunchKernelGGL(multihit_kernel<8>, grid, block, 0, stream, h);
    else hipLaunchKernelGGL(multihit_kernel<16>, grid, block, 0, stream, h);
}

}  // namespace ptk
