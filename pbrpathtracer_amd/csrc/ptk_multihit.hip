// HIP kernel for gfx950 of ordered multi-hit ray queries (include/ptk.h ptk_multihit_rays).  The shape and the
// walk are the one-wave ray queries' (ptk_query_walk.h: one-wave workgroups, one ray per lane, origins and directions staged
// through the stack rows of LDS, query_walk over walk_step_with of ptk_device_fn.h) with a triangle arm that keeps a bounded sorted
// list per lane, and the list's worst entry as the bound once the list is full.  The arm never stops the walk, so every record of
// every leaf the walk reaches is tested exactly once, and a node is only culled when nothing in it can enter the list, so the list
// ends as the first K of the ray's crossings in (t, triangle index) order whatever the tree.  Compiled once, with
// -ffp-contract=off: the triangle arm is tri_test's Moeller-Trumbore (mt_auvt, the same function; the numpy restatement is
// tests/multihit_rule.py); the node arm is acceleration only.
#include "ptk_query_walk.h"
#include "ptk_multihit.h"
#include "ptk.h"

namespace ptk {

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

// The rule of ptk.h for the record at `pos`: the crossings predicate with the ray's own bound, and then the list's - the key must
// be below the worst kept one, which lets a crossing that ties its t with a smaller index in.  W.best.t, which the node arm culls
// against, is refreshed: the ray's tmax while the list has a free slot (its key[0] holds +inf), the worst kept t afterwards - so a
// node is culled only when it lies beyond the worst kept crossing by more than the node arm's margin, and a crossing that ties it
// is still reached.  a, u, v, t are mt_auvt's, as in the epilogue: what the epilogue writes is what the walk decided on.
template <int KT>
__device__ __forceinline__ void mh_tri(Walk& W, const float4 t0, const float4 t1, const float4 t2, const uint32_t pos, const float tmax, MhList<KT>& L,
                                       const int K)
{
    float a, u, v, t;
    mt_auvt(W.ro, W.rd, t0, t1, t2, a, u, v, t);
    const uint64_t key = ((uint64_t)__float_as_uint(t) << 32) | (uint64_t)__float_as_uint(t2.y);
    bool ok = !(fabsf(a) < PTK_EPS) & !(u < 0.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t > PTK_EPS) & (t < tmax);
    ok = ok & (key < L.key[0]);
    if (__ballot(ok))
    {
        L.insert(ok, key, pos, K);
        W.best.t = fminf(tmax, __uint_as_float((uint32_t)(L.key[0] >> 32)));
    }
}

// The first K crossings of every ray, K <= KT.  Column c of a ray's answer is the list's slot K - 1 - c.
template <int KT>
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void multihit_kernel(const MultihitParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    static_assert(KT >= 1 && KT <= PTK_MULTIHIT_MAX, "the list holds at most PTK_MULTIHIT_MAX entries");
    const uint32_t lane = threadIdx.x;
    v3 ro, rd;
    const QueryGroup G = query_group<true>(lds_stack, H.num, H.origins, ro, H.dirs, &rd);
    const uint32_t ray0 = G.first, n = G.n, i = G.i;
    const bool live = G.live;
    float tmax;
    const bool walks = query_bound(G, H.tmax, tmax);
    const int K = min(__builtin_amdgcn_readfirstlane(H.max_hits), KT);              // (the launcher's choice: K <= KT)

    const QueryWalkParams WP = query_walk_params(H);
    MhList<KT> L;
    L.clear();
    int* const stack = lds_stack + lane;
    Walk W;
    W.occl_tri = -1;
    W.begin(ro, rd, walks ? H.num_nodes : 0, stack, H.scene_bound);                 // (no nodes: done at once)
    W.best.t = tmax;
    query_walk(WP, W, stack, [&](const float4 t0, const float4 t1, const float4 t2, const uint32_t pos) {
        mh_tri(W, t0, t1, t2, pos, tmax, L, K);
        return false;
    });

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
        for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.tri[first + e] = (int32_t)out[e];
    }
    if (H.t)
    {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && live) out[mine + (uint32_t)(K - 1 - j)] = (uint32_t)(L.key[j] >> 32);
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.t[first + e] = __uint_as_float(out[e]);
    }
    if (H.bary || H.side)
    {
        // u, v and the sign of a once more, from the records the entries name: mt_auvt again, so the bits the walk decided on.  side
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
                    mt_auvt(ro, rd, ldg4(tp), ldg4(tp + 1), ldg4(tp + 2), a, u, v, t);
                }
                L.pos[j] = kept ? (a > 0.0f ? 1u : 0xffu) : 0u;
                const uint32_t at = 2u * (mine + (uint32_t)(K - 1 - j));
                out[at] = __float_as_uint(u); out[at + 1] = __float_as_uint(v);
            }
        }
        __syncthreads();
        if (H.bary)
            for (uint32_t e = lane; e < 2u * nk; e += PTK_QUERY_BLOCK) H.bary[2 * first + e] = __uint_as_float(out[e]);
        if (H.side)
        {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KT; j++)
                if (j < K && live) out[mine + (uint32_t)(K - 1 - j)] = L.pos[j];
            __syncthreads();
            for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.side[first + e] = (int8_t)out[e];
        }
    }
}

void launch_multihit(const MultihitParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0 || h.max_hits < 1 || h.max_hits > PTK_MULTIHIT_MAX) return;
    const dim3 grid((unsigned)(((size_t)h.num + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK)), block(PTK_QUERY_BLOCK);
    if (h.max_hits <= 1) hipLaunchKernelGGL(multihit_kernel<1>, grid, block, 0, stream, h);
    else if (h.max_hits <= 2) hipLaunchKernelGGL(multihit_kernel<2>, grid, block, 0, stream, h);
    else if (h.max_hits <= 4) hipLaunchKernelGGL(multihit_kernel<4>, grid, block, 0, stream, h);
    else if (h.max_hits <= 8) hipLaunchKernelGGL(multihit_kernel<8>, grid, block, 0, stream, h);
    else hipLaunchKernelGGL(multihit_kernel<16>, grid, block, 0, stream, h);
}

}  // namespace ptk
