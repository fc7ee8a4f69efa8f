// HIP kernel for gfx950 of K-nearest triangle queries (include/ptk.h ptk_nearest_triangles): for every caller point
// the K triangles nearest to it, in order.  closest_kernel's walk (ptk_point_walk.h: one-wave workgroups, one point per lane, the
// points staged through LDS, the per-lane LDS stack of links, a distance-ordered, distance-pruned descent of the 4-wide quantised BVH
// under walk_step's push discipline) around multihit_kernel's list (ptk_multihit.hip: a bounded sorted list per lane in registers,
// integer keys, its worst entry the bound once it is full, the lists leaving coalesced through the stack rows).  Compiled once, with
// -ffp-contract=off: the triangle arm is the rule of ptk.h operation by operation (ptk_closest_rule.h; the numpy restatement is
// tests/knearest_rule.py); the box arm is acceleration only, behind the slack derived in DESIGN.md §4.17.
#include "ptk_point_walk.h"
#include "ptk_closest_rule.h"
#include "ptk_knearest.h"
#include "ptk.h"

namespace ptk {

// An entry's key: d2k (finite and >= +0, so its bits order as the floats do) above the triangle index - one unsigned 64-bit compare
// is the rule's (d2k, index) order, and the only comparison the list ever makes.  A free slot is all ones: above every entry's key.
#define PTK_NEAREST_FREE 0xffffffffffffffffull

// The list of one lane, in registers: every index below is a compile-time constant (the loops are unrolled), so nothing of it is
// addressed at run time.  MhList's order (ptk_multihit.hip): DESCENDING - key[0] is the worst entry kept, key[K - 1] the nearest
// triangle - so that the bound is always read from key[0], whatever K is.  Slots K .. KT - 1 stay free and are never touched.
// pos: the record's position in the triangle table, from which the epilogue finds v, w and q again.
template <int KT>
struct NearList {
    uint64_t key[KT];
    uint32_t pos[KT];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < KT; j++) { key[j] = PTK_NEAREST_FREE; pos[j] = 0u; }
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

// The K nearest triangles of every point, K <= KT.  Column c of a point's answer is the list's slot K - 1 - c.
template <int KT, bool STATS>
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void nearest_kernel(const NearestParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    static_assert(KT >= 1 && KT <= PTK_NEAREST_MAX_K, "the list holds at most PTK_NEAREST_MAX_K entries");
    const uint32_t lane = threadIdx.x;
    int* const stack = lds_stack + lane;
    const int K = min(__builtin_amdgcn_readfirstlane(H.k), KT);                     // (the launcher's choice: K <= KT)
    v3 p;
    const QueryGroup G = query_group(lds_stack, H.num_points, H.points, p);
    float md;
    const bool walks = query_bound(G, H.max_dist, md);                              // a NaN, zero or negative radius accepts nothing
    const float r2 = md * md;
    NearList<KT> L;
    L.clear();
    const float E = prune_slack(p, H.scene_bound);
    // the bound: r2 while the list has a free slot, the worst kept d2k afterwards.  It never grows: key[0] only falls, and below r2
    float thr2 = prune_bound(r2, E);

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
            const uint64_t before = L.key[0];
            for (uint32_t k = 0; k < count; k++)
            {
                const uint32_t pos = first + k;
                const float4* tp = (const float4*)((const char*)tris + pos * (uint32_t)(TRI_F4 * 16));
                const float4 t0 = ldg4(tp), t1 = ldg4(tp + 1), t2 = ldg4(tp + 2);
                const float d2k = closest_rule(p, t0, t1, t2).d2k;
                const uint64_t ck = ((uint64_t)__float_as_uint(d2k) << 32) | (uint64_t)__float_as_uint(t2.y);
                // finite, STRICTLY inside the radius, and below the worst kept entry: a NaN or an inf never enters the list
                const bool ok = (fabsf(d2k) < __builtin_inff()) & (d2k < r2) & (ck < L.key[0]);
                if (__ballot(ok)) L.insert(ok, ck, pos, K);
            }
            if (STATS) n_tris += count;
            // behind a leaf that changed key[0] of a full list, the bound is the d2k there (a free key[0] leaves the bound at r2)
            if ((L.key[0] != before) & (L.key[0] != PTK_NEAREST_FREE)) thr2 = prune_bound(__uint_as_float((uint32_t)(L.key[0] >> 32)), E);
            node = pop_link(stack, top);
        }
    }

    if (STATS)
    {
        atomicAdd(H.stats, (unsigned long long)n_nodes);
        atomicAdd(H.stats + 1, (unsigned long long)n_tris);
        return;
    }

    // The answers leave through the stack rows, free again (multihit_kernel's output stage): a group's part of an output is one
    // contiguous run of n * K elements, laid out in LDS as it lies in memory - column c of lane l at l * K + c - and then stored by
    // consecutive lanes to consecutive addresses.
    static_assert(PTK_STACK_ROWS >= 2 * PTK_NEAREST_MAX_K, "a group's bary, 2 x 64 x 16 words, passes through the stack rows");
    static_assert(2 * PTK_STACK_ROWS >= 3 * PTK_NEAREST_MAX_K, "half a group's points, 3 x 32 x 16 words, pass through the stack rows");
    uint32_t* const out = (uint32_t*)lds_stack;
    const uint32_t nk = G.n * (uint32_t)K;
    const size_t at = (size_t)G.first * (uint32_t)K;
    const uint32_t mine = lane * (uint32_t)K;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KT; j++) cnt += (j < K && L.key[j] != PTK_NEAREST_FREE) ? 1 : 0;
    if (H.count && G.live) H.count[G.i] = cnt;
    if (H.tri)
    {
        __syncthreads();                                                            // every lane's stack is done
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && G.live) out[mine + (uint32_t)(K - 1 - j)] = (uint32_t)L.key[j];      // (a free key's low word is -1)
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.tri[at + e] = (int32_t)out[e];
    }
    if (H.dist)
    {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && G.live)
            {
                const bool kept = L.key[j] != PTK_NEAREST_FREE;
                const float d = kept ? sqrt_ieee(__uint_as_float((uint32_t)(L.key[j] >> 32))) : __builtin_inff();
                out[mine + (uint32_t)(K - 1 - j)] = __float_as_uint(d);
            }
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.dist[at + e] = __uint_as_float(out[e]);
    }
    // v, w and q once more, from the records the entries name: closest_rule again, so the bits the walk decided on
    if (H.bary)
    {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KT; j++)
            if (j < K && G.live)
            {
                float v = 0.0f, w = 0.0f;
                if (L.key[j] != PTK_NEAREST_FREE)
                {
                    const float4* tp = (const float4*)((const char*)tris + L.pos[j] * (uint32_t)(TRI_F4 * 16));
                    const ClosestRule r = closest_rule(p, ldg4(tp), ldg4(tp + 1), ldg4(tp + 2));
                    v = r.v; w = r.w;
                }
                const uint32_t o = 2u * (mine + (uint32_t)(K - 1 - j));
                out[o] = __float_as_uint(v); out[o + 1] = __float_as_uint(w);
            }
        __syncthreads();
        for (uint32_t e = lane; e < 2u * nk; e += PTK_QUERY_BLOCK) H.bary[2 * at + e] = __uint_as_float(out[e]);
    }
    if (H.point)
    {
        // 3 x 64 x 16 words are more than the rows hold: the group's two halves of 32 lanes, one after the other
#pragma unroll
        for (uint32_t half = 0; half < 2; half++)
        {
            const uint32_t base = half * (PTK_QUERY_BLOCK / 2);
            const bool here = G.live & (lane >= base) & (lane < base + PTK_QUERY_BLOCK / 2);
            const uint32_t nh = G.n > base ? min(G.n - base, (uint32_t)(PTK_QUERY_BLOCK / 2)) : 0u;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KT; j++)
                if (j < K && here)
                {
                    v3 q = V(0.0f, 0.0f, 0.0f);
                    if (L.key[j] != PTK_NEAREST_FREE)
                    {
                        const float4* tp = (const float4*)((const char*)tris + L.pos[j] * (uint32_t)(TRI_F4 * 16));
                        q = closest_rule(p, ldg4(tp), ldg4(tp + 1), ldg4(tp + 2)).q;
                    }
                    const uint32_t o = 3u * ((lane - base) * (uint32_t)K + (uint32_t)(K - 1 - j));
                    out[o] = __float_as_uint(q.x); out[o + 1] = __float_as_uint(q.y); out[o + 2] = __float_as_uint(q.z);
                }
            __syncthreads();
            float* const gq = H.point + 3 * (at + (size_t)base * (uint32_t)K);
            for (uint32_t e = lane; e < 3u * nh * (uint32_t)K; e += PTK_QUERY_BLOCK) gq[e] = __uint_as_float(out[e]);
        }
    }
}

template <int KT>
static void launch_list(const NearestParams& h, const dim3 grid, hipStream_t stream)
{
    const dim3 block(PTK_QUERY_BLOCK);
    if (h.stats) hipLaunchKernelGGL((nearest_kernel<KT, true>), grid, block, 0, stream, h);
    else hipLaunchKernelGGL((nearest_kernel<KT, false>), grid, block, 0, stream, h);
}

void launch_nearest(const NearestParams& h, hipStream_t stream)
{
    if (h.num_points <= 0 || h.num_nodes <= 0 || h.k < 1 || h.k > PTK_NEAREST_MAX_K) return;
    const dim3 grid((unsigned)(((size_t)h.num_points + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK));
    if (h.k <= 1) launch_list<1>(h, grid, stream);
    else if (h.k <= 4) launch_list<4>(h, grid, stream);
    else launch_list<16>(h, grid, stream);
}

}  // namespace ptk
