// HIP kernel for gfx950 of overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres): for every caller
// box or sphere the number of triangles that meet it and the smallest of their indices.  The shape is closest_kernel's
// (ptk_closest.hip) - one-wave workgroups, one query per lane, the query arrays staged through LDS (ptk_query_walk.h), the per-lane
// LDS stack of links - around a third kind of walk of the 4-wide quantised BVH: the region is fixed, so nothing is ordered and no
// bound moves; a child survives or it does not.  The node's decode, the bound and the pop are ptk_point_walk.h's, the node arm's
// choice of what to enter and what to defer is this file's.  Compiled once, with -ffp-contract=off: the triangle arm is the rule of
// ptk.h operation by operation (a sphere's is closest_rule, ptk_closest_rule.h; the numpy restatement is tests/overlap_rule.py);
// the box arm is acceleration only, behind the slack derived in DESIGN.md §4.27.
#include "ptk_point_walk.h"
#include "ptk_closest_rule.h"
#include "ptk_overlap.h"
#include "ptk.h"

namespace ptk {

// The experiment of DESIGN.md §4.27.  0: the box rule as straight-line code over all 13 axes.  1: the three box axes first, the
// other ten behind a wave vote of the lanes those three did not separate.  Same bits either way.
#ifndef PTK_OVERLAP_VOTE
#define PTK_OVERLAP_VOTE 0
#endif
#define PTK_OVERLAP_FREE 0x7fffffff // a free slot of a lane's list: above every triangle index

// min / max of the rule: a NaN operand is ignored (fminf / fmaxf; v_min_f32 / v_max_f32 with IEEE mode on), so an extreme is NaN only
// when every operand is, and then its comparison is false: no separation
__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// The three box axes of the rule: additions and comparisons alone.
__device__ __forceinline__ bool box_axes_meet(const v3 v0, const v3 v1, const v3 v2, const v3 h)
{
    const float nx = min3(v0.x, v1.x, v2.x), ny = min3(v0.y, v1.y, v2.y), nz = min3(v0.z, v1.z, v2.z);
    const float mx = max3(v0.x, v1.x, v2.x), my = max3(v0.y, v1.y, v2.y), mz = max3(v0.z, v1.z, v2.z);
    const bool sx = (nx > h.x) | (mx < -h.x), sy = (ny > h.y) | (my < -h.y), sz = (nz > h.z) | (mz < -h.z);
    return !(sx | sy | sz);
}

// One edge axis cross(unit j, f): k = j + 1 mod 3, l = j + 2 mod 3 are the two components named.
#define PTK_OVERLAP_EDGE(f, k, l)                                                                                               \
    {                                                                                                                           \
        const float p0 = v0.l * f.k - v0.k * f.l, p1 = v1.l * f.k - v1.k * f.l, p2 = v2.l * f.k - v2.k * f.l;                   \
        const float rr = h.k * fabsf(f.l) + h.l * fabsf(f.k);                                                                   \
        const float pn = min3(p0, p1, p2), px = max3(p0, p1, p2);                                                               \
        sep |= (pn > rr) | (px < -rr);                                                                                          \
    }

// The plane and the nine edge axes of the rule.  The plane axis projects all three vertices, as the edge axes do: for a proper
// triangle the three agree up to rounding, and for a nearly collinear one - whose computed n is rounding noise - the test stays a
// separating-axis test, which n . v0 alone is not (it then rejects boxes that hold the far end of the sliver: DESIGN.md 4.27).
__device__ __forceinline__ bool other_axes_meet(const v3 v0, const v3 v1, const v3 v2, const v3 e1, const v3 e2, const v3 h)
{
    const v3 n = cross(e1, e2);
    const float d0 = (n.x * v0.x + n.y * v0.y) + n.z * v0.z, d1 = (n.x * v1.x + n.y * v1.y) + n.z * v1.z, d2 = (n.x * v2.x + n.y * v2.y) + n.z * v2.z;
    const float r = (h.x * fabsf(n.x) + h.y * fabsf(n.y)) + h.z * fabsf(n.z);
    const float dn = min3(d0, d1, d2), dx = max3(d0, d1, d2);
    bool sep = (dn > r) | (dx < -r);
    const v3 f1 = sub(e2, e1);
    PTK_OVERLAP_EDGE(e1, y, z) PTK_OVERLAP_EDGE(e1, z, x) PTK_OVERLAP_EDGE(e1, x, y)
    PTK_OVERLAP_EDGE(f1, y, z) PTK_OVERLAP_EDGE(f1, z, x) PTK_OVERLAP_EDGE(f1, x, y)
    PTK_OVERLAP_EDGE(e2, y, z) PTK_OVERLAP_EDGE(e2, z, x) PTK_OVERLAP_EDGE(e2, x, y)
    return !sep;
}
#undef PTK_OVERLAP_EDGE

// The list of one lane, in registers, indexed by unrolled loops only (multihit's discipline, ptk_multihit.hip): DESCENDING, so
// key[0] is the largest index kept - or PTK_OVERLAP_FREE while a slot is free - and one compare against it rejects what cannot enter.
template <int KT>
struct OverlapList {
    int key[KT > 0 ? KT : 1];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < KT; j++) key[j] = PTK_OVERLAP_FREE;
    }
    // tri replaces key[0] in the lanes where `in`, then sinks to its place: one compare-exchange per slot
    __device__ __forceinline__ void insert(const bool in, const int tri)
    {
        key[0] = in ? tri : key[0];
#pragma unroll
        for (int j = 0; j + 1 < KT; j++)
        {
            const int k0 = key[j], k1 = key[j + 1];
            const bool sw = k0 < k1;
            key[j] = sw ? k1 : k0; key[j + 1] = sw ? k0 : k1;
        }
    }
};

// SHAPE: OVERLAP_BOX / OVERLAP_SPHERE.  KT: the list's capacity, 0 = count only; H.k <= KT columns are written.
template <int SHAPE, int KT, bool STATS>
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void overlap_kernel(const OverlapParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    constexpr bool BOX = SHAPE == OVERLAP_BOX;
    const uint32_t lane = threadIdx.x;
    int* const stack = lds_stack + lane;
    static_assert(PTK_STACK_ROWS >= PTK_OVERLAP_MAX_K && KT <= PTK_OVERLAP_MAX_K, "a group's lists, 64 x 16 words, pass through the stack rows");
    // lo / centers and, of boxes, hi (a sphere's radius is one dword per lane, read below)
    v3 A, B;
    const QueryGroup G = query_group<BOX>(lds_stack, H.num, H.qa, A, H.qb, &B);

    int from = 0;
    if (G.live && H.tri_from) from = max(H.tri_from[G.i], 0);
    // what the walk prunes with.  Boxes: the query box grown by E, against which a child's decoded planes are compared; c, h of
    // the rule.  Spheres: the squared bound, fixed for the whole walk; A is the centre, r2 the rule's
    bool walks;
    v3 c = V(0.0f, 0.0f, 0.0f), h = c, loE = c, hiE = c;
    float r2 = 0.0f, thr2 = 0.0f;
    if (BOX)
    {
        walks = G.live & (A.x <= B.x) & (A.y <= B.y) & (A.z <= B.z);                  // a reversed or NaN box accepts nothing
        c = V((A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f);
        h = V((B.x - A.x) * 0.5f, (B.y - A.y) * 0.5f, (B.z - A.z) * 0.5f);
        const float M = fmaxf(fmaxf(fmaxf(fabsf(A.x), fabsf(A.y)), fabsf(A.z)), fmaxf(fmaxf(fabsf(B.x), fabsf(B.y)), fabsf(B.z)));
        const float E = prune_slack(M, H.scene_bound);
        loE = V(A.x - E, A.y - E, A.z - E); hiE = V(B.x + E, B.y + E, B.z + E);
    }
    else
    {
        float r = 0.0f;
        if (G.live) r = H.qb[G.i];
        walks = G.live & (r > 0.0f);                                                  // a NaN, zero or negative radius accepts nothing
        r2 = r * r;
        thr2 = prune_bound(r2, prune_slack(A, H.scene_bound));
    }

    OverlapList<KT> L;
    L.clear();
    int count = 0;
    const float4* const nodes = uniform_ptr(H.nodes);
    const float4* const tris = uniform_ptr(H.tris);
    int node = walks ? 0 : NODE_EXIT;
    int* top = stack;
    uint32_t n_nodes = 0, n_tris = 0, n_past = 0;
    while (__ballot(node != NODE_EXIT))
    {
        if (node >= 0)                                        // ---- one 4-wide interior node
        {
            if (STATS) n_nodes++;
            const PointNode N = point_node(nodes, node);
            // a box query drops a child whose planes lie beyond the grown query box on some axis, a sphere query one whose box
            // distance exceeds the bound.  Every comparison is false for a NaN: nothing is dropped then
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                bool out;
                if (BOX)
                {
                    const ChildBox b = child_box(N, k);
                    out = (b.lx > hiE.x) | (b.hx < loE.x) | (b.ly > hiE.y) | (b.hy < loE.y) | (b.lz > hiE.z) | (b.hz < loE.z);
                }
                else out = child_dist2(N, k, A) > thr2;
                in[k] = (N.link[k] != NODE_EXIT) & !out;
            }
            // the lane descends into its first survivor and defers the others: walk_step's pushes - every link is written at the
            // running top, which moves on only behind a link that stays - at most three per node, the discipline the builders'
            // stack_need counts (slot 0 is entered or dropped, never deferred)
            int next = in[0] ? N.link[0] : (in[1] ? N.link[1] : (in[2] ? N.link[2] : N.link[3]));
            *top = N.link[1]; top += (in[1] & in[0]) ? PTK_QUERY_BLOCK : 0;
            *top = N.link[2]; top += (in[2] & (in[0] | in[1])) ? PTK_QUERY_BLOCK : 0;
            *top = N.link[3]; top += (in[3] & (in[0] | in[1] | in[2])) ? PTK_QUERY_BLOCK : 0;
            check_stack(stack, top);
            if (!(in[0] | in[1] | in[2] | in[3])) next = pop_link(stack, top);
            node = next;
        }
        else if (node != NODE_EXIT)                           // ---- a leaf: its 1 .. 8 records, then the next deferred link
        {
            const int code = ~node;
            const uint32_t first = (uint32_t)(code >> 3), cnt = (uint32_t)(code & 7) + 1u;
            for (uint32_t k = 0; k < cnt; k++)
            {
                const float4* tp = (const float4*)((const char*)tris + (first + k) * (uint32_t)(TRI_F4 * 16));
                const float4 t0 = ldg4(tp), t1 = ldg4(tp + 1), t2 = ldg4(tp + 2);
                const int tri = __float_as_int(t2.y);
                bool ok;
                if (BOX)
                {
                    const v3 a = V(t0.x, t0.y, t0.z), e1 = V(t0.w, t1.x, t1.y), e2 = V(t1.z, t1.w, t2.x);
                    const v3 v0 = sub(a, c), v1 = add(v0, e1), v2 = add(v0, e2);
                    ok = box_axes_meet(v0, v1, v2, h);
                    if (STATS) n_past += ok ? 1u : 0u;
#if PTK_OVERLAP_VOTE
                    if (__ballot(ok)) ok = ok & other_axes_meet(v0, v1, v2, e1, e2, h);
#else
                    ok = ok & other_axes_meet(v0, v1, v2, e1, e2, h);
#endif
                }
                else
                {
                    const float d2k = closest_rule(A, t0, t1, t2).d2k;
                    ok = (fabsf(d2k) < __builtin_inff()) & (d2k < r2);              // finite, and STRICTLY inside
                }
                ok = ok & (tri >= from);
                count += ok ? 1 : 0;
                if (KT > 0)
                {
                    const bool enters = ok & (tri < L.key[0]);
                    if (__ballot(enters)) L.insert(enters, tri);
                }
            }
            if (STATS) n_tris += cnt;
            node = pop_link(stack, top);
        }
    }

    if (STATS)
    {
        atomicAdd(H.stats, (unsigned long long)n_nodes);
        atomicAdd(H.stats + 1, (unsigned long long)n_tris);
        atomicAdd(H.stats + 2, (unsigned long long)count);
        atomicAdd(H.stats + 3, (unsigned long long)n_past);
        return;
    }
    if (H.count && G.live) H.count[G.i] = count;
    if (KT > 0 && H.list)
    {
        // The lists leave through the stack rows, free again: a group's part is one contiguous run of n * k indices, laid out in
        // LDS as it lies in memory - column c of lane l at l * k + c - and stored by consecutive lanes to consecutive addresses.
        // Column c is the list's slot KT - 1 - c: the smallest index first.
        const int K = min(__builtin_amdgcn_readfirstlane(H.k), KT);
        int* const out = lds_stack;
        const uint32_t nk = G.n * (uint32_t)K;
        const size_t at = (size_t)G.first * (uint32_t)K;
        const uint32_t mine = lane * (uint32_t)K;
        __syncthreads();                                                            // every lane's stack is done
#pragma unroll
        for (int j = 0; j < KT; j++)
        {
            const int col = KT - 1 - j;
            if (col < K && G.live) out[mine + (uint32_t)col] = L.key[j] == PTK_OVERLAP_FREE ? -1 : L.key[j];
        }
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_QUERY_BLOCK) H.list[at + e] = out[e];
    }
}

template <int SHAPE>
static void launch_shape(const OverlapParams& h, const dim3 grid, hipStream_t stream)
{
    const dim3 block(PTK_QUERY_BLOCK);
    if (h.stats) hipLaunchKernelGGL((overlap_kernel<SHAPE, 0, true>), grid, block, 0, stream, h);
    else if (h.k <= 0 || !h.list) hipLaunchKernelGGL((overlap_kernel<SHAPE, 0, false>), grid, block, 0, stream, h);
    else if (h.k <= 4) hipLaunchKernelGGL((overlap_kernel<SHAPE, 4, false>), grid, block, 0, stream, h);
    else hipLaunchKernelGGL((overlap_kernel<SHAPE, 16, false>), grid, block, 0, stream, h);
}

void launch_overlap(const OverlapParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0 || h.k < 0 || h.k > PTK_OVERLAP_MAX_K) return;
    const dim3 grid((unsigned)(((size_t)h.num + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK));
    if (h.shape == OVERLAP_BOX) launch_shape<OVERLAP_BOX>(h, grid, stream);
    else launch_shape<OVERLAP_SPHERE>(h, grid, stream);
}

}  // namespace ptk
