// HIP kernel for gfx950 of overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres): for every caller
// box or sphere the number of triangles that meet it and the smallest of their indices.  The shape is closest_kernel's
// (ptk_closest.hip) - one-wave workgroups, one query per lane, the query arrays staged through LDS, the per-lane LDS stack of links -
// around a third kind of walk of the 4-wide quantised BVH: the region is fixed, so nothing is ordered and no bound moves; a child
// survives or it does not.  Compiled once, with -ffp-contract=off: the triangle arm is the rule of ptk.h operation by operation (the
// numpy restatement is tests/overlap_rule.py); the box arm is acceleration only, behind the slack derived in DESIGN.md §4.27.
#include "ptk_device_fn.h"
#include "ptk_overlap.h"
#include "ptk.h"
#ifdef PTK_DEBUG
#include <cassert>
#endif

namespace ptk {

#define PTK_OVERLAP_BLOCK 64        // one wave per workgroup, one query per lane
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

// d2k of ptk_closest_points' rule for one record, bit for bit (ptk_closest.hip closest_tri up to dot(d, d): the same operations in
// the same order; that kernel is left as it is).
__device__ __forceinline__ float closest_d2(const v3 p, const v3 a, const v3 e1, const v3 e2)
{
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
    const float den = (va + vb) + vc;
    const bool useA = (reg == 3) | (reg == 7), useB = reg >= 4;
    const float numA = reg == 3 ? d1 : vb, denA = reg == 3 ? d1 - d3 : den;
    const float numB = reg == 4 ? d2 : (reg == 5 ? e43 : vc), denB = reg == 4 ? d2 - d6 : (reg == 5 ? e43 + e56 : den);
    const float A = (useA ? numA : 0.0f) / (useA ? denA : 1.0f), B = (useB ? numB : 0.0f) / (useB ? denB : 1.0f);
    float v = reg == 1 ? 1.0f : (reg == 5 ? 1.0f - B : (useA ? A : 0.0f));
    float w = reg == 2 ? 1.0f : (useB ? B : 0.0f);
    v = v > 0.0f ? v : 0.0f;
    v = v < 1.0f ? v : 1.0f;
    w = w > 0.0f ? w : 0.0f;
    const float top = 1.0f - v;
    w = w < top ? w : top;
    const v3 q = V((a.x + e1.x * v) + e2.x * w, (a.y + e1.y * v) + e2.y * w, (a.z + e1.z * v) + e2.z * w);
    const v3 d = sub(p, q);
    return dot(d, d);
}

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

// (sqrt(r2) * (1 + REL) + E)^2, rounded up: the squared box distance a child must exceed for a sphere query to drop it
__device__ __forceinline__ float sphere_prune_bound(float r2, float E)
{
    const float thr = __builtin_fmaf(__builtin_amdgcn_sqrtf(r2), 1.0f + PTK_OVERLAP_REL, E);
    return thr * thr * (1.0f + 0x1p-20f);
}

// SHAPE: OVERLAP_BOX / OVERLAP_SPHERE.  KT: the list's capacity, 0 = count only; H.k <= KT columns are written.
template <int SHAPE, int KT, bool STATS>
__global__ __launch_bounds__(PTK_OVERLAP_BLOCK) void overlap_kernel(const OverlapParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_OVERLAP_BLOCK];
    constexpr bool BOX = SHAPE == OVERLAP_BOX;
    const uint32_t lane = threadIdx.x;
    const uint32_t g0 = blockIdx.x * (uint32_t)PTK_OVERLAP_BLOCK;                   // < num <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_OVERLAP_BLOCK, (uint32_t)H.num - g0);
    const bool live = lane < n;
    const uint32_t i = g0 + lane;
    int* const stack = lds_stack + lane;
    float* const stage = (float*)lds_stack;
    static_assert(PTK_STACK_ROWS >= 6, "the staging area is three rows of the stack per array");
    static_assert(PTK_STACK_ROWS >= PTK_OVERLAP_MAX_K && KT <= PTK_OVERLAP_MAX_K, "a group's lists, 64 x 16 words, pass through the stack rows");

    // The group's lo / centers (and hi) are 3 n consecutive floats each: consecutive lanes read consecutive floats, through the rows
    // of the stack the walk does not use yet (stride 3 dwords on the way out: no two lanes of a half-wave on one bank).
    {
        const float* const ga = H.qa + (size_t)g0 * 3;
        const float* const gb = BOX ? H.qb + (size_t)g0 * 3 : nullptr;     // (a sphere's radius is one dword per lane, read below)
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t e = lane + k * PTK_OVERLAP_BLOCK;
            if (e < n * 3u)
            {
                stage[e] = ga[e];
                if (BOX) stage[3 * PTK_OVERLAP_BLOCK + e] = gb[e];
            }
        }
    }
    __syncthreads();
    const v3 A = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
    v3 B = V(0.0f, 0.0f, 0.0f);
    if (BOX && live) B = V(stage[3 * PTK_OVERLAP_BLOCK + lane * 3], stage[3 * PTK_OVERLAP_BLOCK + lane * 3 + 1], stage[3 * PTK_OVERLAP_BLOCK + lane * 3 + 2]);
    __syncthreads();                                                                // the rows are the stack from here on

    int from = 0;
    if (live && H.tri_from) from = max(H.tri_from[i], 0);
    // what the walk prunes with.  Boxes: the query box grown by E, against which a child's decoded planes are compared; c, h of
    // the rule.  Spheres: the squared bound, fixed for the whole walk; A is the centre, r2 the rule's
    bool walks;
    v3 c = V(0.0f, 0.0f, 0.0f), h = c, loE = c, hiE = c;
    float r2 = 0.0f, thr2 = 0.0f;
    if (BOX)
    {
        walks = live & (A.x <= B.x) & (A.y <= B.y) & (A.z <= B.z);                  // a reversed or NaN box accepts nothing
        c = V((A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f);
        h = V((B.x - A.x) * 0.5f, (B.y - A.y) * 0.5f, (B.z - A.z) * 0.5f);
        const float M = fmaxf(fmaxf(fmaxf(fabsf(A.x), fabsf(A.y)), fabsf(A.z)), fmaxf(fmaxf(fabsf(B.x), fabsf(B.y)), fabsf(B.z)));
        const float E = (M + H.scene_bound) * (PTK_OVERLAP_K * 0x1p-21f);
        loE = V(A.x - E, A.y - E, A.z - E); hiE = V(B.x + E, B.y + E, B.z + E);
    }
    else
    {
        float r = 0.0f;
        if (live) r = H.qb[i];
        walks = live & (r > 0.0f);                                                  // a NaN, zero or negative radius accepts nothing
        r2 = r * r;
        const float E = (fmaxf(fmaxf(fabsf(A.x), fabsf(A.y)), fabsf(A.z)) + H.scene_bound) * (PTK_OVERLAP_K * 0x1p-21f);
        thr2 = sphere_prune_bound(r2, E);
    }

    OverlapList<KT> L;
    L.clear();
    int count = 0;
    const float4* const nodes = uniform_ptr(H.nodes);
    const float4* const tris = uniform_ptr(H.tris);
    int node = walks ? 0 : NODE_EXIT;
    int* top = stack;
    uint32_t n_nodes = 0, n_tris = 0, n_past = 0;
    // the next deferred link, NODE_EXIT when there is none
#define PTK_OVERLAP_POP(into) { if (top == stack) into = NODE_EXIT; else { top -= PTK_OVERLAP_BLOCK; into = *top; } }
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
            // per child: plane = origin + q * scale (closest_kernel's decode).  An empty slot has an inverted box, lo = 255 and
            // hi = 0, which says nothing: its link does.  Every comparison is false for a NaN: nothing is dropped then
            bool in[4];
#define PTK_OVERLAP_CHILD(k, link)                                                                                                              \
            {                                                                                                                                   \
                const float lx = __builtin_fmaf((float)((lox >> (8 * k)) & 255u), q0.w, q0.x), hx = __builtin_fmaf((float)((hix >> (8 * k)) & 255u), q0.w, q0.x); \
                const float ly = __builtin_fmaf((float)((loy >> (8 * k)) & 255u), q1.x, q0.y), hy = __builtin_fmaf((float)((hiy >> (8 * k)) & 255u), q1.x, q0.y); \
                const float lz = __builtin_fmaf((float)((loz >> (8 * k)) & 255u), q1.y, q0.z), hz = __builtin_fmaf((float)((hiz >> (8 * k)) & 255u), q1.y, q0.z); \
                bool out;                                                                                                                       \
                if (BOX) out = (lx > hiE.x) | (hx < loE.x) | (ly > hiE.y) | (hy < loE.y) | (lz > hiE.z) | (hz < loE.z);                         \
                else                                                                                                                            \
                {                                                                                                                               \
                    const float dx = fmaxf(fmaxf(lx - A.x, A.x - hx), 0.0f), dy = fmaxf(fmaxf(ly - A.y, A.y - hy), 0.0f), dz = fmaxf(fmaxf(lz - A.z, A.z - hz), 0.0f); \
                    out = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz)) > thr2;                                                       \
                }                                                                                                                               \
                in[k] = ((link) != NODE_EXIT) & !out;                                                                                           \
            }
            PTK_OVERLAP_CHILD(0, link0) PTK_OVERLAP_CHILD(1, link1) PTK_OVERLAP_CHILD(2, link2) PTK_OVERLAP_CHILD(3, link3)
#undef PTK_OVERLAP_CHILD
            // the lane descends into its first survivor and defers the others: walk_step's pushes - every link is written at the
            // running top, which moves on only behind a link that stays - at most three per node, the discipline the builders'
            // stack_need counts (slot 0 is entered or dropped, never deferred)
            int next = in[0] ? link0 : (in[1] ? link1 : (in[2] ? link2 : link3));
            *top = link1; top += (in[1] & in[0]) ? PTK_OVERLAP_BLOCK : 0;
            *top = link2; top += (in[2] & (in[0] | in[1])) ? PTK_OVERLAP_BLOCK : 0;
            *top = link3; top += (in[3] & (in[0] | in[1] | in[2])) ? PTK_OVERLAP_BLOCK : 0;
#ifdef PTK_DEBUG                                                // (make EXTRA=-DPTK_DEBUG: DESIGN.md §4.17)
            assert(top - stack <= (PTK_STACK_ROWS - 1) * PTK_OVERLAP_BLOCK);
#endif
            if (!(in[0] | in[1] | in[2] | in[3])) PTK_OVERLAP_POP(next)
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
                const v3 a = V(t0.x, t0.y, t0.z), e1 = V(t0.w, t1.x, t1.y), e2 = V(t1.z, t1.w, t2.x);
                const int tri = __float_as_int(t2.y);
                bool ok;
                if (BOX)
                {
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
                    const float d2k = closest_d2(A, a, e1, e2);
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
            PTK_OVERLAP_POP(node)
        }
    }
#undef PTK_OVERLAP_POP

    if (STATS)
    {
        atomicAdd(H.stats, (unsigned long long)n_nodes);
        atomicAdd(H.stats + 1, (unsigned long long)n_tris);
        atomicAdd(H.stats + 2, (unsigned long long)count);
        atomicAdd(H.stats + 3, (unsigned long long)n_past);
        return;
    }
    if (H.count && live) H.count[i] = count;
    if (KT > 0 && H.list)
    {
        // The lists leave through the stack rows, free again: a group's part is one contiguous run of n * k indices, laid out in
        // LDS as it lies in memory - column c of lane l at l * k + c - and stored by consecutive lanes to consecutive addresses.
        // Column c is the list's slot KT - 1 - c: the smallest index first.
        const int K = min(__builtin_amdgcn_readfirstlane(H.k), KT);
        int* const out = lds_stack;
        const uint32_t nk = n * (uint32_t)K;
        const size_t at = (size_t)g0 * (uint32_t)K;
        const uint32_t mine = lane * (uint32_t)K;
        __syncthreads();                                                            // every lane's stack is done
#pragma unroll
        for (int j = 0; j < KT; j++)
        {
            const int col = KT - 1 - j;
            if (col < K && live) out[mine + (uint32_t)col] = L.key[j] == PTK_OVERLAP_FREE ? -1 : L.key[j];
        }
        __syncthreads();
        for (uint32_t e = lane; e < nk; e += PTK_OVERLAP_BLOCK) H.list[at + e] = out[e];
    }
}

template <int SHAPE>
static void launch_shape(const OverlapParams& h, const dim3 grid, hipStream_t stream)
{
    const dim3 block(PTK_OVERLAP_BLOCK);
    if (h.stats) hipLaunchKernelGGL((overlap_kernel<SHAPE, 0, true>), grid, block, 0, stream, h);
    else if (h.k <= 0 || !h.list) hipLaunchKernelGGL((overlap_kernel<SHAPE, 0, false>), grid, block, 0, stream, h);
    else if (h.k <= 4) hipLaunchKernelGGL((overlap_kernel<SHAPE, 4, false>), grid, block, 0, stream, h);
    else hipLaunchKernelGGL((overlap_kernel<SHAPE, 16, false>), grid, block, 0, stream, h);
}

void launch_overlap(const OverlapParams& h, hipStream_t stream)
{
    if (h.num <= 0 || h.num_nodes <= 0 || h.k < 0 || h.k > PTK_OVERLAP_MAX_K) return;
    const dim3 grid((unsigned)(((size_t)h.num + PTK_OVERLAP_BLOCK - 1) / PTK_OVERLAP_BLOCK));
    if (h.shape == OVERLAP_BOX) launch_shape<OVERLAP_BOX>(h, grid, stream);
    else launch_shape<OVERLAP_SPHERE>(h, grid, stream);
}

}  // namespace ptk
