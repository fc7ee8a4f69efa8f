// HIP kernels for gfx950 of closest-hit and occlusion queries along caller-supplied rays (include/ptk.h ptk_intersect_rays,
// ptk_occluded_rays).  Both are the walk of rays_kernel (ptk_rays.hip) with everything but the walk taken out: one-wave
// workgroups, the per-lane LDS stack, the node record kept in flight across iterations, the triangle arm voted by the wave - over
// the trace kernels' own device functions (ptk_device_fn.h: Walk, walk_step, tri_test, the RNG keys).  Compiled once, with
// -ffp-contract=off like the exact build: every operation is the IEEE operation of the exact trace kernel and the CPU oracle.
#include "ptk_device_fn.h"
#include "ptk_hits.h"

namespace ptk {

#define PTK_HITS_BLOCK 64           // one wave per workgroup, one ray per lane

// The rays of the workgroup - 64 consecutive ones, fewer in the last group - and each lane's walk to its end.
// OCCL: the shadow-ray exit of tri_test as it stands (Walk::occl_tri).  best.t = tmax bounds the candidates, best.tri < 0 keeps the
// tie arm (t == best.t & tri < best.tri) from firing, so the bound is strict, and occl_tri = PTK_NOHIT - a value no triangle has -
// makes the first accepted triangle end the walk: afterwards best.tri >= 0 exactly when some accepted triangle has t < tmax.  Which
// one the walk met first depends on the tree; whether there is one does not.
// Returns whether the lane has a ray; W.best holds the answer.
template <bool OCCL>
__device__ __forceinline__ bool hits_walk(const HitsParams& H, int* lds_stack, Walk& W, uint32_t& ray_i)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t ray0 = blockIdx.x * (uint32_t)PTK_HITS_BLOCK;                   // < num_rays <= 2^31 - 1
    const uint32_t n = min((uint32_t)PTK_HITS_BLOCK, (uint32_t)H.num_rays - ray0);
    const bool live = lane < n;
    ray_i = ray0 + lane;
    int* const stack = lds_stack + lane;

    // The group's origins and directions are 3 n consecutive floats each: consecutive lanes read consecutive floats (three
    // instructions per array instead of three of stride 12 B), through the rows of the stack the walk does not use yet.
    {
        float* const stage = (float*)lds_stack;
        static_assert(PTK_STACK_ROWS >= 6, "the staging area is six rows of the stack");
        const float* const go = H.origins + (size_t)ray0 * 3, * const gd = H.dirs + (size_t)ray0 * 3;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t e = lane + k * PTK_HITS_BLOCK;
            if (e < n * 3u) { stage[e] = go[e]; stage[3 * PTK_HITS_BLOCK + e] = gd[e]; }
        }
        __syncthreads();
        // (stride 3 dwords: no two lanes of a half-wave on one bank)
        const v3 ro = live ? V(stage[lane * 3], stage[lane * 3 + 1], stage[lane * 3 + 2]) : V(0.0f, 0.0f, 0.0f);
        const v3 rd = live ? V(stage[3 * PTK_HITS_BLOCK + lane * 3], stage[3 * PTK_HITS_BLOCK + lane * 3 + 1], stage[3 * PTK_HITS_BLOCK + lane * 3 + 2])
                           : V(0.0f, 0.0f, 1.0f);
        __syncthreads();                                                            // the rows are the stack from here on
        bool walks = live;
        float tmax = __builtin_inff();
        if (OCCL)
        {
            if (live && H.tmax) tmax = H.tmax[ray_i];
            walks = live & (tmax > 0.0f);                                           // a NaN, zero or negative bound admits nothing
        }
        W.occl_tri = OCCL ? PTK_NOHIT : -1;
        W.begin(ro, rd, walks ? H.num_nodes : 0, stack, H.scene_bound);             // (no nodes: done at once)
        if (OCCL) { W.best.t = tmax; W.best.tri = -1; }
    }

    // only the key counts: tri_test draws from no stream.  The key of ray 0 of sample `sample` of RNG pixel key_base + i
    Rng rng; rng.inc = 1u; rng.state = 0u;
    rng.key = hash32(H.sample + pixel_key(H.seed_lo, H.seed_hi, H.key_base + ray_i));
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };

    WalkParams WP;
    WP.nodes = uniform_ptr(H.nodes); WP.tris = uniform_ptr(H.tris); WP.shade = uniform_ptr(H.shade);
    WP.texinfo = uniform_ptr(H.texinfo); WP.texels = uniform_ptr(H.texels);
    WP.tri_thr = __builtin_amdgcn_readfirstlane(H.tri_thr); WP.shade_thr = 0; WP.gen_thr = 0;
    NodeRec nrec;
    request_node(WP, W, nrec);                                                      // one node record in flight across iterations (walk_step)
    while (__ballot(!W.done()))
    {
        // rays_kernel's vote: the triangle arm runs when enough lanes have triangles queued, and always when no lane has a node
        const int n_tq = __popcll(__ballot(W.tri_left > 0)), n_nr = __popcll(__ballot(W.node >= 0));
        const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));
        if (!W.done()) walk_step<false, PTK_HITS_BLOCK, true>(WP, W, rng, 0u, stack, cnt, run_tri_arm, &nrec);
    }
    return live;
}

// The closest accepted hit of every ray.  Only the outputs with a non-null pointer are stored (kernel arguments: uniform
// branches); 4-byte stores of consecutive lanes to consecutive addresses, the barycentrics dealt to that shape by two shuffles.
__global__ __launch_bounds__(PTK_HITS_BLOCK) void hits_kernel(const HitsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_HITS_BLOCK];
    Walk W;
    uint32_t i;
    const bool live = hits_walk<false>(H, lds_stack, W, i);
    const bool hit = live & (W.best.tri != PTK_NOHIT);
    if (H.tri && live) H.tri[i] = hit ? W.best.tri : -1;
    if (H.t && live) H.t[i] = hit ? W.best.t : __builtin_inff();
    if (H.material && live)
        H.material[i] = hit ? (__float_as_int(ldg4(H.shade + (size_t)W.best.tri * SHADE_F4).w) & 0x7fffffff) : -1;
    if (H.bary)
    {
        const uint32_t lane = threadIdx.x, ray0 = blockIdx.x * (uint32_t)PTK_HITS_BLOCK;
        const uint32_t n = min((uint32_t)PTK_HITS_BLOCK, (uint32_t)H.num_rays - ray0);
        const float u = hit ? W.best.u : 0.0f, v = hit ? W.best.v : 0.0f;
        float* const gb = H.bary + (size_t)ray0 * 2;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++)
        {
            const uint32_t e = lane + k * PTK_HITS_BLOCK;                           // float e of the group's 2 n: u or v of ray e / 2
            const float su = __shfl(u, (int)(e >> 1)), sv = __shfl(v, (int)(e >> 1));
            if (e < n * 2u) gb[e] = (e & 1u) ? sv : su;
        }
    }
}

// Whether some accepted triangle lies nearer than tmax, per ray
__global__ __launch_bounds__(PTK_HITS_BLOCK) void occluded_kernel(const HitsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_HITS_BLOCK];
    Walk W;
    uint32_t i;
    const bool live = hits_walk<true>(H, lds_stack, W, i);
    if (live) H.occluded[i] = W.best.tri >= 0 ? 1 : 0;
}

static dim3 hits_grid(const HitsParams& h) { return dim3((unsigned)(((size_t)h.num_rays + PTK_HITS_BLOCK - 1) / PTK_HITS_BLOCK)); }

void launch_hits(const HitsParams& h, hipStream_t stream)
{
    if (h.num_rays <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(hits_kernel, hits_grid(h), dim3(PTK_HITS_BLOCK), 0, stream, h);
}

void launch_occluded(const HitsParams& h, hipStream_t stream)
{
    if (h.num_rays <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(occluded_kernel, hits_grid(h), dim3(PTK_HITS_BLOCK), 0, stream, h);
}

}  // namespace ptk
