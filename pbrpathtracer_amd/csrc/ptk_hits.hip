// HIP kernels for gfx950 of closest-hit and occlusion queries along caller-supplied rays (include/ptk.h ptk_intersect_rays,
// ptk_occluded_rays).  Both are the one-wave ray queries' shape and walk (ptk_query_walk.h: the walk of rays_kernel, ptk_rays.hip,
// with everything but the walk taken out) with the trace kernels' own triangle arm (ptk_device_fn.h: tri_test, the RNG keys).
// Compiled once, with -ffp-contract=off like the exact build: every operation is the IEEE operation of the exact trace kernel and
// the CPU oracle.
#include "ptk_query_walk.h"
#include "ptk_hits.h"

namespace ptk {

// The rays of the workgroup - 64 consecutive ones, fewer in the last group - and each lane's walk to its end.
// OCCL: the shadow-ray exit of tri_test as it stands (Walk::occl_tri).  best.t = tmax bounds the candidates, best.tri < 0 keeps the
// tie arm (t == best.t & tri < best.tri) from firing, so the bound is strict, and occl_tri = PTK_NOHIT - a value no triangle has -
// makes the first accepted triangle end the walk: afterwards best.tri >= 0 exactly when some accepted triangle has t < tmax.  Which
// one the walk met first depends on the tree; whether there is one does not.
// Returns the group, whose `live` says whether the lane has a ray; W.best holds the answer.
template <bool OCCL>
__device__ __forceinline__ QueryGroup hits_walk(const HitsParams& H, int* lds_stack, Walk& W)
{
    int* const stack = lds_stack + threadIdx.x;
    v3 ro, rd;
    const QueryGroup G = query_group<true>(lds_stack, H.num_rays, H.origins, ro, H.dirs, &rd);
    bool walks = G.live;
    float tmax = __builtin_inff();
    if (OCCL) walks = query_bound(G, H.tmax, tmax);
    W.occl_tri = OCCL ? PTK_NOHIT : -1;
    W.begin(ro, rd, walks ? H.num_nodes : 0, stack, H.scene_bound);                 // (no nodes: done at once)
    if (OCCL) { W.best.t = tmax; W.best.tri = -1; }

    // only the key counts: tri_test draws from no stream.  The key of ray 0 of sample `sample` of RNG pixel key_base + i
    Rng rng; rng.inc = 1u; rng.state = 0u;
    rng.key = hash32(H.sample + pixel_key(H.seed_lo, H.seed_hi, H.key_base + G.i));
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };           // (tri_test's argument; query_walk has the step's.  Neither is touched)

    // (the whole of WalkParams: tri_test reads the shade tables for opacity)
    WalkParams WP;
    WP.nodes = uniform_ptr(H.nodes); WP.tris = uniform_ptr(H.tris); WP.shade = uniform_ptr(H.shade);
    WP.texinfo = uniform_ptr(H.texinfo); WP.texels = uniform_ptr(H.texels);
    WP.tri_thr = __builtin_amdgcn_readfirstlane(H.tri_thr); WP.shade_thr = 0; WP.gen_thr = 0;
    query_walk(WP, W, stack, [&](const float4 t0, const float4 t1, const float4 t2, uint32_t) {
        return tri_test<false>(WP, W, t0, t1, t2, rng, 0u, cnt);
    });
    return G;
}

// The closest accepted hit of every ray.  Only the outputs with a non-null pointer are stored (kernel arguments: uniform
// branches); 4-byte stores of consecutive lanes to consecutive addresses, the barycentrics dealt to that shape by two shuffles.
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void hits_kernel(const HitsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    Walk W;
    const QueryGroup G = hits_walk<false>(H, lds_stack, W);
    const bool live = G.live;
    const uint32_t i = G.i;
    const bool hit = live & (W.best.tri != PTK_NOHIT);
    if (H.tri && live) H.tri[i] = hit ? W.best.tri : -1;
    if (H.t && live) H.t[i] = hit ? W.best.t : __builtin_inff();
    if (H.material && live)
        H.material[i] = hit ? (__float_as_int(ldg4(H.shade + (size_t)W.best.tri * SHADE_F4).w) & 0x7fffffff) : -1;
    if (H.bary)
    {
        const uint32_t lane = threadIdx.x, ray0 = G.first, n = G.n;
        const float u = hit ? W.best.u : 0.0f, v = hit ? W.best.v : 0.0f;
        float* const gb = H.bary + (size_t)ray0 * 2;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++)
        {
            const uint32_t e = lane + k * PTK_QUERY_BLOCK;                           // float e of the group's 2 n: u or v of ray e / 2
            const float su = __shfl(u, (int)(e >> 1)), sv = __shfl(v, (int)(e >> 1));
            if (e < n * 2u) gb[e] = (e & 1u) ? sv : su;
        }
    }
}

// Whether some accepted triangle lies nearer than tmax, per ray
__global__ __launch_bounds__(PTK_QUERY_BLOCK) void occluded_kernel(const HitsParams H)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_QUERY_BLOCK];
    Walk W;
    const QueryGroup G = hits_walk<true>(H, lds_stack, W);
    if (G.live) H.occluded[G.i] = W.best.tri >= 0 ? 1 : 0;
}

static dim3 hits_grid(const HitsParams& h) { return dim3((unsigned)(((size_t)h.num_rays + PTK_QUERY_BLOCK - 1) / PTK_QUERY_BLOCK)); }

void launch_hits(const HitsParams& h, hipStream_t stream)
{
    if (h.num_rays <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(hits_kernel, hits_grid(h), dim3(PTK_QUERY_BLOCK), 0, stream, h);
}

void launch_occluded(const HitsParams& h, hipStream_t stream)
{
    if (h.num_rays <= 0 || h.num_nodes <= 0) return;
    hipLaunchKernelGGL(occluded_kernel, hits_grid(h), dim3(PTK_QUERY_BLOCK), 0, stream, h);
}

}  // namespace ptk
