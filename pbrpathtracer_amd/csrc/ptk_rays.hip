// HIP kernels for gfx950 of radiance queries along caller-supplied rays (include/ptk.h ptk_trace_rays).  rays_kernel is the BVH
// variant of trace_kernel (ptk_kernels.hip) with its camera-ray block taken out: the same persistent one-wave workgroups, the
// same voted state machine over the same device functions (ptk_device_fn.h: Walk, walk_step with the node record kept in flight,
// shade_interaction), a path's first ray read from the caller's arrays instead of generated.  Compiled once, with
// -ffp-contract=off like the exact build: every operation is the IEEE operation of the exact trace kernel and the CPU oracle.
#include <algorithm>

#include "ptk_device_fn.h"
#include "ptk_rays.h"

namespace ptk {

#define PTK_RAYS_BLOCK 64           // one wave per workgroup
#define PTK_RAYS_WAVES 4            // waves per SIMD the register allocator must allow (trace_kernel's BVH variant: PTK_TRACE_WAVES_BVH)

// the current work item, in LDS: read only when units are dealt
enum { RI_UNITS = 0,    // rays x samples of the item; 0: the counter has run past the last item
       RI_N,            // its rays (64, fewer in the last group)
       RI_MAGIC,        // ceil(2^32 / rays): unit / rays = mulhi(unit, magic), exact while unit * rays < 2^32
       RI_RAY0, RI_SBEGIN, RI_OUTBASE, RI_WORDS };

enum : int { ST_NEED = 0, ST_TRAV = 2, ST_SHADE = 3, ST_DONE = 4 };

// Work item = (64 consecutive rays, chunk of samples), the chunks of one group of rays being consecutive items; its work UNITS =
// (ray, sample), sample-major, dealt to whichever lane needs one.  Items are popped from ONE counter: an item is 256 or 512 paths,
// so the chip pops a few items per microsecond, far below what one word sustains.
// Sample buffer: P.samples[(item * chunk + sample in chunk) * 64 + ray in group].
#define PTK_RAYS_KERNEL rays_kernel
#define PTK_RAYS_KEYED 0
#include "ptk_rays_kernel.h"
#undef PTK_RAYS_KERNEL
#undef PTK_RAYS_KEYED
#define PTK_RAYS_KERNEL rays_keyed_kernel
#define PTK_RAYS_KEYED 1
#include "ptk_rays_kernel.h"
#undef PTK_RAYS_KERNEL
#undef PTK_RAYS_KEYED

// Folds the samples of one pass into out, strictly in sample order: one thread per ray, so that consecutive lanes read
// consecutive float4 of the sample buffer.
__global__ __launch_bounds__(PTK_BLOCK) void rays_fold_kernel(const float4* __restrict__ samples, float* __restrict__ out, int num_rays,
                                                              int chunk, int num_chunks, uint32_t spp, int add_to_out)
{
    const size_t i = (size_t)blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= (size_t)num_rays) return;
    float* o = out + i * 3;
    v3 acc = add_to_out ? V(o[0], o[1], o[2]) : V(0.0f, 0.0f, 0.0f);
    const float4* s = samples + (i >> 6) * (size_t)num_chunks * (size_t)chunk * 64 + (i & 63);
    // sample k of the pass (chunk k / chunk, sample k % chunk of it) sits at s[k * 64]: the chunks of a group are consecutive
    // items.  Eight loads in flight per lane, added strictly in sample order (accumulate_kernel's loop).
    uint32_t k = 0;
    for (; k + 8 <= spp; k += 8)
    {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = s[(size_t)(k + j) * 64];
#pragma unroll
        for (int j = 0; j < 8; j++) acc = add(acc, V(v[j].x, v[j].y, v[j].z));
    }
    for (; k < spp; k++)
    {
        const float4 v = s[(size_t)k * 64];
        acc = add(acc, V(v.x, v.y, v.z));
    }
    o[0] = acc.x; o[1] = acc.y; o[2] = acc.z;
}

__global__ void rays_init_kernel(RaysBlock* block, const RenderParams p, const RaysParams r)
{
    static_assert(sizeof(RenderParams) % 4 == 0 && sizeof(RaysParams) % 4 == 0, "copied word by word");
    const int t = threadIdx.x;
    const uint32_t* sp = (const uint32_t*)&p; uint32_t* dp = (uint32_t*)&block->p;
    for (int i = t; i < (int)(sizeof(RenderParams) / 4); i += 64) dp[i] = sp[i];
    const uint32_t* sr = (const uint32_t*)&r; uint32_t* dr = (uint32_t*)&block->r;
    for (int i = t; i < (int)(sizeof(RaysParams) / 4); i += 64) dr[i] = sr[i];
    if (t == 0) block->counter = 0u;
}

void launch_rays(const RenderParams& p, const RaysParams& r, RaysBlock* block, int resident_waves, hipStream_t stream)
{
    if (p.num_items <= 0) return;
    hipLaunchKernelGGL(rays_init_kernel, dim3(1), dim3(64), 0, stream, block, p, r);
    // persistent waves: as many one-wave workgroups as the chip holds at once, or one per item where there are fewer
    const int blocks = std::min(p.num_items, resident_waves / 16 * 4 * PTK_RAYS_WAVES);
    if (r.keys) hipLaunchKernelGGL(rays_keyed_kernel, dim3(blocks), dim3(PTK_RAYS_BLOCK), 0, stream, block);
    else hipLaunchKernelGGL(rays_kernel, dim3(blocks), dim3(PTK_RAYS_BLOCK), 0, stream, block);
}

void launch_rays_fold(const float4* samples, float* out, int num_rays, int chunk, int num_chunks, uint32_t spp, int add, hipStream_t stream)
{
    if (num_rays <= 0) return;
    hipLaunchKernelGGL(rays_fold_kernel, dim3((num_rays + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, samples, out, num_rays,
                       chunk, num_chunks, spp, add);
}

}  // namespace ptk
