// Radiance along caller-supplied rays (include/ptk.h ptk_trace_rays): parameter blocks and launchers of the kernels in ptk_rays.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// What rays_kernel needs beside the scene half of RenderParams.  Of that block it reads the scene tables, the scheduling
// thresholds, max_depth, the seed, and - with the meaning they have for a render pass - samples, chunk, num_chunks, num_items,
// first_sample (of this pass) and spp (of this pass).
struct RaysParams {
    const float* origins;       // [num_rays][3]
    const float* dirs;          // [num_rays][3], unit length (the caller's business)
    int num_rays;
    uint32_t key_base;          // ray i draws from the streams of RNG pixel key_base + i (mod 2^32)
    int lens_draws;             // 1: every stream starts behind the two SampleCircle draws of a camera ray
    const uint32_t* keys;       // [num_rays] or null; not null: ray i draws from the streams of RNG pixel keys[i] (rays_keyed_kernel)
};

// One launch's device block: the item counter on a 128-B line of its own, then the parameters, which the kernel reads through the
// constant address space like the trace kernels read theirs (ptk_device.h, queue block).  Written by a one-wave kernel on the
// stream ahead of every launch, which also zeroes the counter.
struct RaysBlock {
    unsigned counter;
    unsigned pad[31];
    RenderParams p;
    RaysParams r;
};

// items = ceil(num_rays / 64) * p.num_chunks; p.samples holds items * p.chunk * 64 float4
void launch_rays(const RenderParams& p, const RaysParams& r, RaysBlock* block, int resident_waves, hipStream_t stream);
// out[i] = (((add ? out[i] : 0) + sample 0 of ray i) + sample 1) + ... over the spp samples of the pass, in float32
void launch_rays_fold(const float4* samples, float* out, int num_rays, int chunk, int num_chunks, uint32_t spp, int add, hipStream_t stream);

}  // namespace ptk
