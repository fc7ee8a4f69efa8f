// Adaptive ray queries and lightmap bakes (include/ptk.h ptk_trace_rays_adaptive, ptk_bake_lightmap_adaptive): launchers of the
// kernels in ptk_rays_adaptive.hip.  The trace itself is rays_keyed_kernel (ptk_rays.hip) over the round's compacted rays.
#pragma once

#include "ptk_device.h"

namespace ptk {

// Compacted ray j <- ray i = list[j] (list null: i = j): origins, dirs, its RNG pixel keys_in[i] (keys_in null: key_base + i
// mod 2^32) and src[j] = i.
void launch_rays_gather(const uint32_t* list, uint32_t count, const float* origins_in, const float* dirs_in, const uint32_t* keys_in, uint32_t key_base,
                        float* origins, float* dirs, uint32_t* keys, uint32_t* src, hipStream_t stream);
// For compacted ray j < num_rays with i = src[j]: s1[i] = ((s1[i] + sample 0) + sample 1) + ..., s2[i] = ((s2[i] + sample 0 *
// sample 0) + ...) over the spp samples of the pass, in float32 (the sample buffer's layout: ptk_rays.hip); counts[i] += add_count.
void launch_rays_fold_moments(const float4* samples, const uint32_t* src, float* s1, float* s2, uint32_t* counts, int num_rays, int chunk,
                              int num_chunks, uint32_t spp, uint32_t add_count, hipStream_t stream);
// The rule of ptk_render_adaptive for compacted ray j < count, i = src[j]: open = !done(s1[i], s2[i], counts[i], threshold).
// need null: keep[j] = open.  Otherwise need[texel[i]] = open (a byte plane over the lightmap's texels).
void launch_rays_converge(const uint32_t* src, uint32_t count, const float* s1, const float* s2, const uint32_t* counts, float threshold,
                          uint32_t* keep, uint8_t* need, const uint32_t* texel, hipStream_t stream);
// keep[j] = some texel of the 3x3 neighbourhood of texel[src[j]], clipped to the map, has need set
void launch_bake_keep(const uint32_t* src, uint32_t count, const uint32_t* texel, const uint8_t* need, int width, int height, uint32_t* keep,
                      hipStream_t stream);
// list <- the src[j] with keep[j] != 0, in ascending j; *total <- their number.  block_counts: one word per 256 rays.
void launch_rays_compact(const uint32_t* src, const uint32_t* keep, uint32_t count, uint32_t* block_counts, uint32_t* total, uint32_t* list,
                         hipStream_t stream);
// out[texel[i]] = counts[i] for i < count
void launch_bake_scatter_counts(const uint32_t* counts, const uint32_t* texel, uint32_t count, uint32_t* out, hipStream_t stream);

}  // namespace ptk
