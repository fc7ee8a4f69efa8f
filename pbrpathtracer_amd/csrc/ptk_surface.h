// Surface sampling (include/ptk.h ptk_sample_surface): the parameter blocks and launchers of the kernels in ptk_surface.hip - the
// weight table, its quantisation, the exact prefix sum and the sampler.
#pragma once

#include "ptk_device.h"

namespace ptk {

// words of the table build's reduction block (the first two come back to the host, eight bytes)
enum { SURF_RED_MAX = 0, SURF_RED_FLAG = 1, SURF_RED_DRAWABLE = 2, SURF_RED_CHECK = 3, SURF_RED_WORDS = 4 };     // (CHECK: ptk_surface_weights_device's own)
// bits of SURF_RED_FLAG
enum { SURF_FLAG_AREA = 1, SURF_FLAG_WEIGHT = 2 };

// items one workgroup of the production scan takes: 256 threads x 16
constexpr int SURF_SCAN_ITEMS = 4096;
// variants of surface_sample_kernel: speed only, every variant computes the same bits
enum { SURF_VARIANT_PLAIN = 0, SURF_VARIANT_COARSE = 1, SURF_VARIANT_COUNT = 2 };

// a_i of the rule per triangle, as the bit pattern of a float in the low word of table[i]; red[SURF_RED_MAX] = the largest pattern,
// red[SURF_RED_FLAG] |= what went wrong.  red is zeroed by the caller.
void launch_surface_weights(const float* d_verts, const float* d_weights, int num_tris, uint64_t* d_table, uint32_t* d_red, hipStream_t stream);
// table[i] = q_i = trunc(a_i * 2^shift) in place; red[SURF_RED_DRAWABLE] += triangles with q_i > 0
void launch_surface_quantise(uint64_t* d_table, int num_tris, int shift, uint32_t* d_red, hipStream_t stream);
// table[num_tris + k] = every ceil(num_tris / 1024)-th inclusive sum, k < SURF_COARSE_WORDS: the COARSE variant's table
constexpr int SURF_COARSE_WORDS = 1024;
void launch_surface_coarse(uint64_t* d_table, int num_tris, hipStream_t stream);
// device check of a weight array of the caller's: *d_flag |= SURF_FLAG_WEIGHT for a negative or non-finite element
void launch_surface_check_weights(const float* d_weights, int num_tris, uint32_t* d_flag, hipStream_t stream);

// words of `sums` an inclusive scan of n items at `items` per workgroup needs (every level's workgroup sums)
size_t scan_u64_sums(size_t n, int items);
// out[i] = in[0] + .. + in[i] mod 2^64, reduce-then-scan in separate launches: per-workgroup sums, their scan (this function again
// while more than one workgroup is left), the add-back.  in == out is allowed.  items >= 2.
void launch_scan_u64(const uint64_t* d_in, uint64_t* d_out, size_t n, int items, uint64_t* d_sums, hipStream_t stream);

// By value.  One sample per thread; the kernel writes every output that is not null.
struct SurfaceSampleParams {
    const uint64_t* incl;       // [num_tris] inclusive sums of q; incl[num_tris - 1] = total > 0
    const float* verts;         // [num_tris][9] resident world-space vertices
    const float4* shade;        // the shading records: s0 = (face normal, material | smoothing << 31)
    int32_t* tri;               // [num]
    float* bary;                // [num][2]
    float* position;            // [num][3]
    float* normal;              // [num][3]
    int32_t* material;          // [num]
    int num;                    // > 0
    int num_tris;               // > 0
    uint32_t key_base, sample, seed_lo, seed_hi;
};
void launch_surface_sample(const SurfaceSampleParams& p, int variant, hipStream_t stream);

}  // namespace ptk
