// Geometry updates after ptk_upload_scene (include/ptk.h ptk_update_geometry): launchers of the kernels in ptk_refit.hip.
// The tree keeps its links; records are repacked in place and the child boxes refitted bottom-up, one launch per level.
#pragma once

#include "ptk_device.h"

namespace ptk {

// words of the bounds reduction (all folded with atomicMax from 0): [0..2] ~enc(min.xyz), [3..5] enc(max.xyz) in the
// order-preserving encoding of bvh_device.hip, [6] bits of max |coordinate|, [7] != 0: a coordinate is not finite or
// reaches 2^61
constexpr int GEO_RED_WORDS = 8;

// tri_pos[tri] = position of triangle tri's record in the leaf order, from the index each record carries
void launch_inverse_order(const float4* d_tris, int32_t* d_tri_pos, int n, hipStream_t stream);
// bounds of the scene as it WOULD be with triangles [first, first + count) taken from `staged`: nothing is written but `red`
void launch_geometry_bounds(const float* d_verts, const float* d_staged, int first, int count, int n, uint32_t* d_red, hipStream_t stream);
// staged [count][9] arrays -> resident vertices, intersection records (leaf order; flat_tris in index order when not null)
// and, when normals / tbn are given, the shading records; only the words an upload derives from those arrays are written
void launch_repack_geometry(const float* d_staged_verts, const float* d_staged_normals, const float* d_staged_tbn, int first, int count,
                            float* d_verts, const int32_t* d_tri_pos, float4* d_tris, float4* d_flat_tris, float4* d_shade, hipStream_t stream);
// v1 v2 v3 of the light records whose triangle lies in the range, from the resident vertices
void launch_repack_lights(const float* d_verts, int first, int count, float4* d_lights, int num_lights, hipStream_t stream);
// One level of the refit: one thread per node of level_nodes[0 .. count).  Child boxes: leaves from the resident vertices,
// interior children from d_side (2 float4 per node: union min + the node's summed child half-area, union max), which the
// level below wrote.  write_nodes = 0 only measures (d_side is written, the node records are not).
void launch_refit_level(const int32_t* d_level_nodes, int count, float4* d_nodes, const float4* d_tris, const float* d_verts, float4* d_side,
                        float pad, int write_nodes, hipStream_t stream);
// SAH cost = sum over nodes of child half-area / root half-area, added in a fixed order (deterministic): one partial sum per 256
// nodes into d_partial ((num_nodes + 255) / 256 doubles), then one workgroup over those
void launch_refit_cost(const float4* d_side, int num_nodes, double* d_partial, double* d_cost, hipStream_t stream);

}  // namespace ptk
